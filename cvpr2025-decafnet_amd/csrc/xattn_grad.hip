// Backward of the global cross-attention core (dcf_op_xattn, attn.hip; MaskedMHA global branch, libs/modeling/blocks.py:374-389) and
// the AdaLN modulation of a fusion decoder layer (blocks.py:643-645) with its backward.
//
// Cross attention, per sequence b, head h (head dimension d = C / heads), query row t < T, key j < Lk, scale = d^-1/4 on q and on k:
//   s_tj = (scale q_t) . (scale k_j)   over the keys with kvmask[b,j] != 0; a masked key contributes exactly 0 (masked_fill(-inf))
//   p_t. = softmax_j s_tj,  O_t = sum_j p_tj v_j
//   dP_tj = dO_t . v_j,  delta_t = sum_j p_tj dP_tj,  dS_tj = p_tj (dP_tj - delta_t)
//   dQ_t = scale^2 sum_j dS_tj k_j,  dK_j = scale^2 sum_t dS_tj q_t,  dV_j = sum_t p_tj dO_t
// There is no query mask (the reference's global branch has none): dO at every row is used.
//
// k_xattn_bwd: a workgroup of four waves owns (a slice of XG_SLICE_ROWS query rows, a head, a sequence).  It stages scale K_h and V_h
// in LDS once (Lk <= 64 rows of d + 4 floats) and walks its slice in batches of R = 1024 / d rows, three phases per batch:
//   load  : thread (row, channel quad) brings scale q and dO of the batch into LDS, one 16-byte load each;
//   row   : a wave per row, a lane per key: the two dot products against the lane's own K / V row (q, dO are LDS broadcasts), the
//           softmax and delta as wave reductions on DPP; p and dS of the row go to LDS.  The exponential carries its rounding residual
//           (exp_res, grad_common.h).  delta comes from p and dP, not from a stored O: with one key p = 1, delta = dP and dS = 0 exactly;
//   sum   : thread (row, channel quad) forms dQ of the batch (ascending j); thread (key group, channel quad) adds the batch's
//           dS q and p dO into its dK / dV accumulators -- d / 16 keys x 4 channels each, in registers for the whole slice, ascending t.
// At the end the accumulators go to scratch as the slice's partial; k_xg_reduce adds the slices of a sequence in the fixed blocked
// order of blocked_sum (grad_common.h).  No floating-point atomics, neither global nor LDS; the slicing is a constant, not a function of the device: results are bit-identical
// from run to run, and every product has dO as one factor, so a power-of-two scale of dO scales the results by exactly that.
//
// Arithmetic: fp32 on the vector ALU, five Lk x d products per row and head (scores, dP, dQ, dK, dV) = 10 Lk C flops per row against
// 12 C bytes of HBM traffic (q, dO in, dQ out): at Lk = 33 that is 27 flops per byte, above the machine balance of the fp32 vector
// rate -- the kernel is bound by the vector ALU and the LDS operand reads behind it, not by HBM (profiles/dec_grad.md).
//
// AdaLN, per row: Y = N(X m) * H[:, :C] + H[:, C:], N the affine-free channel LayerNorm (blocks.py:125-131, two-pass, eps 1e-5) or the
// identity (xattn_mode 'affine'); dH[:, :C] = dY * N(X m), dH[:, C:] = dY, dX = m LN'(dY * H[:, :C]).  Row-local: a wave per row as in
// rowops.hip, no reduction across rows.
#include <math.h>

#include "../../include/decafnet_hip.h"
#include "grad_common.h"
#include "xattn_grad.h"

namespace dcf {

// acc + s v and s v with the four channels written out: a vector-typed `s * v` lowers to packed fp32 instructions that broadcast the
// scalar through op_sel, the form tools/isa_gate.py keeps out of every object (profiles/r04_pkfma_hazard.md)
__device__ __forceinline__ f32x4 xg_fma_s(float s, const f32x4& v, const f32x4& acc) {
  return f32x4{__builtin_fmaf(s, v.x, acc.x), __builtin_fmaf(s, v.y, acc.y), __builtin_fmaf(s, v.z, acc.z), __builtin_fmaf(s, v.w, acc.w)};
}
__device__ __forceinline__ f32x4 xg_mul_s(float s, const f32x4& v) { return f32x4{s * v.x, s * v.y, s * v.z, s * v.w}; }

// ------------------------------------------------------------------------------------------
// cross attention backward
// ------------------------------------------------------------------------------------------
// LDS floats: K, V [Lk][D + 4], q, dO [R][D] (R D = 1024), p, dS [R][64]
template <int D>
static inline size_t xg_lds_bytes(int Lk) {
  return ((size_t)2 * Lk * (D + 4) + 2048 + (size_t)2 * (1024 / D) * 64) * sizeof(float);
}

template <int D>
__global__ __launch_bounds__(256) void k_xattn_bwd(XAttnGradArgs p) {
  constexpr int KP = D + 4;            // row pitch of K / V: 16-byte aligned, consecutive rows four banks apart
  constexpr int QN = D / 4;            // channel quads of a head
  constexpr int R = 256 / QN;          // rows of a batch = key groups of the accumulation (1024 / D)
  constexpr int NK = D / 16;           // keys of a thread in the accumulation: R NK = 64
  extern __shared__ __attribute__((aligned(16))) float s_xg[];
  const int Lk = p.Lk, C = p.C, T = p.T;
  float* Ks = s_xg;
  float* Vs = Ks + Lk * KP;
  float* qs = Vs + Lk * KP;
  float* gs = qs + 1024;
  float* Ps = gs + 1024;
  float* Ss = Ps + R * 64;
  const int s = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rr = tid / QN, c4 = 4 * (tid % QN);       // (row of the batch | key group, first channel of the quad)
  const float scale = 1.0f / sqrtf(sqrtf((float)D));
  const bool want_k = p.partK != nullptr, want_v = p.partV != nullptr, want_ds = p.dQ != nullptr || want_k;

  for (int i = tid; i < Lk * QN; i += 256) {
    const int j = i / QN, c = 4 * (i - j * QN);
    const int64_t src = ((int64_t)b * Lk + j) * C + h * D + c;
    st4(Ks + j * KP + c, xg_mul_s(scale, ld4(p.K + src)));
    st4(Vs + j * KP + c, ld4(p.V + src));
  }
  const bool valid = lane < Lk && (!p.kvmask || p.kvmask[(int64_t)b * Lk + (lane < Lk ? lane : 0)] != 0);
  const int jr = lane < Lk ? lane : Lk - 1;           // lanes beyond the text read an existing row and contribute 0
  const float* kr = Ks + jr * KP;
  const float* vr = Vs + jr * KP;

  f32x4 dk[NK], dv[NK];
#pragma unroll
  for (int i = 0; i < NK; ++i) { dk[i] = zero4(); dv[i] = zero4(); }

  const int t0 = s * XG_SLICE_ROWS, t_end = t0 + XG_SLICE_ROWS < T ? t0 + XG_SLICE_ROWS : T;
  for (int tb = t0; tb < t_end; tb += R) {
    const int nr = t_end - tb < R ? t_end - tb : R;
    const int64_t row = (int64_t)b * T + tb + rr;
    // load
    f32x4 q4 = zero4(), g4 = zero4();
    if (rr < nr) {
      q4 = xg_mul_s(scale, ld4(p.Q + row * C + h * D + c4));
      g4 = ld4(p.dO + row * C + h * D + c4);
    }
    st4(qs + rr * D + c4, q4);
    st4(gs + rr * D + c4, g4);
    __syncthreads();                                  // (the first pass: K / V are staged too)
    // row
    for (int r = wave; r < nr; r += 4) {
      const float* qr = qs + r * D;
      const float* gr = gs + r * D;
      float sc = 0.f, dp = 0.f;
#pragma unroll
      for (int c = 0; c < D; c += 4) sc += dotp(ld4(qr + c), ld4(kr + c));
      if (want_ds) {
#pragma unroll
        for (int c = 0; c < D; c += 4) dp += dotp(ld4(gr + c), ld4(vr + c));
      }
      sc = valid ? sc : -INFINITY;
      const float m = wave_max(sc);
      const float e = valid ? exp_res(sc - m) : 0.f;
      const float il = 1.0f / wave_sum(e);            // a sequence without a valid key: 0 / 0, undefined as in the forward
      const float pj = e * il;
      const float delta = wave_sum(pj * dp);
      Ps[r * 64 + lane] = pj;
      Ss[r * 64 + lane] = pj * (dp - delta);
    }
    __syncthreads();
    // sum
    if (p.dQ && rr < nr) {
      f32x4 acc = zero4();
      for (int j = 0; j < Lk; ++j) acc = xg_fma_s(Ss[rr * 64 + j], ld4(Ks + j * KP + c4), acc);
      st4(p.dQ + row * C + h * D + c4, xg_mul_s(scale, acc));
    }
    if (want_k || want_v) {
      for (int r = 0; r < nr; ++r) {
        const f32x4 qv = ld4(qs + r * D + c4), gv = ld4(gs + r * D + c4);
#pragma unroll
        for (int i = 0; i < NK; ++i) {
          const int j = rr + R * i;
          if (want_k) dk[i] = xg_fma_s(Ss[r * 64 + j], qv, dk[i]);
          if (want_v) dv[i] = xg_fma_s(Ps[r * 64 + j], gv, dv[i]);
        }
      }
    }
    __syncthreads();                                  // the next batch overwrites q, dO, p, dS
  }
#pragma unroll
  for (int i = 0; i < NK; ++i) {
    const int j = rr + R * i;
    if (j < Lk) {
      const int64_t dst = (((int64_t)b * p.S + s) * Lk + j) * C + h * D + c4;
      if (want_k) st4(p.partK + dst, xg_mul_s(scale, dk[i]));
      if (want_v) st4(p.partV + dst, dv[i]);
    }
  }
}

// out[b][i] = sum_s part[b][s][i], i < per = Lk C, the slices in the fixed blocked order of blocked_sum (grad_common.h)
__global__ __launch_bounds__(256) void k_xg_reduce(const float* __restrict__ part, float* __restrict__ out, int S, int64_t per, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int64_t b = i / per;
  const float* src = part + b * S * per + (i - b * per);
  float sum = 0.f;
  DCF_BLOCKED_SUM(sum, src, S, per, 0);
  out[i] = sum;
}

// d = 128 with more than 45 keys needs more than the 64 KiB of LDS a launch gets by default
template <int D>
static int xg_launch(const XAttnGradArgs& a, hipStream_t st) {
  const size_t lds = xg_lds_bytes<D>(a.Lk);
  if (lds > 64 * 1024) { if (int rc = raise_lds_limit<&k_xattn_bwd<D>>(lds)) return rc; }
  hipLaunchKernelGGL(k_xattn_bwd<D>, dim3(a.S, a.heads, a.B), dim3(256), lds, st, a);
  return 0;
}

// ------------------------------------------------------------------------------------------
// AdaLN modulation
// ------------------------------------------------------------------------------------------
template <int NCH, bool BWD>
__global__ __launch_bounds__(256) void k_adaln(AdaLnArgs p) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int C = p.C;
  const float inv_c = 1.0f / (float)C;
  for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < p.rows; r += (int64_t)gridDim.x * 4) {
    const bool live = !p.mask || p.mask[r] != 0;      // uniform: a wave owns the row
    Row<NCH> x;
    if (live) x.load(p.X + r * C, C, lane);
    else x.zero();
    float rs = 1.f;
    if (p.norm) {                                     // mean / rstd as row_layernorm (common.h) computes them; N(0) = 0
      const float mean = x.sum() * inv_c;
      float sq = 0.f;
#pragma unroll
      for (int j = 0; j < NCH; ++j) {
        if (256 * j + 4 * lane < C) {
          x.v[j] = f32x4{x.v[j].x - mean, x.v[j].y - mean, x.v[j].z - mean, x.v[j].w - mean};
          sq += (x.v[j].x * x.v[j].x + x.v[j].y * x.v[j].y) + (x.v[j].z * x.v[j].z + x.v[j].w * x.v[j].w);
        }
      }
      rs = 1.0f / sqrtf(wave_sum(sq) * inv_c + 1e-5f);
#pragma unroll
      for (int j = 0; j < NCH; ++j) x.v[j] = xg_mul_s(rs, x.v[j]);
    }
    const float* Hr = p.H + r * 2 * C;
    if constexpr (!BWD) {
      Row<NCH> sc, sh;
      sc.load(Hr, C, lane);
      sh.load(Hr + C, C, lane);
#pragma unroll
      for (int j = 0; j < NCH; ++j)
        x.v[j] = f32x4{__builtin_fmaf(x.v[j].x, sc.v[j].x, sh.v[j].x), __builtin_fmaf(x.v[j].y, sc.v[j].y, sh.v[j].y),
                       __builtin_fmaf(x.v[j].z, sc.v[j].z, sh.v[j].z), __builtin_fmaf(x.v[j].w, sc.v[j].w, sh.v[j].w)};
      x.store(p.Y + r * C, C, lane);
    } else {
      Row<NCH> g;
      g.load(p.dY + r * C, C, lane);
      if (p.dH) {
        Row<NCH> ds;
#pragma unroll
        for (int j = 0; j < NCH; ++j) ds.v[j] = f32x4{g.v[j].x * x.v[j].x, g.v[j].y * x.v[j].y, g.v[j].z * x.v[j].z, g.v[j].w * x.v[j].w};
        ds.store(p.dH + r * 2 * C, C, lane);
        g.store(p.dH + r * 2 * C + C, C, lane);
      }
      if (p.dX) {
        Row<NCH> o;
        o.zero();
        if (live) {
          Row<NCH> sc;
          sc.load(Hr, C, lane);
#pragma unroll
          for (int j = 0; j < NCH; ++j)                                       // d / d N(X m)
            o.v[j] = f32x4{g.v[j].x * sc.v[j].x, g.v[j].y * sc.v[j].y, g.v[j].z * sc.v[j].z, g.v[j].w * sc.v[j].w};
          if (p.norm) {
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
              const f32x4 dh = o.v[j], xh = x.v[j];
              s1 += (dh.x + dh.y) + (dh.z + dh.w);
              s2 += (dh.x * xh.x + dh.y * xh.y) + (dh.z * xh.z + dh.w * xh.w);
            }
            s1 = wave_sum(s1) * inv_c;
            s2 = wave_sum(s2) * inv_c;
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
              const f32x4 dh = o.v[j], xh = x.v[j];
              o.v[j] = f32x4{rs * ((dh.x - s1) - xh.x * s2), rs * ((dh.y - s1) - xh.y * s2), rs * ((dh.z - s1) - xh.z * s2), rs * ((dh.w - s1) - xh.w * s2)};
            }
          }
        }
        o.store(p.dX + r * C, C, lane);
      }
    }
  }
}

template <bool BWD>
static int adaln_launch(const AdaLnArgs& a, hipStream_t st) {
  const int64_t g = ((int64_t)a.rows + 3) / 4;
  const dim3 grid((unsigned)(g > (1 << 20) ? (1 << 20) : g));
  switch ((a.C + 255) / 256) {
    case 1: hipLaunchKernelGGL((k_adaln<1, BWD>), grid, dim3(256), 0, st, a); break;
    case 2: hipLaunchKernelGGL((k_adaln<2, BWD>), grid, dim3(256), 0, st, a); break;
    case 3: hipLaunchKernelGGL((k_adaln<3, BWD>), grid, dim3(256), 0, st, a); break;
    default: hipLaunchKernelGGL((k_adaln<4, BWD>), grid, dim3(256), 0, st, a);
  }
  DCF_HIP(hipGetLastError());
  return 0;
}

}  // namespace dcf

using namespace dcf;

extern "C" {

int dcf_op_xattn_bwd(const float* Q, const float* K, const float* V, const uint8_t* kvmask, const float* dO, float* dQ, float* dK,
                     float* dV, int32_t B, int32_t T, int32_t Lk, int32_t C, int32_t heads, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  DCF_CHECK(B > 0 && T > 0 && heads > 0, "dcf_op_xattn_bwd: empty batch (B = %d, T = %d, heads = %d)", B, T, heads);
  DCF_CHECK(Lk >= 1, "dcf_op_xattn_bwd: Lk = %d: a sequence needs at least one key", Lk);
  DCF_CHECK(Lk <= XG_MAX_LK, "dcf_op_xattn_bwd: Lk = %d keys (at most %d: a lane owns a key)", Lk, XG_MAX_LK);
  DCF_CHECK(Q && K && V && dO, "dcf_op_xattn_bwd: null operand");
  DCF_CHECK(C > 0 && C % 4 == 0 && C <= 1024 && C % heads == 0, "dcf_op_xattn_bwd: C = %d must be a multiple of 4 and of heads = %d, up to 1024", C,
            heads);
  const int d = C / heads;
  DCF_CHECK(d == 16 || d == 32 || d == 64 || d == 128, "dcf_op_xattn_bwd: head dimension %d (C = %d, heads = %d) is not one of 16, 32, 64, 128", d, C,
            heads);
  DCF_CHECK((int64_t)B * T < (1ll << 31) - 64 && B <= 65535, "dcf_op_xattn_bwd: %lld rows in %d sequences (< 2^31 rows, <= 65535 sequences)",
            (long long)B * T, B);
  DCF_CHECK(aligned16(Q) && aligned16(K) && aligned16(V) && aligned16(dO) && aligned16(dQ) && aligned16(dK) && aligned16(dV),
            "dcf_op_xattn_bwd: pointers must be 16-byte aligned");
  if (!dQ && !dK && !dV) return 0;
  XAttnGradArgs a{};
  a.Q = Q; a.K = K; a.V = V; a.kvmask = kvmask; a.dO = dO; a.dQ = dQ;
  a.B = B; a.T = T; a.Lk = Lk; a.C = C; a.heads = heads;
  a.S = (T + XG_SLICE_ROWS - 1) / XG_SLICE_ROWS;                                     // a fixed function of T
  const int64_t per = (int64_t)Lk * C, total = (int64_t)B * per;
  const size_t part_floats = (size_t)total * a.S;
  StreamScratch sc(st);
  if (dK && sc.take(&a.partK, part_floats)) return -1;
  if (dV && sc.take(&a.partV, part_floats)) return -1;
  int rc = 0;
  switch (d) {
    case 16: rc = xg_launch<16>(a, st); break;
    case 32: rc = xg_launch<32>(a, st); break;
    case 64: rc = xg_launch<64>(a, st); break;
    default: rc = xg_launch<128>(a, st);
  }
  if (rc == 0) {
    const dim3 grid((unsigned)((total + 255) / 256));
    if (dK) hipLaunchKernelGGL(k_xg_reduce, grid, dim3(256), 0, st, (const float*)a.partK, dK, a.S, per, total);
    if (dV) hipLaunchKernelGGL(k_xg_reduce, grid, dim3(256), 0, st, (const float*)a.partV, dV, a.S, per, total);
    if (hipGetLastError() != hipSuccess) { set_error("dcf_op_xattn_bwd: launch failed"); rc = -1; }
  }
  return sc.end(rc);
}

static int adaln_check(const char* what, int rows, int C) {
  DCF_CHECK(rows > 0, "%s: no rows", what);
  DCF_CHECK(C > 0 && C % 4 == 0 && C <= 1024, "%s: C = %d must be a multiple of 4 up to 1024", what, C);
  return 0;
}

int dcf_op_adaln(const float* X, const uint8_t* mask, const float* H, float* Y, int32_t rows, int32_t C, int32_t norm, void* stream) {
  DCF_CHECK(X && H && Y, "dcf_op_adaln: null argument");
  if (adaln_check("dcf_op_adaln", rows, C)) return -1;
  DCF_CHECK(aligned16(X) && aligned16(H) && aligned16(Y), "dcf_op_adaln: pointers must be 16-byte aligned");
  AdaLnArgs a{};
  a.X = X; a.mask = mask; a.H = H; a.Y = Y; a.rows = rows; a.C = C; a.norm = norm != 0;
  return adaln_launch<false>(a, (hipStream_t)stream);
}

int dcf_op_adaln_bwd(const float* X, const uint8_t* mask, const float* H, const float* dY, float* dX, float* dH, int32_t rows, int32_t C,
                     int32_t norm, void* stream) {
  DCF_CHECK(X && dY, "dcf_op_adaln_bwd: null argument");
  DCF_CHECK(!dX || H, "dcf_op_adaln_bwd: dX needs H");
  if (adaln_check("dcf_op_adaln_bwd", rows, C)) return -1;
  DCF_CHECK(aligned16(X) && aligned16(H) && aligned16(dY) && aligned16(dX) && aligned16(dH),
            "dcf_op_adaln_bwd: pointers must be 16-byte aligned");
  if (!dX && !dH) return 0;
  AdaLnArgs a{};
  a.X = X; a.mask = mask; a.H = H; a.dY = dY; a.dX = dX; a.dH = dH; a.rows = rows; a.C = C; a.norm = norm != 0;
  return adaln_launch<true>(a, (hipStream_t)stream);
}

}  // extern "C"
