// Backward of the global self-attention core (k_global_attn, attn.hip; MaskedMHA global branch with q = k = v's sequence,
// blocks.py:374-393) and its export, include/decafnet_hip_attn.h.
//
// Per sequence b, head h, d = C / heads, scale = d^-1/4 on q and on k:
//   s_tj = (scale q_t) . (scale k_j)   over the keys j < T with mask[b, j] != 0; a masked key is excluded exactly (-inf)
//   p_t. = softmax_j s_tj,  O_t = sum_j p_tj v_j
//   dP_tj = dO_t . v_j,  delta_t = sum_j p_tj dP_tj,  dS_tj = p_tj (dP_tj - delta_t)
//   dV_j = sum_t p_tj dO_t,  dQ_t = scale^2 sum_j dS_tj k_j,  dK_j = scale^2 sum_t dS_tj q_t
// The mask masks KEYS only: a padded query row is an ordinary row (it has an output, takes a dQ and feeds dK / dV with whatever dO
// holds there); at a padded key dK = dV = 0 exactly.  A sequence without a valid key has O = 0 in the forward (the reference has NaN
// there): its dQ = dK = dV = 0, a defined deviation.
//
// Two kernels with the forward's layout (thread (row = tid >> 2, part = tid & 3) of a 64-row tile: the row's d channels of one head
// in registers, 16 of the 64 columns of the score tile, a quarter of the d output channels; tiles go through LDS):
//   k_gattn_bwd_q  : a workgroup per (64 queries, head, sequence).  Pass 1 walks the key tiles: scores and dP, the softmax statistics
//                    carried online (running maximum m, running sum l, running sum of e * dP); it leaves (m, 1 / l, delta) per
//                    (row, head) in scratch.  Pass 2 walks them again: p = exp(s - m) / l, dS through LDS, dQ.
//   k_gattn_bwd_kv : a workgroup per (64 keys, head, sequence).  It walks the query tiles in ascending t with q (times scale^2) and
//                    dO in LDS, reads the three statistics, forms the same s and dP (the same fma chain over the channels on the same
//                    operands: the same bits), and accumulates dV and dK in registers; both are written once.
// No atomics and one fixed summation order: equal inputs give equal bits, and every product and sum is linear in dO with nothing but
// roundings in between, so dO times a power of two gives that power of two times each output.  delta is formed from p and dP (not
// from a stored O) and m and 1 / l are kept apart, for the reasons at the top of attn_grad.hip; the exponential carries its residual
// (exp_res, grad_common.h).  Every accumulation is written as an explicit fma, so what the compiler may contract does not depend on which
// outputs are wanted: with one of dQ / dK / dV absent the others keep their bits.
//
// Arithmetic: fp32 on the vector ALU, 2 T^2 C flops per product and nine products (the query side forms s and dP twice and dQ, the key
// side s and dP a third time, dV and dK): 4.5x the forward's two.  LDS: two 64 x (d + 4) operand tiles and one 64 x 68 score tile,
// 52 KB at d = 64.
#include "global_attn_grad.h"

#include "../../include/decafnet_hip_attn.h"
#include "grad_common.h"

namespace dcf {

constexpr int GG_TILE = 64;           // rows of a query tile and of a key tile
constexpr int GG_PP = GG_TILE + 4;    // row pitch of the score tile

// stage rows [r0, r0 + 64) of head `hd` of X (rows past T read row T - 1: they are excluded by index, never by value), times `mul`
template <int D, bool MUL>
__device__ __forceinline__ void gg_stage(float* dst, const float* __restrict__ X, int64_t base, int r0, int T, int C, int hd, float mul, int tid) {
  constexpr int P = D + 4;
  for (int i = tid; i < GG_TILE * (D / 4); i += 256) {
    const int j = i / (D / 4), c4 = (i - j * (D / 4)) * 4;
    const int r = r0 + j < T ? r0 + j : T - 1;
    f32x4 x = *reinterpret_cast<const f32x4*>(X + (base + r) * C + hd * D + c4);
    if (MUL) { x.x *= mul; x.y *= mul; x.z *= mul; x.w *= mul; }
    *reinterpret_cast<f32x4*>(dst + j * P + c4) = x;
  }
}

// the dot product of a register row with row j of an LDS tile: ONE fma chain over the channels in ascending order, the same in both
// kernels (fma is symmetric in its factors, so which side sits in registers does not matter)
template <int D>
__device__ __forceinline__ float gg_dot(const float* reg, const float* tile_row) {
  float a = 0.f;
#pragma unroll
  for (int d = 0; d < D; d += 4) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(tile_row + d);
    a = __builtin_fmaf(reg[d], x.x, a); a = __builtin_fmaf(reg[d + 1], x.y, a);
    a = __builtin_fmaf(reg[d + 2], x.z, a); a = __builtin_fmaf(reg[d + 3], x.w, a);
  }
  return a;
}

// ------------------------------------------------------------------------------------------
// query side: statistics and dQ
// ------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void k_gattn_bwd_q(GlobalAttnGradArgs p) {
  constexpr int KP = D + 4, DP = D / 4;
  __shared__ float Ks[GG_TILE * KP], Vs[GG_TILE * KP], Ss[GG_TILE * GG_PP];
  __shared__ float valid[GG_TILE];
  const int tid = threadIdx.x, qi = tid >> 2, part = tid & 3;
  const int b = blockIdx.z, hd = blockIdx.y, q0 = blockIdx.x * GG_TILE;
  const int T = p.T, C = p.C;
  const int64_t base = (int64_t)b * T;
  const bool live = q0 + qi < T;
  const int qrow = live ? q0 + qi : T - 1;
  const float sc = 1.0f / sqrtf((float)D);               // scale^2: on q here, as the forward has it
  float q[D], g[D];
  {
    const float* qp = p.Q + (base + qrow) * C + hd * D;
    const float* gp = p.dO + (base + qrow) * C + hd * D;
#pragma unroll
    for (int d = 0; d < D; d += 4) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(qp + d), y = *reinterpret_cast<const f32x4*>(gp + d);
      q[d] = x.x * sc; q[d + 1] = x.y * sc; q[d + 2] = x.z * sc; q[d + 3] = x.w * sc;
      g[d] = y.x; g[d + 1] = y.y; g[d + 2] = y.z; g[d + 3] = y.w;
    }
  }
  // one loop over both passes, so that the score code exists once: pass 1 (it < nt) carries the statistics online, pass 2 forms dS
  // and dQ from the same expressions on the same operands, hence the same s and dP.  This thread's 16 keys of a tile are
  // j = 4 jj + part: neighbouring threads read neighbouring LDS rows.
  const int nt = (T + GG_TILE - 1) / GG_TILE;
  float m = -INFINITY, l = 0.f, Dn = 0.f, il = 0.f, delta = 0.f;
  float dq[DP];
#pragma unroll
  for (int d = 0; d < DP; ++d) dq[d] = 0.f;
  for (int it = 0; it < 2 * nt; ++it) {
    const bool second = it >= nt;                        // (uniform)
    const int k0 = (second ? it - nt : it) * GG_TILE;
    if (it == nt) {
      il = l > 0.f ? 1.0f / l : 0.f;                     // a sequence without a valid key: p = 0 everywhere
      delta = Dn * il;
      if (p.stats && live && part == 0)
        *reinterpret_cast<f32x4*>(p.stats + ((base + q0 + qi) * p.heads + hd) * 4) = f32x4{m, il, delta, 0.f};
      if (!p.dQ) break;
    }
    __syncthreads();                                     // the previous tile is consumed
    gg_stage<D, false>(Ks, p.K, base, k0, T, C, hd, 1.f, tid);
    gg_stage<D, false>(Vs, p.V, base, k0, T, C, hd, 1.f, tid);
    if (tid < GG_TILE) valid[tid] = (k0 + tid < T && (!p.mask || p.mask[base + k0 + tid] != 0)) ? 1.f : 0.f;
    __syncthreads();
    float s[16], dp[16];
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) {
      const int j = jj * 4 + part;
      s[jj] = gg_dot<D>(q, Ks + j * KP);
      dp[jj] = gg_dot<D>(g, Vs + j * KP);
      __builtin_amdgcn_sched_barrier(0);                 // one key at a time: hoisting every tile read to the top spills
    }
    if (!second) {
      float tmax = -INFINITY;
#pragma unroll
      for (int jj = 0; jj < 16; ++jj) tmax = valid[jj * 4 + part] != 0.f ? fmaxf(tmax, s[jj]) : tmax;
      tmax = fmaxf(tmax, dpp_self<DPP_XOR1>(tmax));
      tmax = fmaxf(tmax, dpp_self<DPP_XOR2>(tmax));
      const float mn = fmaxf(m, tmax);
      const float corr = m == -INFINITY ? 0.f : exp_res(m - mn);   // (nothing so far: nothing to rescale)
      float ls = 0.f, ds = 0.f;
#pragma unroll
      for (int jj = 0; jj < 16; ++jj) {
        const bool ok = valid[jj * 4 + part] != 0.f;
        const float e = ok ? exp_res(s[jj] - mn) : 0.f;
        ls += e;
        ds = ok ? __builtin_fmaf(e, dp[jj], ds) : ds;
      }
      ls += dpp_zero<DPP_XOR1>(ls); ls += dpp_zero<DPP_XOR2>(ls);   // the four threads of a query: the same sums in the same order
      ds += dpp_zero<DPP_XOR1>(ds); ds += dpp_zero<DPP_XOR2>(ds);
      l = __builtin_fmaf(l, corr, ls);
      Dn = __builtin_fmaf(Dn, corr, ds);
      m = mn;
      continue;
    }
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) {
      const int j = jj * 4 + part;
      const float pj = exp_res(s[jj] - m) * il;
      const float dsj = pj * (dp[jj] - delta);
      Ss[qi * GG_PP + j] = valid[j] != 0.f ? dsj : 0.f;
    }
    __syncthreads();
#pragma unroll 2
    for (int j = 0; j < GG_TILE; ++j) {
      const float dsj = Ss[qi * GG_PP + j];
#pragma unroll
      for (int d = 0; d < DP; d += 4) {
        const f32x4 kk = *reinterpret_cast<const f32x4*>(Ks + j * KP + part * DP + d);
        dq[d] = __builtin_fmaf(dsj, kk.x, dq[d]); dq[d + 1] = __builtin_fmaf(dsj, kk.y, dq[d + 1]);
        dq[d + 2] = __builtin_fmaf(dsj, kk.z, dq[d + 2]); dq[d + 3] = __builtin_fmaf(dsj, kk.w, dq[d + 3]);
      }
    }
  }
  if (!p.dQ) return;
  if (live) {
    float* op = p.dQ + (base + q0 + qi) * C + hd * D + part * DP;
#pragma unroll
    for (int d = 0; d < DP; d += 4) *reinterpret_cast<f32x4*>(op + d) = f32x4{dq[d] * sc, dq[d + 1] * sc, dq[d + 2] * sc, dq[d + 3] * sc};
  }
}

// ------------------------------------------------------------------------------------------
// key side: dK and dV over the query tiles in ascending t
// ------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void k_gattn_bwd_kv(GlobalAttnGradArgs p) {
  constexpr int QP = D + 4, DP = D / 4;
  __shared__ float Qs[GG_TILE * QP], Gs[GG_TILE * QP], Ps[GG_TILE * GG_PP];
  __shared__ f32x4 St[GG_TILE];
  const int tid = threadIdx.x, kj = tid >> 2, part = tid & 3;
  const int b = blockIdx.z, hd = blockIdx.y, k0 = blockIdx.x * GG_TILE;
  const int T = p.T, C = p.C;
  const int64_t base = (int64_t)b * T;
  const bool in_seq = k0 + kj < T;
  const int krow = in_seq ? k0 + kj : T - 1;
  const bool kvalid = in_seq && (!p.mask || p.mask[base + krow] != 0);
  const bool want_dk = p.dK != nullptr, want_dv = p.dV != nullptr;   // (uniform)
  const float sc = 1.0f / sqrtf((float)D);
  float k[D], v[D];
  {
    const float* kp = p.K + (base + krow) * C + hd * D;
    const float* vp = p.V + (base + krow) * C + hd * D;
#pragma unroll
    for (int d = 0; d < D; d += 4) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(kp + d), y = *reinterpret_cast<const f32x4*>(vp + d);
      k[d] = x.x; k[d + 1] = x.y; k[d + 2] = x.z; k[d + 3] = x.w;
      v[d] = y.x; v[d + 1] = y.y; v[d + 2] = y.z; v[d + 3] = y.w;
    }
  }
  float dk[DP], dv[DP];
#pragma unroll
  for (int d = 0; d < DP; ++d) { dk[d] = 0.f; dv[d] = 0.f; }

  for (int t0 = 0; t0 < T; t0 += GG_TILE) {
    __syncthreads();                                     // the previous tile is consumed
    gg_stage<D, true>(Qs, p.Q, base, t0, T, C, hd, sc, tid);        // q * scale^2: the query side's own product
    gg_stage<D, false>(Gs, p.dO, base, t0, T, C, hd, 1.f, tid);
    if (tid < GG_TILE)
      St[tid] = t0 + tid < T ? *reinterpret_cast<const f32x4*>(p.stats + ((base + t0 + tid) * p.heads + hd) * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    __syncthreads();
    float pj[16], ds[16];
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) {
      const int t = jj * 4 + part;
      const f32x4 st = St[t];
      const bool ok = kvalid && t0 + t < T;              // a padded QUERY row is live; rows past T are not rows
      const float s = gg_dot<D>(k, Qs + t * QP);
      pj[jj] = ok ? exp_res(s - st.x) * st.y : 0.f;
      if (want_dk) {
        const float dpj = gg_dot<D>(v, Gs + t * QP);
        ds[jj] = ok ? pj[jj] * (dpj - st.z) : 0.f;
      }
      __builtin_amdgcn_sched_barrier(0);                 // one query at a time, as on the query side
    }
    if (want_dv) {
#pragma unroll
      for (int jj = 0; jj < 16; ++jj) Ps[kj * GG_PP + jj * 4 + part] = pj[jj];
      __syncthreads();
#pragma unroll 2
      for (int t = 0; t < GG_TILE; ++t) {
        const float pt = Ps[kj * GG_PP + t];
#pragma unroll
        for (int d = 0; d < DP; d += 4) {
          const f32x4 gg = *reinterpret_cast<const f32x4*>(Gs + t * QP + part * DP + d);
          dv[d] = __builtin_fmaf(pt, gg.x, dv[d]); dv[d + 1] = __builtin_fmaf(pt, gg.y, dv[d + 1]);
          dv[d + 2] = __builtin_fmaf(pt, gg.z, dv[d + 2]); dv[d + 3] = __builtin_fmaf(pt, gg.w, dv[d + 3]);
        }
      }
    }
    if (want_dk) {
      if (want_dv) __syncthreads();                      // the probabilities are consumed
#pragma unroll
      for (int jj = 0; jj < 16; ++jj) Ps[kj * GG_PP + jj * 4 + part] = ds[jj];
      __syncthreads();
#pragma unroll 2
      for (int t = 0; t < GG_TILE; ++t) {
        const float dt = Ps[kj * GG_PP + t];
#pragma unroll
        for (int d = 0; d < DP; d += 4) {
          const f32x4 qq = *reinterpret_cast<const f32x4*>(Qs + t * QP + part * DP + d);
          dk[d] = __builtin_fmaf(dt, qq.x, dk[d]); dk[d + 1] = __builtin_fmaf(dt, qq.y, dk[d + 1]);
          dk[d + 2] = __builtin_fmaf(dt, qq.z, dk[d + 2]); dk[d + 3] = __builtin_fmaf(dt, qq.w, dk[d + 3]);
        }
      }
    }
  }
  if (!in_seq) return;
  const int64_t o = (base + k0 + kj) * C + hd * D + part * DP;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int d = 0; d < DP; d += 4) {                      // a padded key: exactly 0, whatever dO holds
    if (want_dk) *reinterpret_cast<f32x4*>(p.dK + o + d) = kvalid ? f32x4{dk[d], dk[d + 1], dk[d + 2], dk[d + 3]} : zero;
    if (want_dv) *reinterpret_cast<f32x4*>(p.dV + o + d) = kvalid ? f32x4{dv[d], dv[d + 1], dv[d + 2], dv[d + 3]} : zero;
  }
}

// ------------------------------------------------------------------------------------------
// launcher
// ------------------------------------------------------------------------------------------
int launch_global_attn_bwd(const GlobalAttnGradArgs& a, hipStream_t st) {
  const char* who = "global attention backward";
  DCF_CHECK(a.Q && a.K && a.V && a.dO, "%s: null operand", who);
  DCF_CHECK(a.B > 0 && a.T > 0 && a.heads > 0, "%s: empty batch (B=%d T=%d heads=%d)", who, a.B, a.T, a.heads);
  DCF_CHECK(a.C > 0 && a.C % a.heads == 0, "%s: C=%d not divisible by heads=%d", who, a.C, a.heads);
  const int D = a.C / a.heads;
  DCF_CHECK(D == 32 || D == 64, "%s: head dimension %d (32 or 64, the forward's)", who, D);
  DCF_CHECK(a.C <= 1024, "%s: C=%d (at most 1024)", who, a.C);
  DCF_CHECK(a.B <= 65535, "%s: B=%d sequences exceed one grid (65535)", who, a.B);
  DCF_CHECK((int64_t)a.B * a.T < (1ll << 31) - 64, "%s: %lld rows (< 2^31)", who, (long long)a.B * a.T);
  const bool kv = a.dK || a.dV;
  DCF_CHECK(!kv || a.stats, "%s: dK / dV need the row statistics scratch", who);
  if (!a.dQ && !kv) return 0;
  const dim3 grid((unsigned)((a.T + GG_TILE - 1) / GG_TILE), (unsigned)a.heads, (unsigned)a.B);
  const double prod = 2.0 * a.B * (double)a.T * a.T * a.C;
  ProfScope prof("global_attn_bwd", st, prod * ((a.dQ ? 5 : 2) + (kv ? 1 : 0) + (a.dK ? 2 : 0) + (a.dV ? 1 : 0)), 4.0 * 8.0 * a.B * (double)a.T * a.C);
  if (D == 64) {
    hipLaunchKernelGGL(k_gattn_bwd_q<64>, grid, dim3(256), 0, st, a);
    if (kv) hipLaunchKernelGGL(k_gattn_bwd_kv<64>, grid, dim3(256), 0, st, a);
  } else {
    hipLaunchKernelGGL(k_gattn_bwd_q<32>, grid, dim3(256), 0, st, a);
    if (kv) hipLaunchKernelGGL(k_gattn_bwd_kv<32>, grid, dim3(256), 0, st, a);
  }
  DCF_HIP(hipGetLastError());
  return 0;
}

}  // namespace dcf

extern "C" {

int dcf_attn_ext_version(void) { return DCF_ATTN_EXT_VERSION; }

int dcf_op_global_attn_bwd(const float* Q, const float* K, const float* V, const uint8_t* mask, const float* dO, float* dQ, float* dK,
                           float* dV, int32_t B, int32_t T, int32_t C, int32_t heads, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  dcf::GlobalAttnGradArgs a{Q, K, V, mask, dO, dQ, dK, dV, nullptr, B, T, C, heads};
  DCF_CHECK(B > 0 && T > 0 && heads > 0, "dcf_op_global_attn_bwd: empty batch (B=%d T=%d heads=%d)", B, T, heads);
  if (!dK && !dV) return dcf::launch_global_attn_bwd(a, st);
  // every shape check comes before the scratch: an unsupported shape allocates and launches nothing
  DCF_CHECK(C > 0 && C % heads == 0 && (C / heads == 32 || C / heads == 64),
            "dcf_op_global_attn_bwd: C=%d on %d heads: the head dimension must be 32 or 64 (the forward's)", C, heads);
  // the row statistics the key-side kernel reads: stream-ordered scratch, no host wait
  dcf::StreamScratch sc(st);
  if (sc.take(&a.stats, dcf::global_attn_grad_stats_floats((int64_t)B * T, heads))) return -1;
  return sc.end(dcf::launch_global_attn_bwd(a, st));
}

}  // extern "C"
