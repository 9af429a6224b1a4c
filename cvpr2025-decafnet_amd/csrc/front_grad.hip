// vid_map of the training step on shared products (include/decafnet_hip_front.h): the first stage of the training forward
// (model.py:567-583) without the (B', T, Cin) input tensor, and its weight gradient.
//
//   forward   P1[b] = vid[b]^T W1^T, P2[b] = shallow[b]^T W2^T   once per video: the library's channel-major GEMM launches, the split
//             tile path (f16x3, weight planes split per call, row tiles under a closed gate skipped: GemmArgs::tile_skip) where its
//             shape constraints hold, the generic fp32 path otherwise;
//             Y[q,t,:] = bias + m ( g P1[b,t,:] + P2[b,t,:] + c w3 )   k_vidmap_combine (rowops.hip) with a row -> video table
//   backward  R1[b,t,:] = sum_{q in b} m g dY[q,t,:], R2 = sum_{q in b} m dY[q,t,:]   k_fg_rowsums: one pass over dY, which also leaves the
//             per-strip partial sums of db = sum dY and dw3 = sum m c dY
//             dW1[e,d] = sum_b sum_t R1[b,t,e] vid[b,d,t], dW2 from R2 and shallow       k_fg_wgrad
//
// k_fg_wgrad is k_wgrad of conv_grad.hip with the X operand channel-major: the reduction index t is CONTIGUOUS in X (four adjacent
// lanes read 128 contiguous bytes of one channel, a thread's 8 clips are one 16-byte vector per fp16 plane in LDS without a
// transposition) and strided in R (a thread reads 8 consecutive rows of one column, as k_wgrad reads dY).  f16x3: both operands
// split into (hi, lo) fp16 planes, three products; X pre-scaled by 2^4, R by the power of two conv_grad.h derives from the bits of
// max |R| (launch_absmax on R itself, a device word per half: no host wait).  A workgroup owns a 64 (e) x 64 (d) tile of dW and one
// slice of one video's clips; a slice is a whole number of 64-clip gate tiles, and a 32-clip chunk of a tile that no query of the
// video keeps takes no K step (R1 is zero there, so the bits do not depend on the skipping while vid is finite).  The fp32
// partials of the slices go to scratch and k_fg_reduce adds them in the fixed blocked order of blocked_sum (grad_common.h): no floating-point
// atomics, equal inputs give equal bits, and powers of two commute with every rounding here.
//
// The per-video query counts arrive as a host array; k_fg_tables receives them by value, 64 videos per launch, and writes the
// device tables (first row of every video, video of every row): no host memory is read after the call returns.
//
// Features stored as IEEE binary16 (include/decafnet_hip_front_half.h): dcf_op_vidmap_shared_h / dcf_op_vidmap_shared_bwd_h share
// everything above.  The forward products take the A_CHANMAJOR_H mode of the split tile path where it applies and one upcast into
// scratch otherwise; the weight gradient is k_fg_wgrad<true>, which reads the halves for every shape.  Both return the bits of the
// fp32 operators on the upcast values.
#include <type_traits>

#include "../../include/decafnet_hip_front.h"
#include "../../include/decafnet_hip_front_half.h"
#include "conv_grad.h"
#include "engine.h"
#include "front_grad.h"
#include "gemm.h"
#include "grad_common.h"
#include "rowops.h"

namespace dcf {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// a thread's 8 clips of X on their way to LDS: fp32 values one by one, or the 16 bytes of eight halves
template <bool HALF> struct FrontXRegs { float v[8]; };
template <> struct FrontXRegs<true> { f16x8 v; };

constexpr int FG_ROWS = 32;      // clips per LDS chunk (two k-steps of 16)
constexpr int FG_PITCH = 40;     // halfs per (plane, column): 32 clips + 8 pad = 80 B, every 16-byte vector stays aligned
constexpr float FG_SX = 16.f;    // feature pre-scale (conv_grad.hip WG_SX)
constexpr int FG_WANT_WGS = 2048; // workgroups the weight-gradient grid aims at (8 per CU) when it chooses the number of T slices
constexpr int FG_STRIP = 64;    // clips per workgroup of k_fg_rowsums (one partial of db / dw3 each)

struct FrontNq {
  int nq[FG_NQ_CHUNK];
  int v0, q0, n;
};

// qoff[v] = first row of video v (qoff[nvid] = B'), vtab[q] = video of row q, for the videos v0 .. v0 + n - 1 of this chunk
__global__ __launch_bounds__(64) void k_fg_tables(FrontNq c, int* __restrict__ qoff, int* __restrict__ vtab) {
  const int i = threadIdx.x;
  if (i >= c.n) return;
  int off = c.q0, mine = 0;
#pragma unroll
  for (int j = 0; j < FG_NQ_CHUNK; ++j) {         // (constant indices: a dynamically indexed by-value argument would go to scratch)
    off += j < i ? c.nq[j] : 0;
    mine = j == i ? c.nq[j] : mine;
  }
  qoff[c.v0 + i] = off;
  for (int k = 0; k < mine; ++k) vtab[off + k] = c.v0 + i;
  if (i == c.n - 1) qoff[c.v0 + c.n] = off + mine;
}

// flags[b][f] = some query of video b keeps a clip of 64 f .. 64 f + 63 (or all: every tile)
__global__ __launch_bounds__(64) void k_fg_tileflags(const float* __restrict__ gate, const int* __restrict__ qoff, uint8_t* __restrict__ flags,
                                                    int T, int ntiles, int all) {
  const int f = blockIdx.x, b = blockIdx.y, t = f * FG_TILE + threadIdx.x;
  bool any = all != 0;
  if (!any && t < T)
    for (int q = qoff[b]; q < qoff[b + 1]; ++q) any |= gate[(int64_t)q * T + t] != 0.f;
  const unsigned long long m = __ballot(any);
  if (threadIdx.x == 0) flags[(int64_t)b * ntiles + f] = m ? 1 : 0;
}

// the column groups of W (E, Cin) as compact matrices: W1c / W2c (E, D) for the generic GEMM (16-byte rows), w3c (E)
__global__ __launch_bounds__(256) void k_fg_unpack_w(const float* __restrict__ W, int Cin, int D, int E, float* __restrict__ W1c,
                                                    float* __restrict__ W2c, float* __restrict__ w3c) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= E * D) return;
  const int e = i / D, d = i - e * D;
  if (W1c) W1c[i] = W[(int64_t)e * Cin + d];
  if (W2c) W2c[i] = W[(int64_t)e * Cin + D + d];
  if (w3c && d == 0) w3c[e] = W[(int64_t)e * Cin + Cin - 1];
}

// One pass over dY.  Workgroup (strip s, video b): wave w takes the clips t0 + w, t0 + w + 4, ... of the strip, adds the rows of the
// video's queries in their order and writes R1[b,t,:] / R2[b,t,:]; the sums over ITS clips of dY (db) and m c dY (dw3) stay in
// registers, the four waves are added in a fixed order and go to part[(b nstrips + s)][2][E].
template <int NCH>
__global__ __launch_bounds__(256) void k_fg_rowsums(const float* __restrict__ dY, const float* __restrict__ gate, const uint8_t* __restrict__ mask,
                                                   const float* __restrict__ correl, const int* __restrict__ qoff, float* __restrict__ R1,
                                                   float* __restrict__ R2, float* __restrict__ part, int T, int E) {
  extern __shared__ float s_fg[];             // [4 waves][2][E]
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.y, t0 = blockIdx.x * FG_STRIP;
  const int t1 = t0 + FG_STRIP < T ? t0 + FG_STRIP : T;
  const int q0 = qoff[b], q1 = qoff[b + 1];
  Row<NCH> db, dw3;
  db.zero(); dw3.zero();
  for (int t = t0 + wave; t < t1; t += 4) {
    Row<NCH> r1, r2;
    r1.zero(); r2.zero();
    for (int q = q0; q < q1; ++q) {
      const int64_t row = (int64_t)q * T + t;
      Row<NCH> d;
      d.load(dY + row * E, E, lane);
      const float m = mask[row] ? 1.f : 0.f;
      const float mg = m * gate[row];
      const float mc = correl ? m * correl[row] : 0.f;
#pragma unroll
      for (int j = 0; j < NCH; ++j) {
        db.v[j] += d.v[j];
        r2.v[j] += m * d.v[j];
        r1.v[j] += mg * d.v[j];
        dw3.v[j] += mc * d.v[j];
      }
    }
    const int64_t o = ((int64_t)b * T + t) * E;
    r1.store(R1 + o, E, lane);
    if (R2) r2.store(R2 + o, E, lane);
  }
  db.store(s_fg + (wave * 2 + 0) * E, E, lane);
  dw3.store(s_fg + (wave * 2 + 1) * E, E, lane);
  __syncthreads();
  const int64_t po = ((int64_t)b * gridDim.x + blockIdx.x) * 2 * E;
  for (int i = threadIdx.x; i < 2 * E; i += 256)
    part[po + i] = (s_fg[i] + s_fg[2 * E + i]) + (s_fg[4 * E + i] + s_fg[6 * E + i]);
}

// accumulator element e of lane (h, r32): n = 4 h + (e & 3) + 8 (e >> 2) (the A operand's row), c = r32 (the B operand's column)
// HALF: X holds binary16 values (include/decafnet_hip_front_half.h).  A thread's 8 clips are ONE 16-byte load where their address
// is 16-byte aligned and all 8 lie in the slice, 8 two-byte loads otherwise.  The value times 2^4 -- an exact fp16 product over the
// operator's range -- IS the hi plane of the fp32 form and the lo plane of the fp32 form is exactly zero for it, so one X plane is
// staged and the product r_hi . x_lo (exact zeros into the accumulator) is not issued: r_lo . x_hi, then r_hi . x_hi, the order of
// the fp32 form without its middle term.
template <bool HALF>
__global__ __launch_bounds__(256) void k_fg_wgrad(FrontWgradArgs p) {
  constexpr int XPL = HALF ? 1 : 2;                 // planes of the X tile
  using x_elem = std::conditional_t<HALF, _Float16, float>;
  __shared__ __attribute__((aligned(16))) _Float16 s_r[2 * 64 * FG_PITCH];
  __shared__ __attribute__((aligned(16))) _Float16 s_x[XPL * 64 * FG_PITCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int z = blockIdx.z;
  const float* __restrict__ Rp = z == 0 ? p.R[0] : p.R[1];
  const x_elem* __restrict__ Xp = static_cast<const x_elem*>(z == 0 ? p.X[0] : p.X[1]);
  const unsigned* __restrict__ am = z == 0 ? p.absmax[0] : p.absmax[1];
  const uint8_t* __restrict__ skip = z == 0 ? p.skip[0] : p.skip[1];
  float* __restrict__ part = z == 0 ? p.part[0] : p.part[1];
  const int N = p.N, C = p.C, T = p.T;
  const int tiles_c = (C + 63) / 64;
  const int tn = blockIdx.x / tiles_c, tc = blockIdx.x - tn * tiles_c;
  const int slice = blockIdx.y;
  const int b = slice / p.slices_per_video, sv = slice - b * p.slices_per_video;
  const int t_begin = sv * p.slice_t;
  const int t_end = t_begin + p.slice_t < T ? t_begin + p.slice_t : T;
  float inv;
  const float s = cg_scale(*am, inv);
  // R: lane -> column n, wave -> 8 consecutive clips of the chunk;  X: thread -> (channel tid / 4, 8 consecutive clips (tid & 3) * 8)
  const int n_g = tn * 64 + lane;
  const bool n_ok = n_g < N;
  const int xc = tid >> 2, xt = (tid & 3) * 8;
  const int c_g = tc * 64 + xc;
  const bool c_ok = c_g < C;
  const float* __restrict__ rp = Rp + (int64_t)b * T * N + n_g;
  const x_elem* __restrict__ xp = Xp + ((int64_t)b * C + (c_ok ? c_g : 0)) * T;
  const int h = lane >> 5, r32 = lane & 31;
  const int wn = wave & 1, wc = wave >> 1;
  const bool active = tn * 64 + wn * 32 < N && tc * 64 + wc * 32 < C;      // (N, C are multiples of 32: a 32-block is whole or absent)
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;

  // the next chunk of the slice that takes a K step, from r on (uniform per workgroup; t_begin is a multiple of 64, so a chunk of
  // 32 lies inside one gate tile)
  auto next_chunk = [&](int r) {
    while (r < t_end && skip && !skip[(int64_t)b * p.ntiles + r / FG_TILE]) r += FG_ROWS;
    return r;
  };
  float rv[8];
  FrontXRegs<HALF> xv;
  auto load = [&](int r0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int t = r0 + wave * 8 + i;
      rv[i] = (n_ok && t < t_end) ? rp[(int64_t)t * N] : 0.f;
    }
    if constexpr (HALF) {
      const int t = r0 + xt;
      if (c_ok && t + 8 <= t_end && (reinterpret_cast<uintptr_t>(xp + t) & 15) == 0) {
        xv.v = *reinterpret_cast<const f16x8*>(xp + t);
        return;
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int t = r0 + xt + i;
      xv.v[i] = (c_ok && t < t_end) ? xp[t] : (x_elem)0;
    }
  };

  int r0 = next_chunk(t_begin);
  if (r0 < t_end) load(r0);
  while (r0 < t_end) {
    {
      f16x8 rh, rl;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float v = rv[i] * s;
        const _Float16 hi = (_Float16)v;
        rh[i] = hi;
        rl[i] = (_Float16)(v - (float)hi);
      }
      f16x8 xh, xl;
      if constexpr (HALF) {
        xh = xv.v * (_Float16)FG_SX;                 // exact; there is no lo plane
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float v = xv.v[i];
          const _Float16 hi = (_Float16)(v * FG_SX);
          xh[i] = hi;
          xl[i] = (_Float16)__builtin_fmaf(v, FG_SX, -(float)hi);
        }
      }
      *reinterpret_cast<f16x8*>(&s_r[(0 * 64 + lane) * FG_PITCH + wave * 8]) = rh;
      *reinterpret_cast<f16x8*>(&s_r[(1 * 64 + lane) * FG_PITCH + wave * 8]) = rl;
      *reinterpret_cast<f16x8*>(&s_x[(0 * 64 + xc) * FG_PITCH + xt]) = xh;
      if constexpr (!HALF) *reinterpret_cast<f16x8*>(&s_x[(1 * 64 + xc) * FG_PITCH + xt]) = xl;
    }
    __syncthreads();
    r0 = next_chunk(r0 + FG_ROWS);
    if (r0 < t_end) load(r0);                    // the next chunk travels while this one is multiplied
    if (active) {
#pragma unroll
      for (int ks = 0; ks < FG_ROWS / 16; ++ks) {
        const int ko = ks * 16 + h * 8;
        const f16x8 a_hi = *reinterpret_cast<const f16x8*>(&s_r[(0 * 64 + wn * 32 + r32) * FG_PITCH + ko]);
        const f16x8 a_lo = *reinterpret_cast<const f16x8*>(&s_r[(1 * 64 + wn * 32 + r32) * FG_PITCH + ko]);
        const f16x8 b_hi = *reinterpret_cast<const f16x8*>(&s_x[(0 * 64 + wc * 32 + r32) * FG_PITCH + ko]);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_lo, b_hi, acc, 0, 0, 0);
        if constexpr (!HALF) {
          const f16x8 b_lo = *reinterpret_cast<const f16x8*>(&s_x[(1 * 64 + wc * 32 + r32) * FG_PITCH + ko]);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, b_lo, acc, 0, 0, 0);
        }
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, b_hi, acc, 0, 0, 0);
      }
    }
    __syncthreads();
  }

  if (active) {
    const int c = tc * 64 + wc * 32 + r32;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int n = tn * 64 + wn * 32 + 4 * h + (e & 3) + 8 * (e >> 2);
      part[((int64_t)slice * N + n) * C + c] = acc[e];
    }
  }
}

// out[(i / rowlen) pitch + i % rowlen] (+)= extra * inv_scale * sum_s part[s][i], the parts in the fixed blocked order of
// grad_common.h, in its rolled form: the unrolled one's scalar address arithmetic did not fit the scalar registers here
__global__ __launch_bounds__(256) void k_fg_reduce(const float* __restrict__ part, int nparts, int64_t stride, int count, int rowlen, int pitch,
                                                  const unsigned* __restrict__ absmax, float extra, float* __restrict__ out, int accumulate,
                                                  unsigned* __restrict__ status) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  float sum = 0.f;
  DCF_BLOCKED_SUM_ROLLED(sum, part, nparts, stride, i);
  float inv = 1.f;
  if (absmax) (void)cg_scale(*absmax, inv);
  const float v = (sum * extra) * inv;
  if (!(__builtin_fabsf(v) <= 3.4028234664e38f)) atomicOr(status, 1u);
  const int n = i / rowlen;
  const int64_t o = (int64_t)n * pitch + (i - n * rowlen);
  out[o] = accumulate ? out[o] + v : v;
}

int launch_front_wgrad(const FrontWgradArgs& a, int pairs, hipStream_t st, bool half) {
  const dim3 grid(((a.N + 63) / 64) * ((a.C + 63) / 64), a.nvid * a.slices_per_video, pairs);
  if (half) hipLaunchKernelGGL(k_fg_wgrad<true>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_fg_wgrad<false>, grid, dim3(256), 0, st, a);
  DCF_HIP(hipGetLastError());
  return 0;
}

// ---- host side ---------------------------------------------------------------------------------------------------
struct FrontShape {
  int nvid, D, T, E, Cin, rows_q, ntiles;      // rows_q = B'
};

static int front_check(const char* what, const void* vid, const float* gate, const uint8_t* mask, const int32_t* nq, int32_t nvid, int32_t D,
                       int32_t T, int32_t E, bool msf, bool scat, FrontShape* s) {
  DCF_CHECK(vid && gate && mask && nq, "%s: null argument", what);
  DCF_CHECK(nvid > 0 && nvid <= 65535 && T > 0, "%s: nvid = %d (1 .. 65535), T = %d (>= 1)", what, nvid, T);
  DCF_CHECK(D > 0 && D % 32 == 0, "%s: D = %d must be a positive multiple of 32", what, D);
  DCF_CHECK(E > 0 && E % 32 == 0 && E <= 1024, "%s: E = %d must be a positive multiple of 32, at most 1024", what, E);
  int64_t rows = 0;
  for (int v = 0; v < nvid; ++v) {
    DCF_CHECK(nq[v] >= 1, "%s: nq[%d] = %d (every video has at least one query)", what, v, nq[v]);
    rows += nq[v];
    DCF_CHECK(rows * T < (1ll << 31) - 64, "%s: %lld rows (< 2^31)", what, (long long)rows * T);
  }
  DCF_CHECK((int64_t)nvid * D * T < (1ll << 40), "%s: feature tensor too large", what);
  s->nvid = nvid; s->D = D; s->T = T; s->E = E; s->Cin = D + (msf ? D : 0) + (scat ? 1 : 0); s->rows_q = (int)rows;
  s->ntiles = (T + FG_TILE - 1) / FG_TILE;
  return 0;
}

// the device tables of the call: qoff (nvid + 1), vtab (B'), tile flags (nvid, ntiles)
static int front_tables(const FrontShape& s, const int32_t* nq, const float* gate, int noskip, int* qoff, int* vtab, uint8_t* flags, hipStream_t st) {
  if (launch_front_qtables(s.nvid, nq, qoff, vtab, st)) return -1;
  hipLaunchKernelGGL(k_fg_tileflags, dim3(s.ntiles, s.nvid), dim3(64), 0, st, gate, qoff, flags, s.T, s.ntiles, noskip);
  DCF_HIP(hipGetLastError());
  return 0;
}

int launch_front_qtables(int nvid, const int32_t* nq, int* qoff, int* vtab, hipStream_t st) {
  int q0 = 0;
  for (int v0 = 0; v0 < nvid; v0 += FG_NQ_CHUNK) {
    FrontNq c{};
    c.v0 = v0; c.q0 = q0; c.n = nvid - v0 < FG_NQ_CHUNK ? nvid - v0 : FG_NQ_CHUNK;
    for (int i = 0; i < c.n; ++i) { c.nq[i] = nq[v0 + i]; q0 += nq[v0 + i]; }
    hipLaunchKernelGGL(k_fg_tables, dim3(1), dim3(64), 0, st, c, qoff, vtab);
  }
  DCF_HIP(hipGetLastError());
  return 0;
}

int launch_front_unpack_w(const float* W, int Cin, int D, int E, float* W1c, float* W2c, float* w3c, hipStream_t st) {
  hipLaunchKernelGGL(k_fg_unpack_w, dim3((E * D + 255) / 256), dim3(256), 0, st, W, Cin, D, E, W1c, W2c, w3c);
  DCF_HIP(hipGetLastError());
  return 0;
}

int launch_front_reduce(const float* part, int nparts, int64_t stride, int count, int rowlen, int pitch, const unsigned* absmax, float extra,
                        float* out, int accumulate, unsigned* status, hipStream_t st) {
  hipLaunchKernelGGL(k_fg_reduce, dim3((count + 255) / 256), dim3(256), 0, st, part, nparts, stride, count, rowlen, pitch, absmax, extra, out,
                     accumulate, status);
  DCF_HIP(hipGetLastError());
  return 0;
}

static bool aligned_to(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

// dcf_op_vidmap_shared (half = false: vid / shallow fp32) and dcf_op_vidmap_shared_h (half = true: binary16, read by the split tile
// path's A_CHANMAJOR_H mode where it applies, upcast once into scratch otherwise; the option half_native decides as in the engine)
static int front_forward(const char* what, const void* vid_in, const void* shallow_in, bool half, const float* W, const float* bias,
                         const float* gate, const uint8_t* mask, const float* correl, const int32_t* nq, float* Y, int32_t nvid, int32_t D,
                         int32_t T, int32_t E, int32_t flags, hipStream_t st) {
  FrontShape s{};
  DCF_CHECK(W && bias && Y, "%s: null argument", what);
  if (front_check(what, vid_in, gate, mask, nq, nvid, D, T, E, shallow_in != nullptr, correl != nullptr, &s)) return -1;
  bool native = false;
  if (half) {
    const int want = debug_option("half_native", 1);
    native = want != 0 && E % 128 == 0 && T % 4 == 0 && aligned_to(vid_in, 8) && aligned_to(shallow_in, 8);
    DCF_CHECK(native || want != 2, "%s: these products cannot read the half features natively (E %% 128 != 0, T %% 4 != 0 or a feature pointer "
                                   "that is not 8-byte aligned) and the option half_native = 2 forbids the upcast", what);
  }
  unsigned* status = nullptr;
  if (cg_begin(what, st, &status)) return -1;
  const int Cin = s.Cin;
  const size_t pe = (size_t)nvid * T * E, px = (size_t)nvid * D * T;
  StreamScratch sc(st);
  const void *vid = vid_in, *shallow = shallow_in;
  if (half && !native) {                              // the fp32 path on fp32 copies
    float *up1 = nullptr, *up2 = nullptr;
    if (sc.take(&up1, px) || (shallow_in && sc.take(&up2, px))) return -1;
    if (launch_half_to_f32(static_cast<const uint16_t*>(vid_in), up1, (int64_t)px, st)) return -1;
    if (shallow_in && launch_half_to_f32(static_cast<const uint16_t*>(shallow_in), up2, (int64_t)px, st)) return -1;
    vid = up1; shallow = up2;
  }
  const size_t xbytes = native ? sizeof(uint16_t) : sizeof(float);
  // the split tile path of the channel-major GEMM: 64-row tiles of 128 columns, 16-byte loads along T (8-byte loads of halves)
  const bool split = native || (E % 128 == 0 && T % 4 == 0 && aligned_to(vid, 16) && aligned_to(shallow, 16));
  int *qoff = nullptr, *vtab = nullptr;
  uint8_t* tflags = nullptr;
  float *P1 = nullptr, *P2 = nullptr, *W1c = nullptr, *W2c = nullptr, *w3c = nullptr;
  unsigned short *pl1 = nullptr, *pl2 = nullptr;
  if (sc.take(&qoff, (size_t)nvid + 1) || sc.take(&vtab, (size_t)s.rows_q) || sc.take(&tflags, (size_t)nvid * s.ntiles)) return -1;
  if (sc.take(&P1, pe) || (shallow && sc.take(&P2, pe))) return -1;
  if (split) {
    if (sc.take(&pl1, (size_t)3 * E * D) || (shallow && sc.take(&pl2, (size_t)3 * E * D))) return -1;
  } else {
    if (sc.take(&W1c, (size_t)E * D) || (shallow && sc.take(&W2c, (size_t)E * D))) return -1;
  }
  if (correl && sc.take(&w3c, (size_t)E)) return -1;
  int rc = front_tables(s, nq, gate, flags & DCF_FRONT_NO_SKIP, qoff, vtab, tflags, st);
  if (rc == 0 && (!split || correl)) {
    hipLaunchKernelGGL(k_fg_unpack_w, dim3((E * D + 255) / 256), dim3(256), 0, st, W, Cin, D, E, W1c, W2c, w3c);
    if (hipGetLastError() != hipSuccess) { set_error("%s: launch failed", what); rc = -1; }
  }
  if (rc == 0 && split) {
    rc = launch_split_planes(W, pl1, E, D, Cin, st, GEMM_F16X3, status);
    if (rc == 0 && shallow) rc = launch_split_planes(W + D, pl2, E, D, Cin, st, GEMM_F16X3, status);
  }
  // the products, three videos per grid; the expert half leaves the row tiles no query keeps unwritten (split path)
  for (int pair = 0; pair < (shallow ? 2 : 1) && rc == 0; ++pair) {
    const char* X = static_cast<const char*>(pair ? shallow : vid);       // (GemmArgs::A carries the address of the halves too)
    float* P = pair ? P2 : P1;
    for (int v0 = 0; v0 < nvid && rc == 0; v0 += 3) {
      GemmArgs g[3];
      const int ng = nvid - v0 < 3 ? nvid - v0 : 3;
      for (int i = 0; i < ng; ++i) {
        g[i] = GemmArgs{};
        g[i].A = reinterpret_cast<const float*>(X + (size_t)(v0 + i) * D * T * xbytes); g[i].lda = T;
        g[i].C = P + (size_t)(v0 + i) * T * E; g[i].ldc = E;
        g[i].M = T; g[i].N = E; g[i].K = D;
        if (split) {
          g[i].W = W + (pair ? D : 0); g[i].ldw = Cin; g[i].Ws = pair ? pl2 : pl1; g[i].status = status;
          if (!pair) { g[i].tile_skip = tflags + (size_t)(v0 + i) * s.ntiles; g[i].skip_nq = 1; g[i].skip_stride = s.ntiles; }
        } else {
          g[i].W = pair ? W2c : W1c; g[i].ldw = D;
        }
      }
      rc = split ? launch_gemm_split(g, ng, native ? A_CHANMAJOR_H : A_CHANMAJOR, GEMM_F16X3, st) : launch_gemm(g, ng, A_CHANMAJOR, st);
    }
  }
  if (rc == 0) rc = launch_vidmap_combine(P1, P2, bias, gate, mask, w3c, correl, Y, T, s.rows_q * T, E, 0ull, st, vtab);
  rc = sc.end(rc);
  return rc == 0 ? cg_end(st) : rc;
}

// dcf_op_vidmap_shared_bwd (half = false) and dcf_op_vidmap_shared_bwd_h (half = true: k_fg_wgrad<true> reads the stored values, for
// every shape and alignment; nothing is upcast)
static int front_backward(const char* what, const void* vid, const void* shallow, bool half, const float* gate, const uint8_t* mask,
                          const float* correl, const int32_t* nq, const float* dY, float* dW, float* db, int32_t nvid, int32_t D, int32_t T,
                          int32_t E, int32_t flags, int32_t accumulate, hipStream_t st) {
  FrontShape s{};
  DCF_CHECK(dY && dW, "%s: null argument", what);
  if (front_check(what, vid, gate, mask, nq, nvid, D, T, E, shallow != nullptr, correl != nullptr, &s)) return -1;
  unsigned* status = nullptr;
  if (cg_begin(what, st, &status)) return -1;
  const int Cin = s.Cin, pairs = shallow ? 2 : 1;
  const size_t pe = (size_t)nvid * T * E;
  const int nstrips = (T + FG_STRIP - 1) / FG_STRIP;
  // T slices: whole gate tiles, from the shapes alone -- as many as bring the grid to FG_WANT_WGS workgroups, at most CG_MAX_SLICES
  // in all while there are fewer videos than that (every slice costs a 64 x 64 partial per tile, written and read back)
  const int tiles = ((E + 63) / 64) * ((D + 63) / 64) * pairs;
  const int total = FG_WANT_WGS / tiles < 1 ? 1 : (FG_WANT_WGS / tiles > CG_MAX_SLICES ? CG_MAX_SLICES : FG_WANT_WGS / tiles);
  const int want = total / nvid > 1 ? total / nvid : 1;
  const int slice_t = ((T + want - 1) / want + FG_TILE - 1) / FG_TILE * FG_TILE;
  const int spv = (T + slice_t - 1) / slice_t, nslices = nvid * spv;
  const int64_t count = (int64_t)E * D;
  StreamScratch sc(st);
  int *qoff = nullptr, *vtab = nullptr;
  uint8_t* tflags = nullptr;
  float *R1 = nullptr, *R2 = nullptr, *rpart = nullptr, *part = nullptr;
  unsigned* words = nullptr;
  if (sc.take(&qoff, (size_t)nvid + 1) || sc.take(&vtab, (size_t)s.rows_q) || sc.take(&tflags, (size_t)nvid * s.ntiles)) return -1;
  if (sc.take(&R1, pe) || (shallow && sc.take(&R2, pe))) return -1;
  if (sc.take(&rpart, (size_t)nvid * nstrips * 2 * E) || sc.take(&part, (size_t)pairs * nslices * count) || sc.take(&words, 2)) return -1;
  int rc = front_tables(s, nq, gate, flags & DCF_FRONT_NO_SKIP, qoff, vtab, tflags, st);
  if (rc == 0) {
    const dim3 grid(nstrips, nvid);
    const size_t lds = (size_t)8 * E * sizeof(float);
    const int nch = (E + 255) / 256;
    if (nch == 1) hipLaunchKernelGGL(k_fg_rowsums<1>, grid, dim3(256), lds, st, dY, gate, mask, correl, qoff, R1, R2, rpart, T, E);
    else if (nch == 2) hipLaunchKernelGGL(k_fg_rowsums<2>, grid, dim3(256), lds, st, dY, gate, mask, correl, qoff, R1, R2, rpart, T, E);
    else if (nch == 3) hipLaunchKernelGGL(k_fg_rowsums<3>, grid, dim3(256), lds, st, dY, gate, mask, correl, qoff, R1, R2, rpart, T, E);
    else hipLaunchKernelGGL(k_fg_rowsums<4>, grid, dim3(256), lds, st, dY, gate, mask, correl, qoff, R1, R2, rpart, T, E);
    if (hipGetLastError() != hipSuccess) { set_error("%s: launch failed", what); rc = -1; }
  }
  if (rc == 0) rc = launch_absmax(R1, (int64_t)pe, words, st);
  if (rc == 0 && shallow) rc = launch_absmax(R2, (int64_t)pe, words + 1, st);
  if (rc == 0) {
    FrontWgradArgs a{};
    a.R[0] = R1; a.X[0] = vid; a.absmax[0] = words; a.skip[0] = tflags; a.part[0] = part;
    a.R[1] = R2; a.X[1] = shallow; a.absmax[1] = words + 1; a.skip[1] = nullptr; a.part[1] = part + (size_t)nslices * count;
    a.nvid = nvid; a.T = T; a.N = E; a.C = D; a.slice_t = slice_t; a.slices_per_video = spv; a.ntiles = s.ntiles;
    rc = launch_front_wgrad(a, pairs, st, half);
  }
  if (rc == 0) {
    const dim3 gw((unsigned)((count + 255) / 256)), ge((E + 255) / 256);
    for (int pair = 0; pair < pairs; ++pair)
      hipLaunchKernelGGL(k_fg_reduce, gw, dim3(256), 0, st, part + (size_t)pair * nslices * count, nslices, count, (int)count, D, Cin,
                         words + pair, 1.f / FG_SX, dW + (pair ? D : 0), accumulate, status);
    if (correl)
      hipLaunchKernelGGL(k_fg_reduce, ge, dim3(256), 0, st, rpart + E, nvid * nstrips, (int64_t)2 * E, E, 1, Cin, (const unsigned*)nullptr, 1.f,
                         dW + (Cin - 1), accumulate, status);
    if (db)
      hipLaunchKernelGGL(k_fg_reduce, ge, dim3(256), 0, st, rpart, nvid * nstrips, (int64_t)2 * E, E, E, E, (const unsigned*)nullptr, 1.f, db,
                         accumulate, status);
    if (hipGetLastError() != hipSuccess) { set_error("%s: launch failed", what); rc = -1; }
  }
  rc = sc.end(rc);
  return rc == 0 ? cg_end(st) : rc;
}

}  // namespace dcf

using namespace dcf;

extern "C" {

int dcf_front_ext_version(void) { return DCF_FRONT_EXT_VERSION; }

int dcf_front_half_ext_version(void) { return DCF_FRONT_HALF_EXT_VERSION; }

int dcf_op_vidmap_shared(const float* vid, const float* shallow, const float* W, const float* bias, const float* gate,
                         const uint8_t* mask, const float* correl, const int32_t* nq, float* Y, int32_t nvid, int32_t D, int32_t T,
                         int32_t E, int32_t flags, void* stream) {
  return front_forward("dcf_op_vidmap_shared", vid, shallow, false, W, bias, gate, mask, correl, nq, Y, nvid, D, T, E, flags, (hipStream_t)stream);
}

int dcf_op_vidmap_shared_bwd(const float* vid, const float* shallow, const float* gate, const uint8_t* mask, const float* correl,
                             const int32_t* nq, const float* dY, float* dW, float* db, int32_t nvid, int32_t D, int32_t T, int32_t E,
                             int32_t flags, int32_t accumulate, void* stream) {
  return front_backward("dcf_op_vidmap_shared_bwd", vid, shallow, false, gate, mask, correl, nq, dY, dW, db, nvid, D, T, E, flags, accumulate,
                        (hipStream_t)stream);
}

int dcf_op_vidmap_shared_h(const uint16_t* vid, const uint16_t* shallow, const float* W, const float* bias, const float* gate,
                           const uint8_t* mask, const float* correl, const int32_t* nq, float* Y, int32_t nvid, int32_t D, int32_t T,
                           int32_t E, int32_t flags, void* stream) {
  return front_forward("dcf_op_vidmap_shared_h", vid, shallow, true, W, bias, gate, mask, correl, nq, Y, nvid, D, T, E, flags, (hipStream_t)stream);
}

int dcf_op_vidmap_shared_bwd_h(const uint16_t* vid, const uint16_t* shallow, const float* gate, const uint8_t* mask, const float* correl,
                               const int32_t* nq, const float* dY, float* dW, float* db, int32_t nvid, int32_t D, int32_t T, int32_t E,
                               int32_t flags, int32_t accumulate, void* stream) {
  return front_backward("dcf_op_vidmap_shared_bwd_h", vid, shallow, true, gate, mask, correl, nq, dY, dW, db, nvid, D, T, E, flags, accumulate,
                        (hipStream_t)stream);
}

}  // extern "C"
