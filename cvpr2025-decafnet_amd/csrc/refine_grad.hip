// Forward / backward of the refinement stage between the first classification head and the other two heads of
// PtTransformerEarlyFusionIterative (libs/modeling/model.py:449-455, libs/modeling/tcn.py:21-38), on token-major (B*T0, 32) fp32 rows.
//
// refine_in: the stacking of the nearest-upsampled first-pass logits (model.py:449-455) fused with refine.conv_1x1 (tcn.py:69-70)
//   u[b,t,0] = logits1[b,0,t]  (level 0 is not masked, to the letter),  u[b,t,l] = m0[b,t] logits1[b,l,t >> l]  for l > 0
//   H[b,t,c] = b_in[c] + sum_l W_in[c,l] u[b,t,l]                                   (l ascending)
//   dU[b,t,l] = (l == 0 ? 1 : m0[b,t]) sum_c W_in[c,l] dH[b,t,c],   dlogits1[b,l,s] = sum of dU[b,t,l] over t >> l == s, t ascending
//   dW_in[c,l] = sum_{b,t} dH[b,t,c] u[b,t,l],   db_in[c] = sum_{b,t} dH[b,t,c]
//
// tcn_layer: one DilatedResidualLayer (tcn.py:21-38), dilation d, taps inside sequence b, the convolution's input NOT masked
//   h = relu(bd + sum_{j,ci} Wd[.,ci,j] X[t + (j-1) d, ci]),   o = drop(bp + Wp h),   z = (X + o) m,   Y = LN(z) ln_w + ln_b
//   g = dY ln_w,  dz = m rs (g - mean g - zhat mean(g zhat)),  do = dz keep / (1 - p),  dh = (h > 0) Wp^T do
//   dX[t] = dz[t] + sum_j Wd[.,.,j]^T dh[t - (j-1) d],   dWd[co,ci,j] = sum dh[t,co] X[t + (j-1) d, ci],   dbd = sum dh,
//   dWp[co,ci] = sum do[t,co] h[t,ci],   dbp = sum do,   dln_w = sum dY zhat,   dln_b = sum dY
//   The backward saves nothing but X: h, o, the keep bits and the LayerNorm statistics are recomputed by the forward's own code.
//
// Arithmetic: fp32 on the vector ALU throughout, every contraction an explicit fma chain in ascending index; there is no matrix-core
// variant and nothing falls back to another arithmetic.  The layer kernels follow k_tcn_layer (heads.hip): a workgroup of four waves
// owns 64 rows, a lane a row, a wave eight output channels; the weights and the row's 96 tap inputs sit in LDS, the tap tile
// channel-major with a pitch of 65 floats so that both the row-parallel reads (a lane per row) and the channel-parallel reads of the
// outer products (a lane per channel) are free of bank conflicts.  The backward runs in two phases: k_tcn_bwd1 recomputes the forward
// of its rows, forms dz and dh, leaves them in dX and in scratch, and accumulates the parameter gradients of its slice of
// RG_SLICE_ROWS rows -- the two outer products as 12 + 4 register accumulators per thread over the rows in ascending order, the
// four 32-vectors as wave reductions on DPP; k_tcn_bwd2 gathers dX from dh at t and t -+ d.  k_rg_reduce adds the slices in the fixed
// blocked order of blocked_sum (grad_common.h).  No
// floating-point atomics; the slicing is a constant: results are bit-identical from run to run, and every product has the upstream
// gradient as one factor, so a power-of-two scale of it scales the results by exactly that.
#include <math.h>

#include "../../include/decafnet_hip.h"
#include "dropout.h"
#include "grad_common.h"
#include "refine_grad.h"

namespace dcf {

// ------------------------------------------------------------------------------------------
// refine_in
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_refine_in_fwd(RefineInArgs p) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)p.rows * (RG_C / 4)) return;
  const int r = (int)(i >> 3), c = (int)(i & 7) * 4;
  const int b = r / p.T0, t = r - b * p.T0;
  const float mf = (!p.mask0 || p.mask0[r]) ? 1.f : 0.f;
  const float* lg = p.logits1 + (int64_t)b * p.S;
  f32x4 acc = ld4(p.b + c);
  for (int l = 0; l < p.L; ++l) {
    float u = lg[p.off[l] + (t >> l)];
    if (l > 0) u *= mf;
    acc = f32x4{__builtin_fmaf(p.W[(c + 0) * p.L + l], u, acc.x), __builtin_fmaf(p.W[(c + 1) * p.L + l], u, acc.y),
                __builtin_fmaf(p.W[(c + 2) * p.L + l], u, acc.z), __builtin_fmaf(p.W[(c + 3) * p.L + l], u, acc.w)};
  }
  st4(p.H + (int64_t)r * RG_C + c, acc);
}

// a workgroup owns a slice of RG_SLICE_ROWS rows: dH and u of the slice in LDS, then a thread per (l, c) for the slice's sums of
// dW_in / db_in (rows ascending) and a thread per (row, l) for dU (channels ascending)
__global__ __launch_bounds__(256) void k_refine_in_bwd(RefineInArgs p) {
  constexpr int DP = RG_C + 1, UP = RG_MAX_L + 1;
  __shared__ float s_dh[RG_SLICE_ROWS * DP];
  __shared__ float s_u[RG_SLICE_ROWS * UP];
  __shared__ float s_w[RG_C * RG_MAX_L];
  const int tid = threadIdx.x, L = p.L;
  const int r0 = blockIdx.x * RG_SLICE_ROWS;
  for (int i = tid; i < RG_SLICE_ROWS * (RG_C / 4); i += 256) {
    const int rr = i >> 3, c = (i & 7) * 4, r = r0 + rr;
    const f32x4 v = r < p.rows ? ld4(p.dH + (int64_t)r * RG_C + c) : f32x4{0.f, 0.f, 0.f, 0.f};
    s_dh[rr * DP + c] = v.x; s_dh[rr * DP + c + 1] = v.y; s_dh[rr * DP + c + 2] = v.z; s_dh[rr * DP + c + 3] = v.w;
  }
  for (int i = tid; i < RG_SLICE_ROWS * (L + 1); i += 256) {
    const int rr = i / (L + 1), l = i - rr * (L + 1), r = r0 + rr;
    float u = 0.f;
    if (r < p.rows) {
      if (l == L) u = 1.f;                                   // the bias column
      else if (p.logits1) {
        const int b = r / p.T0, t = r - b * p.T0;
        u = p.logits1[(int64_t)b * p.S + p.off[l] + (t >> l)];
        if (l > 0) u *= (!p.mask0 || p.mask0[r]) ? 1.f : 0.f;
      }
    }
    s_u[rr * UP + l] = u;
  }
  for (int i = tid; i < RG_C * L; i += 256) s_w[i] = p.W ? p.W[i] : 0.f;
  __syncthreads();
  if (p.part) {
    for (int i = tid; i < RG_C * (L + 1); i += 256) {
      const int c = i & 31, l = i >> 5;
      float acc = 0.f;
      for (int rr = 0; rr < RG_SLICE_ROWS; ++rr) acc = __builtin_fmaf(s_dh[rr * DP + c], s_u[rr * UP + l], acc);
      p.part[(int64_t)blockIdx.x * (RG_C * (L + 1)) + i] = acc;
    }
  }
  if (p.dU) {
    for (int i = tid; i < RG_SLICE_ROWS * L; i += 256) {
      const int rr = i & (RG_SLICE_ROWS - 1), l = i / RG_SLICE_ROWS, r = r0 + rr;
      if (r >= p.rows) continue;
      float acc = 0.f;
#pragma unroll 8
      for (int c = 0; c < RG_C; ++c) acc = __builtin_fmaf(s_w[c * L + l], s_dh[rr * DP + c], acc);
      const bool keep = l == 0 || !p.mask0 || p.mask0[r];
      p.dU[(int64_t)r * L + l] = keep ? acc : 0.f;
    }
  }
}

// dlogits1[b, off[l] + s] = sum of dU[b, t, l] over the 2^l rows t >> l == s, t ascending
__global__ __launch_bounds__(256) void k_refine_in_gather(RefineInArgs p, float* __restrict__ dlogits, int B) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)B * p.S) return;
  const int b = (int)(i / p.S), e = (int)(i - (int64_t)b * p.S);
  int l = 0;
  while (l + 1 < p.L && e >= p.off[l + 1]) ++l;
  const int s = e - p.off[l], n = 1 << l;
  const float* src = p.dU + ((int64_t)b * p.T0 + ((int64_t)s << l)) * p.L + l;
  float acc = 0.f;
  for (int k = 0; k < n; ++k) acc += src[(int64_t)k * p.L];
  dlogits[i] = acc;
}

// dW_in (32, L) and db_in (32) from the slices' [l][c] sums
__global__ __launch_bounds__(256) void k_refine_in_reduce(const float* __restrict__ part, int nparts, int L, float* __restrict__ dW,
                                                          float* __restrict__ db, int accumulate) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= RG_C * (L + 1)) return;
  const int c = i & 31, l = i >> 5;
  float* out = l == L ? (db ? db + c : nullptr) : (dW ? dW + c * L + l : nullptr);
  if (!out) return;
  const float sum = blocked_sum(part, nparts, (int64_t)RG_C * (L + 1), i);
  *out = accumulate ? *out + sum : sum;
}

// ------------------------------------------------------------------------------------------
// DilatedResidualLayer
// ------------------------------------------------------------------------------------------
// LDS floats of the layer kernels, in this order: wd [96 k = (tap, ci)][32 co], wpT [32 ci][32 co], x [96 k][65], h [32][65],
// p [32][65]; the backward adds wp [32 co][32 ci] and q [32][65]
constexpr int RG_T32 = RG_C * RG_PITCH;                       // a [32][65] tile
constexpr int RG_LDS_FWD = 3 * RG_C * RG_C + RG_C * RG_C + 3 * RG_T32 + 2 * RG_T32;
constexpr int RG_LDS_BWD = RG_LDS_FWD + RG_C * RG_C + RG_T32;

struct TcnLds {
  float *wd, *wpT, *x, *h, *p, *wp, *q;
  __device__ __forceinline__ TcnLds(float* s) {
    wd = s; wpT = wd + 3 * RG_C * RG_C; x = wpT + RG_C * RG_C; h = x + 3 * RG_T32; p = h + RG_T32; wp = p + RG_T32; q = wp + RG_C * RG_C;
  }
};

// PyTorch's Wd (co, ci, tap) as [tap * 32 + ci][co], Wp (co, ci) as [ci][co] (and as it is for the backward)
template <bool BWD>
__device__ __forceinline__ void tcn_stage_weights(const TcnLds& s, const float* __restrict__ Wd, const float* __restrict__ Wp, int tid) {
  for (int i = tid; i < 3 * RG_C * RG_C; i += 256) {
    const int co = i / (3 * RG_C), rem = i - co * 3 * RG_C, ci = rem / 3, tap = rem - ci * 3;
    s.wd[(tap * RG_C + ci) * RG_C + co] = Wd[i];
  }
  for (int i = tid; i < RG_C * RG_C; i += 256) {
    const float w = Wp[i];
    s.wpT[(i & 31) * RG_C + (i >> 5)] = w;
    if constexpr (BWD) s.wp[i] = w;
  }
}

// what a thread (lane = row of the tile, wave = channels c0 .. c0 + 7) knows about its row after the forward
struct TcnRow {
  float z[8];            // (X + drop(o)) m of the thread's channels
  float mean, rs;        // LayerNorm statistics of the row
  float mf;              // the row's mask as 0 / 1
  unsigned keep;         // keep bits of the thread's channels (all ones without dropout)
  int r;
  bool live;
};

// the forward of the tile's rows up to the LayerNorm statistics; leaves the taps in s.x, relu(h) in s.h and z in s.p.  Starts with a
// barrier-free write of s.x: the caller has a barrier between the last read of the previous tile and this call.
template <bool DROP>
__device__ __forceinline__ TcnRow tcn_rows_forward(const TcnLds& s, const TcnLayerArgs& a, int r0, int lane, int w) {
  TcnRow o;
  o.r = r0 + lane;
  o.live = o.r < a.rows;
  const int b = o.live ? o.r / a.T0 : 0, t = o.live ? o.r - b * a.T0 : 0;
  const int c0 = 8 * w;
  // the row's 3 x 32 inputs = 24 quads; wave w stages quads 6 w .. 6 w + 5
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    const int f = w * 6 + q, tap = f >> 3, c4 = (f & 7) * 4;
    const int64_t tt = (int64_t)t + (int64_t)(tap - 1) * a.dil;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (o.live && tt >= 0 && tt < a.T0) v = ld4(a.X + ((int64_t)o.r + (int64_t)(tap - 1) * a.dil) * RG_C + c4);
    float* dst = s.x + (tap * RG_C + c4) * RG_PITCH + lane;
    dst[0] = v.x; dst[RG_PITCH] = v.y; dst[2 * RG_PITCH] = v.z; dst[3 * RG_PITCH] = v.w;
  }
  __syncthreads();                                       // (the first tile: the weights are staged too)
  float h[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) h[c] = a.bd[c0 + c];
#pragma unroll 4
  for (int k = 0; k < 3 * RG_C; ++k) {
    const float xv = s.x[k * RG_PITCH + lane];
    const f32x4 w0 = ld4(s.wd + k * RG_C + c0), w1 = ld4(s.wd + k * RG_C + c0 + 4);
    h[0] = __builtin_fmaf(w0.x, xv, h[0]); h[1] = __builtin_fmaf(w0.y, xv, h[1]);
    h[2] = __builtin_fmaf(w0.z, xv, h[2]); h[3] = __builtin_fmaf(w0.w, xv, h[3]);
    h[4] = __builtin_fmaf(w1.x, xv, h[4]); h[5] = __builtin_fmaf(w1.y, xv, h[5]);
    h[6] = __builtin_fmaf(w1.z, xv, h[6]); h[7] = __builtin_fmaf(w1.w, xv, h[7]);
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) s.h[(c0 + c) * RG_PITCH + lane] = fmaxf(h[c], 0.f);
  __syncthreads();
  float v[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) v[c] = a.bp[c0 + c];
#pragma unroll 4
  for (int ci = 0; ci < RG_C; ++ci) {
    const float hv = s.h[ci * RG_PITCH + lane];
    const f32x4 w0 = ld4(s.wpT + ci * RG_C + c0), w1 = ld4(s.wpT + ci * RG_C + c0 + 4);
    v[0] = __builtin_fmaf(w0.x, hv, v[0]); v[1] = __builtin_fmaf(w0.y, hv, v[1]);
    v[2] = __builtin_fmaf(w0.z, hv, v[2]); v[3] = __builtin_fmaf(w0.w, hv, v[3]);
    v[4] = __builtin_fmaf(w1.x, hv, v[4]); v[5] = __builtin_fmaf(w1.y, hv, v[5]);
    v[6] = __builtin_fmaf(w1.z, hv, v[6]); v[7] = __builtin_fmaf(w1.w, hv, v[7]);
  }
  o.mf = (o.live && (!a.mask || a.mask[o.r])) ? 1.f : 0.f;
  o.keep = 0xffu;
  if constexpr (DROP) {
    const int64_t bg = (int64_t)a.b0 + b;
    o.keep = 0u;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const bool k = drop_keep(a.seed, a.site, (uint64_t)((bg * RG_C + c0 + c) * (int64_t)a.T0 + t), a.p);
      o.keep |= (unsigned)k << c;
      v[c] = k ? v[c] * a.scale : 0.f;
    }
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    o.z[c] = (s.x[(RG_C + c0 + c) * RG_PITCH + lane] + v[c]) * o.mf;       // the residual is the centre tap
    s.p[(c0 + c) * RG_PITCH + lane] = o.z[c];
  }
  __syncthreads();
  float mean = 0.f;
#pragma unroll
  for (int c = 0; c < RG_C; ++c) mean += s.p[c * RG_PITCH + lane];
  mean *= (1.0f / RG_C);
  float var = 0.f;
#pragma unroll
  for (int c = 0; c < RG_C; ++c) {
    const float d = s.p[c * RG_PITCH + lane] - mean;
    var = __builtin_fmaf(d, d, var);
  }
  o.mean = mean;
  o.rs = 1.0f / sqrtf(var * (1.0f / RG_C) + 1e-5f);
  return o;
}

template <bool DROP>
__global__ __launch_bounds__(256) void k_rg_tcn_fwd(TcnLayerArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_rg[];
  const TcnLds s(s_rg);
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  tcn_stage_weights<false>(s, a.Wd, a.Wp, tid);
  const TcnRow o = tcn_rows_forward<DROP>(s, a, blockIdx.x * RG_TILE, lane, w);
  if (!o.live) return;
  const int c0 = 8 * w;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const f32x4 lw = ld4(a.lnw + c0 + 4 * q), lb = ld4(a.lnb + c0 + 4 * q);
    f32x4 y;
    y.x = __builtin_fmaf((o.z[4 * q] - o.mean) * o.rs, lw.x, lb.x);
    y.y = __builtin_fmaf((o.z[4 * q + 1] - o.mean) * o.rs, lw.y, lb.y);
    y.z = __builtin_fmaf((o.z[4 * q + 2] - o.mean) * o.rs, lw.z, lb.z);
    y.w = __builtin_fmaf((o.z[4 * q + 3] - o.mean) * o.rs, lw.w, lb.w);
    st4(a.Y + (int64_t)o.r * RG_C + c0 + 4 * q, y);
  }
}

// phase 1 of the backward: a workgroup owns slice blockIdx.x of RG_SLICE_ROWS rows and walks it in tiles of 64
template <bool DROP>
__global__ __launch_bounds__(256) void k_tcn_bwd1(TcnLayerArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_rg[];
  const TcnLds s(s_rg);
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c0 = 8 * w;
  const bool want_part = a.part != nullptr;
  tcn_stage_weights<true>(s, a.Wd, a.Wp, tid);
  // outer products: thread (ci = tid & 31, co = 4 (tid >> 5) .. + 3)
  const int oci = tid & 31, oco = 4 * (tid >> 5);
  float awd[4][3], awp[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) { awd[i][0] = awd[i][1] = awd[i][2] = 0.f; awp[i] = 0.f; }
  // the four 32-vectors: wave-uniform sums of the wave's eight channels
  float abd[8], abp[8], alw[8], alb[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) abd[c] = abp[c] = alw[c] = alb[c] = 0.f;
  float lw[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) lw[c] = a.lnw[c0 + c];

  const int slice0 = blockIdx.x * RG_SLICE_ROWS;
  for (int r0 = slice0; r0 < slice0 + RG_SLICE_ROWS && r0 < a.rows; r0 += RG_TILE) {
    const TcnRow o = tcn_rows_forward<DROP>(s, a, r0, lane, w);
    float zh[8], g[8], dy[8];
    {
      f32x4 d0 = {0.f, 0.f, 0.f, 0.f}, d1 = d0;
      if (o.live) { d0 = ld4(a.dY + (int64_t)o.r * RG_C + c0); d1 = ld4(a.dY + (int64_t)o.r * RG_C + c0 + 4); }
      dy[0] = d0.x; dy[1] = d0.y; dy[2] = d0.z; dy[3] = d0.w; dy[4] = d1.x; dy[5] = d1.y; dy[6] = d1.z; dy[7] = d1.w;
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      zh[c] = (o.z[c] - o.mean) * o.rs;
      g[c] = dy[c] * lw[c];
    }
    if (want_part) {
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        alw[c] += wave_sum(dy[c] * zh[c]);
        alb[c] += wave_sum(dy[c]);
      }
    }
    __syncthreads();                                     // every thread has read z of all channels (the statistics)
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      s.q[(c0 + c) * RG_PITCH + lane] = g[c];
      s.p[(c0 + c) * RG_PITCH + lane] = g[c] * zh[c];
    }
    __syncthreads();
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int c = 0; c < RG_C; ++c) { s1 += s.q[c * RG_PITCH + lane]; s2 += s.p[c * RG_PITCH + lane]; }
    s1 *= (1.0f / RG_C);
    s2 *= (1.0f / RG_C);
    float dz[8], dout[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      dz[c] = o.mf * (o.rs * ((g[c] - s1) - zh[c] * s2));
      dout[c] = DROP ? (((o.keep >> c) & 1u) ? dz[c] * a.scale : 0.f) : dz[c];
    }
    if (a.dX && o.live) {
      st4(a.dX + (int64_t)o.r * RG_C + c0, f32x4{dz[0], dz[1], dz[2], dz[3]});
      st4(a.dX + (int64_t)o.r * RG_C + c0 + 4, f32x4{dz[4], dz[5], dz[6], dz[7]});
    }
    __syncthreads();                                     // s1 / s2 have been read
#pragma unroll
    for (int c = 0; c < 8; ++c) s.p[(c0 + c) * RG_PITCH + lane] = dout[c];
    __syncthreads();
    // dh[ci] = (h[ci] > 0) sum_co Wp[co][ci] do[co], ci = c0 .. c0 + 7
    float dh[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) dh[c] = 0.f;
#pragma unroll 4
    for (int co = 0; co < RG_C; ++co) {
      const float dv = s.p[co * RG_PITCH + lane];
      const f32x4 w0 = ld4(s.wp + co * RG_C + c0), w1 = ld4(s.wp + co * RG_C + c0 + 4);
      dh[0] = __builtin_fmaf(w0.x, dv, dh[0]); dh[1] = __builtin_fmaf(w0.y, dv, dh[1]);
      dh[2] = __builtin_fmaf(w0.z, dv, dh[2]); dh[3] = __builtin_fmaf(w0.w, dv, dh[3]);
      dh[4] = __builtin_fmaf(w1.x, dv, dh[4]); dh[5] = __builtin_fmaf(w1.y, dv, dh[5]);
      dh[6] = __builtin_fmaf(w1.z, dv, dh[6]); dh[7] = __builtin_fmaf(w1.w, dv, dh[7]);
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      dh[c] = s.h[(c0 + c) * RG_PITCH + lane] > 0.f ? dh[c] : 0.f;       // ReLU passes nothing at h == 0
      s.q[(c0 + c) * RG_PITCH + lane] = dh[c];
    }
    if (a.dH && o.live) {
      st4(a.dH + (int64_t)o.r * RG_C + c0, f32x4{dh[0], dh[1], dh[2], dh[3]});
      st4(a.dH + (int64_t)o.r * RG_C + c0 + 4, f32x4{dh[4], dh[5], dh[6], dh[7]});
    }
    if (want_part) {
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        abp[c] += wave_sum(dout[c]);
        abd[c] += wave_sum(dh[c]);
      }
    }
    __syncthreads();                                     // do in s.p, dh in s.q, relu(h) in s.h, the taps in s.x: rows that are not live hold 0 in p and q
    if (a.want_wd) {
      const float* d0 = s.q + oco * RG_PITCH;
      const float* x0 = s.x + oci * RG_PITCH;
      for (int rr = 0; rr < RG_TILE; ++rr) {
        const float xa = x0[rr], xb = x0[RG_C * RG_PITCH + rr], xc = x0[2 * RG_C * RG_PITCH + rr];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float d = d0[i * RG_PITCH + rr];
          awd[i][0] = __builtin_fmaf(d, xa, awd[i][0]);
          awd[i][1] = __builtin_fmaf(d, xb, awd[i][1]);
          awd[i][2] = __builtin_fmaf(d, xc, awd[i][2]);
        }
      }
    }
    if (a.want_wp) {
      const float* d0 = s.p + oco * RG_PITCH;
      const float* h0 = s.h + oci * RG_PITCH;
      for (int rr = 0; rr < RG_TILE; ++rr) {
        const float hv = h0[rr];
#pragma unroll
        for (int i = 0; i < 4; ++i) awp[i] = __builtin_fmaf(d0[i * RG_PITCH + rr], hv, awp[i]);
      }
    }
    __syncthreads();                                     // the next tile overwrites x, h, p, q
  }
  if (!want_part) return;
  float* part = a.part + (int64_t)blockIdx.x * RG_P_N;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) part[RG_P_WD + ((oco + i) * RG_C + oci) * 3 + j] = awd[i][j];
    part[RG_P_WP + (oco + i) * RG_C + oci] = awp[i];
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      part[RG_P_BD + c0 + c] = abd[c];
      part[RG_P_BP + c0 + c] = abp[c];
      part[RG_P_LNW + c0 + c] = alw[c];
      part[RG_P_LNB + c0 + c] = alb[c];
    }
  }
}

// phase 2: dX[t, ci] = dz[t, ci] (left in dX by phase 1) + sum_j sum_co Wd[co, ci, j] dh[t - (j - 1) d, co], taps inside the sequence
__global__ __launch_bounds__(256) void k_tcn_bwd2(TcnLayerArgs a) {
  __shared__ __attribute__((aligned(16))) float s_w[3 * RG_C * RG_C];      // [tap * 32 + co][ci]
  __shared__ float s_d[3 * RG_T32];                                        // [tap * 32 + co][65]
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c0 = 8 * w;
  for (int i = tid; i < 3 * RG_C * RG_C; i += 256) {
    const int co = i / (3 * RG_C), rem = i - co * 3 * RG_C, ci = rem / 3, tap = rem - ci * 3;
    s_w[(tap * RG_C + co) * RG_C + ci] = a.Wd[i];
  }
  const int r = blockIdx.x * RG_TILE + lane;
  const bool live = r < a.rows;
  const int b = live ? r / a.T0 : 0, t = live ? r - b * a.T0 : 0;
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    const int f = w * 6 + q, tap = f >> 3, c4 = (f & 7) * 4;
    const int64_t tt = (int64_t)t - (int64_t)(tap - 1) * a.dil;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (live && tt >= 0 && tt < a.T0) v = ld4(a.dH + ((int64_t)r - (int64_t)(tap - 1) * a.dil) * RG_C + c4);
    float* dst = s_d + (tap * RG_C + c4) * RG_PITCH + lane;
    dst[0] = v.x; dst[RG_PITCH] = v.y; dst[2 * RG_PITCH] = v.z; dst[3 * RG_PITCH] = v.w;
  }
  __syncthreads();
  float acc[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) acc[c] = 0.f;
#pragma unroll 4
  for (int k = 0; k < 3 * RG_C; ++k) {
    const float dv = s_d[k * RG_PITCH + lane];
    const f32x4 w0 = ld4(s_w + k * RG_C + c0), w1 = ld4(s_w + k * RG_C + c0 + 4);
    acc[0] = __builtin_fmaf(w0.x, dv, acc[0]); acc[1] = __builtin_fmaf(w0.y, dv, acc[1]);
    acc[2] = __builtin_fmaf(w0.z, dv, acc[2]); acc[3] = __builtin_fmaf(w0.w, dv, acc[3]);
    acc[4] = __builtin_fmaf(w1.x, dv, acc[4]); acc[5] = __builtin_fmaf(w1.y, dv, acc[5]);
    acc[6] = __builtin_fmaf(w1.z, dv, acc[6]); acc[7] = __builtin_fmaf(w1.w, dv, acc[7]);
  }
  if (!live) return;
  float* dst = a.dX + (int64_t)r * RG_C + c0;
  const f32x4 z0 = ld4(dst), z1 = ld4(dst + 4);
  st4(dst, f32x4{z0.x + acc[0], z0.y + acc[1], z0.z + acc[2], z0.w + acc[3]});
  st4(dst + 4, f32x4{z1.x + acc[4], z1.y + acc[5], z1.z + acc[6], z1.w + acc[7]});
}

__global__ __launch_bounds__(256) void k_rg_reduce(const float* __restrict__ part, int nparts, TcnLayerOuts o, int accumulate) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= RG_P_N) return;
  float* out;
  if (i < RG_P_WP) out = o.dWd ? o.dWd + i : nullptr;
  else if (i < RG_P_BD) out = o.dWp ? o.dWp + (i - RG_P_WP) : nullptr;
  else if (i < RG_P_BP) out = o.dbd ? o.dbd + (i - RG_P_BD) : nullptr;
  else if (i < RG_P_LNW) out = o.dbp ? o.dbp + (i - RG_P_BP) : nullptr;
  else if (i < RG_P_LNB) out = o.dlnw ? o.dlnw + (i - RG_P_LNW) : nullptr;
  else out = o.dlnb ? o.dlnb + (i - RG_P_LNB) : nullptr;
  if (!out) return;
  const float sum = blocked_sum(part, nparts, (int64_t)RG_P_N, i);
  *out = accumulate ? *out + sum : sum;
}

static int tcn_check(const char* what, int B, int T0, int dil, float p, int layer, int b0) {
  DCF_CHECK(B > 0 && T0 > 0, "%s: empty batch (B = %d, T0 = %d)", what, B, T0);
  DCF_CHECK((int64_t)B * T0 < (1ll << 31) - 2 * RG_SLICE_ROWS, "%s: %lld rows (< 2^31)", what, (long long)B * T0);
  DCF_CHECK(dil >= 1 && dil <= (1 << 30), "%s: dilation = %d (1 to 2^30)", what, dil);
  DCF_CHECK(p >= 0.f && p < 1.f, "%s: p = %g outside [0, 1)", what, (double)p);
  DCF_CHECK(layer >= 0 && layer < 4096 && b0 >= 0, "%s: dropout site layer = %d, b0 = %d (layer 0 to 4095, b0 >= 0)", what, layer, b0);
  return 0;
}

static void tcn_fill(TcnLayerArgs& a, const float* X, const uint8_t* mask, const float* Wd, const float* bd, const float* Wp, const float* bp,
                     const float* lnw, const float* lnb, int B, int T0, int dil, int64_t seed, float p, int layer, int b0) {
  a.X = X; a.mask = mask; a.Wd = Wd; a.bd = bd; a.Wp = Wp; a.bp = bp; a.lnw = lnw; a.lnb = lnb;
  a.rows = B * T0; a.T0 = T0; a.dil = dil;
  a.seed = (uint64_t)seed; a.site = drop_site(DROP_G_REFINE, (uint32_t)layer, DROP_TCN); a.p = p; a.scale = 1.0f / (1.0f - p); a.b0 = b0;
}

}  // namespace dcf

using namespace dcf;

extern "C" {

static int refine_in_fill(const char* what, RefineInArgs& a, int B, int T0, int L) {
  DCF_CHECK(B > 0 && T0 > 0, "%s: empty batch (B = %d, T0 = %d)", what, B, T0);
  DCF_CHECK(L >= 1 && L <= RG_MAX_L, "%s: L = %d pyramid levels (1 to %d)", what, L, RG_MAX_L);
  DCF_CHECK(T0 % (1 << (L - 1)) == 0, "%s: T0 = %d is not a multiple of 2^(L-1) = %d", what, T0, 1 << (L - 1));
  DCF_CHECK((int64_t)B * T0 < (1ll << 31) - 2 * RG_SLICE_ROWS, "%s: %lld rows (< 2^31)", what, (long long)B * T0);
  a.rows = B * T0; a.T0 = T0; a.L = L;
  int acc = 0;
  for (int l = 0; l <= RG_MAX_L; ++l) {
    a.off[l] = acc;
    if (l < L) acc += T0 >> l;
  }
  a.S = acc;
  return 0;
}

int dcf_op_refine_in(const float* logits1, const uint8_t* mask0, const float* W_in, const float* b_in, float* H, int32_t B, int32_t T0,
                     int32_t L, void* stream) {
  DCF_CHECK(logits1 && W_in && b_in && H, "dcf_op_refine_in: null argument");
  RefineInArgs a{};
  if (refine_in_fill("dcf_op_refine_in", a, B, T0, L)) return -1;
  DCF_CHECK(aligned16(b_in) && aligned16(H), "dcf_op_refine_in: pointers must be 16-byte aligned");
  a.logits1 = logits1; a.mask0 = mask0; a.W = W_in; a.b = b_in; a.H = H;
  const int64_t n = (int64_t)a.rows * (RG_C / 4);
  hipLaunchKernelGGL(k_refine_in_fwd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  DCF_HIP(hipGetLastError());
  return 0;
}

int dcf_op_refine_in_bwd(const float* logits1, const uint8_t* mask0, const float* W_in, const float* dH, float* dlogits1, float* dW_in,
                         float* db_in, int32_t B, int32_t T0, int32_t L, int32_t accumulate, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  DCF_CHECK(dH, "dcf_op_refine_in_bwd: null dH");
  DCF_CHECK(!dlogits1 || W_in, "dcf_op_refine_in_bwd: dlogits1 needs W_in");
  DCF_CHECK(!dW_in || logits1, "dcf_op_refine_in_bwd: dW_in needs logits1");
  RefineInArgs a{};
  if (refine_in_fill("dcf_op_refine_in_bwd", a, B, T0, L)) return -1;
  DCF_CHECK(aligned16(dH), "dcf_op_refine_in_bwd: pointers must be 16-byte aligned");
  if (!dlogits1 && !dW_in && !db_in) return 0;
  a.logits1 = logits1; a.mask0 = mask0; a.W = W_in; a.dH = dH;
  const int slices = (a.rows + RG_SLICE_ROWS - 1) / RG_SLICE_ROWS;                  // a fixed function of the row count
  const int per = RG_C * (L + 1);
  StreamScratch sc(st);
  if (dlogits1 && sc.take(&a.dU, (size_t)a.rows * L)) return -1;
  if ((dW_in || db_in) && sc.take(&a.part, (size_t)slices * per)) return -1;
  int rc = 0;
  hipLaunchKernelGGL(k_refine_in_bwd, dim3(slices), dim3(256), 0, st, a);
  if (dlogits1) {
    const int64_t n = (int64_t)B * a.S;
    hipLaunchKernelGGL(k_refine_in_gather, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, dlogits1, B);
  }
  if (a.part) hipLaunchKernelGGL(k_refine_in_reduce, dim3((per + 255) / 256), dim3(256), 0, st, (const float*)a.part, slices, L, dW_in, db_in, accumulate);
  if (hipGetLastError() != hipSuccess) { set_error("dcf_op_refine_in_bwd: launch failed"); rc = -1; }
  return sc.end(rc);
}

int dcf_op_tcn_layer(const float* X, const uint8_t* mask, const float* Wd, const float* bd, const float* Wp, const float* bp,
                     const float* ln_w, const float* ln_b, float* Y, int32_t B, int32_t T0, int32_t dilation, int64_t seed, float p,
                     int32_t layer, int32_t b0, void* stream) {
  DCF_CHECK(X && Wd && bd && Wp && bp && ln_w && ln_b && Y, "dcf_op_tcn_layer: null argument");
  if (tcn_check("dcf_op_tcn_layer", B, T0, dilation, p, layer, b0)) return -1;
  DCF_CHECK(aligned16(X) && aligned16(Y) && aligned16(ln_w) && aligned16(ln_b), "dcf_op_tcn_layer: pointers must be 16-byte aligned");
  TcnLayerArgs a{};
  tcn_fill(a, X, mask, Wd, bd, Wp, bp, ln_w, ln_b, B, T0, dilation, seed, p, layer, b0);
  a.Y = Y;
  const dim3 grid((a.rows + RG_TILE - 1) / RG_TILE);
  const size_t lds = RG_LDS_FWD * sizeof(float);
  if (p > 0.f) hipLaunchKernelGGL(k_rg_tcn_fwd<true>, grid, dim3(256), lds, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(k_rg_tcn_fwd<false>, grid, dim3(256), lds, (hipStream_t)stream, a);
  DCF_HIP(hipGetLastError());
  return 0;
}

int dcf_op_tcn_layer_bwd(const float* X, const uint8_t* mask, const float* Wd, const float* bd, const float* Wp, const float* bp,
                         const float* ln_w, const float* ln_b, const float* dY, float* dX, float* dWd, float* dbd, float* dWp, float* dbp,
                         float* dln_w, float* dln_b, int32_t B, int32_t T0, int32_t dilation, int64_t seed, float p, int32_t layer,
                         int32_t b0, int32_t accumulate, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  DCF_CHECK(X && Wd && bd && Wp && bp && ln_w && ln_b && dY, "dcf_op_tcn_layer_bwd: null argument");
  if (tcn_check("dcf_op_tcn_layer_bwd", B, T0, dilation, p, layer, b0)) return -1;
  DCF_CHECK(aligned16(X) && aligned16(dY) && aligned16(dX), "dcf_op_tcn_layer_bwd: pointers must be 16-byte aligned");
  const bool want_part = dWd || dbd || dWp || dbp || dln_w || dln_b;
  if (!dX && !want_part) return 0;
  TcnLayerArgs a{};
  tcn_fill(a, X, mask, Wd, bd, Wp, bp, ln_w, ln_b, B, T0, dilation, seed, p, layer, b0);
  a.dY = dY; a.dX = dX; a.want_wd = dWd != nullptr; a.want_wp = dWp != nullptr;
  constexpr size_t lds = RG_LDS_BWD * sizeof(float);    // phase 1 needs more than the 64 KiB of LDS a launch gets by default
  if (p > 0.f ? raise_lds_limit<&k_tcn_bwd1<true>>(lds) : raise_lds_limit<&k_tcn_bwd1<false>>(lds)) return -1;
  const int slices = (a.rows + RG_SLICE_ROWS - 1) / RG_SLICE_ROWS;                  // a fixed function of the row count
  StreamScratch sc(st);
  if (dX && sc.take(&a.dH, (size_t)a.rows * RG_C)) return -1;
  if (want_part && sc.take(&a.part, (size_t)slices * RG_P_N)) return -1;
  int rc = 0;
  if (p > 0.f) hipLaunchKernelGGL(k_tcn_bwd1<true>, dim3(slices), dim3(256), lds, st, a);
  else hipLaunchKernelGGL(k_tcn_bwd1<false>, dim3(slices), dim3(256), lds, st, a);
  if (dX) hipLaunchKernelGGL(k_tcn_bwd2, dim3((a.rows + RG_TILE - 1) / RG_TILE), dim3(256), 0, st, a);
  if (want_part) {
    const TcnLayerOuts o{dWd, dbd, dWp, dbp, dln_w, dln_b};
    hipLaunchKernelGGL(k_rg_reduce, dim3((RG_P_N + 255) / 256), dim3(256), 0, st, (const float*)a.part, slices, o, accumulate);
  }
  if (hipGetLastError() != hipSuccess) { set_error("dcf_op_tcn_layer_bwd: launch failed"); rc = -1; }
  return sc.end(rc);
}

}  // extern "C"
