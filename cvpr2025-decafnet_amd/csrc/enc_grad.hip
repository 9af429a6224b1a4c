// Forward / backward pairs of the operators a TransformerEncoder block (libs/modeling/blocks.py:541-591) needs besides the dense
// MaskedConv1D, the channel LayerNorm (conv_grad.hip) and the sliding-window attention (attn_grad.hip), on token-major (B*T, C)
// fp32 rows:
//
//   depthwise convolution (blocks.py:87-106 with groups = C, k = 3, padding 1, no bias, stride s = 1 / 2; the q / k / v_conv of
//   ConvAttNLayer :437-445 share one input, so n of them run in one pass over X)
//       Y_i[b,o,c] = sum_j W_i[c,j] m[b,s o+j-1] X[b,s o+j-1,c]                      (taps stay inside sequence b; Y is not masked)
//       dX[b,t,c]  = m[b,t] sum_i sum_j dY_i[b,o,c] W_i[c,j]   over s o + j - 1 = t   (a gather per input row, i then j ascending)
//       dW_i[c,j]  = sum_{b,o} dY_i[b,o,c] m X[b,s o+j-1,c]
//   masked_max_pool1d (blocks.py:31-47; kernel 3, stride 2, padding 1)
//       f[b,t,c] = m[b,t] ? X[b,t,c] : min_t' X[b,t',c]   (the minimum is detached, :38),  mo[b,o] = any m in the window
//       Y[b,o,c] = mo[b,o] max_{t in {2o-1, 2o, 2o+1}, 0 <= t < T} f[b,t,c]
//       dX[b,t,c] = m[b,t] sum over the (at most two) windows o whose maximum sits at t of dY[b,o,c] mo[b,o];  among equal values
//       the lowest position holds the maximum, and the choice is made on f -- a padded slot can win and swallow the gradient
//   GELU (blocks.py:531, erf form)     y = x Phi(x),   dx = dy (Phi(x) + x phi(x))
//   LayerScale residual (blocks.py:586, :589-590, :670-682)
//       Y = R m_R + ls (H m_H),   dR = dY m_R,   dH = ls dY m_H,   dls[c] = sum_rows dY H m_H
//
// All of it is streaming work on the vector ALU with 16-byte accesses.  The elementwise kernels give a thread one f32x4; the two
// column reductions (dW, dls) follow k_ln_bwd (conv_grad.hip): a wave owns a run of rows, a lane four channels of a 256-channel
// chunk (blockIdx.y), sums stay in registers, four waves meet in LDS, and k_eg_reduce adds the workgroup partials in a fixed order
// (blocked_sum, grad_common.h).  No floating-point atomics, one summation order:
// results are bit-identical from run to run, and every product has the upstream gradient as one factor, so scaling it by a power of
// two scales the results by exactly that.
//
// Accuracy of the GELU pair.  The forward's gelu_erf (common.h) is Abramowitz & Stegun 7.1.26, |error| 1.5e-7 in erf: rounding level
// for a forward value, but the gradient rule of the tests leaves 2^-21 of the largest element for everything.  Here Phi comes from
// erfcf of |x| / sqrt 2 (no cancellation in the lower tail: Phi(-6) = 1e-9 keeps its relative accuracy) and phi from expf of the
// rounded -x^2 / 2 times 1 - (the rounding residual of x^2) / 2.
#include <math.h>

#include "../../include/decafnet_hip.h"
#include "enc_grad.h"
#include "grad_common.h"

namespace dcf {

static inline unsigned eg_grid(int64_t n, int per_block) {
  const int64_t g = (n + per_block - 1) / per_block;
  return (unsigned)(g < 1 ? 1 : (g > (1 << 20) ? (1 << 20) : g));
}

// the three taps of four adjacent channels: W (C, 3) rows c .. c + 3 are 12 consecutive floats; w[j] = tap j of the four channels
__device__ __forceinline__ void load_taps(const float* __restrict__ W, f32x4* w) {
  const f32x4 a = ld4(W), b = ld4(W + 4), c = ld4(W + 8);
  w[0] = f32x4{a.x, a.w, b.z, c.y};
  w[1] = f32x4{a.y, b.x, b.w, c.z};
  w[2] = f32x4{a.z, b.y, c.x, c.w};
}

__device__ __forceinline__ f32x4 fma4(const f32x4& a, const f32x4& b, const f32x4& c) {
  return f32x4{__builtin_fmaf(a.x, b.x, c.x), __builtin_fmaf(a.y, b.y, c.y), __builtin_fmaf(a.z, b.z, c.z), __builtin_fmaf(a.w, b.w, c.w)};
}

// ------------------------------------------------------------------------------------------
// depthwise convolution
// ------------------------------------------------------------------------------------------
template <int N>
__global__ __launch_bounds__(256) void k_dw_fwd(const float* __restrict__ X, const uint8_t* __restrict__ mask, const float* __restrict__ W,
                                                float* __restrict__ Y, int B, int T, int To, int C, int stride) {
  const int c4n = C / 4;
  const int64_t rows_out = (int64_t)B * To, total = rows_out * c4n;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t ro = i / c4n;
    const int c = (int)(i - ro * c4n) * 4;
    const int b = (int)(ro / To), o = (int)(ro - (int64_t)b * To);
    f32x4 x[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int u = stride * o - 1 + j;
      const bool ok = u >= 0 && u < T && (!mask || mask[(int64_t)b * T + u]);
      x[j] = ok ? ld4(X + ((int64_t)b * T + u) * C + c) : zero4();
    }
#pragma unroll
    for (int n = 0; n < N; ++n) {
      f32x4 w[3];
      load_taps(W + ((int64_t)n * C + c) * 3, w);
      const f32x4 y = fma4(x[2], w[2], fma4(x[1], w[1], x[0] * w[0]));
      st4(Y + ((int64_t)n * rows_out + ro) * C + c, y);
    }
  }
}

template <int N>
__global__ __launch_bounds__(256) void k_dw_bwd_x(const float* __restrict__ dY, const uint8_t* __restrict__ mask, const float* __restrict__ W,
                                                  float* __restrict__ dX, int B, int T, int To, int C, int stride) {
  const int c4n = C / 4;
  const int64_t rows_out = (int64_t)B * To, total = (int64_t)B * T * c4n;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / c4n;
    const int c = (int)(i - r * c4n) * 4;
    const int b = (int)(r / T), t = (int)(r - (int64_t)b * T);
    f32x4 acc = zero4();
    if (!mask || mask[r]) {
#pragma unroll
      for (int n = 0; n < N; ++n) {
        f32x4 w[3];
        load_taps(W + ((int64_t)n * C + c) * 3, w);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const int num = t + 1 - j;                     // s o = t + 1 - j
          if (num < 0 || num % stride != 0) continue;
          const int o = num / stride;
          if (o >= To) continue;
          acc = fma4(ld4(dY + ((int64_t)n * rows_out + (int64_t)b * To + o) * C + c), w[j], acc);
        }
      }
    }
    st4(dX + r * C + c, acc);
  }
}

template <int N>
__global__ __launch_bounds__(256) void k_dw_bwd_w(DwGradArgs p) {
  extern __shared__ __attribute__((aligned(16))) float s_dw[];                     // [4 waves][N * 3][256]
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int C = p.C, T = p.T, To = p.To;
  const int c = 256 * blockIdx.y + 4 * lane;
  const bool act = c < C;
  const int64_t rows_out = (int64_t)p.B * To;
  const int64_t r_begin = ((int64_t)blockIdx.x * 4 + wave) * p.rows_per_wave;
  const int64_t r_end = r_begin + p.rows_per_wave < rows_out ? r_begin + p.rows_per_wave : rows_out;
  f32x4 acc[N][3];
#pragma unroll
  for (int n = 0; n < N; ++n)
#pragma unroll
    for (int j = 0; j < 3; ++j) acc[n][j] = zero4();
  for (int64_t r = r_begin; r < r_end; ++r) {
    const int b = (int)(r / To), o = (int)(r - (int64_t)b * To);
    f32x4 x[3], dy[N];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int u = p.stride * o - 1 + j;
      const bool ok = act && u >= 0 && u < T && (!p.mask || p.mask[(int64_t)b * T + u]);
      x[j] = ok ? ld4(p.X + ((int64_t)b * T + u) * C + c) : zero4();
    }
#pragma unroll
    for (int n = 0; n < N; ++n) dy[n] = act ? ld4(p.dY + ((int64_t)n * rows_out + r) * C + c) : zero4();
#pragma unroll
    for (int n = 0; n < N; ++n)
#pragma unroll
      for (int j = 0; j < 3; ++j) acc[n][j] = fma4(dy[n], x[j], acc[n][j]);
  }
#pragma unroll
  for (int n = 0; n < N; ++n)
#pragma unroll
    for (int j = 0; j < 3; ++j) st4(s_dw + ((wave * N + n) * 3 + j) * 256 + 4 * lane, acc[n][j]);
  __syncthreads();
  constexpr int PER = N * 3 * 256;
  for (int i = threadIdx.x; i < PER; i += 256) {
    const int nj = i >> 8, cg = 256 * blockIdx.y + (i & 255);
    if (cg < C) p.part[((int64_t)blockIdx.x * N * 3 + nj) * C + cg] = (s_dw[i] + s_dw[PER + i]) + (s_dw[2 * PER + i] + s_dw[3 * PER + i]);
  }
}

// out[o(i)] (+)= sum_s part[s][i] in the fixed blocked order of blocked_sum (grad_common.h).  KT = 3: part is laid out [n][j][c], out is
// PyTorch's [n][c][j].
__global__ __launch_bounds__(256) void k_eg_reduce(const float* __restrict__ part, int nparts, int64_t stride, int count, float* __restrict__ out,
                                                   int KT, int C, int accumulate) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  float sum = 0.f;
  DCF_BLOCKED_SUM(sum, part, nparts, stride, i);
  int o = i;
  if (KT > 1) {
    const int n = i / (KT * C), rem = i - n * KT * C, j = rem / C, c = rem - j * C;
    o = (n * C + c) * KT + j;
  }
  out[o] = accumulate ? out[o] + sum : sum;
}

void launch_eg_reduce(const float* part, int nparts, int64_t stride, int count, float* out, int KT, int C, int accumulate, hipStream_t st) {
  hipLaunchKernelGGL(k_eg_reduce, dim3((count + 255) / 256), dim3(256), 0, st, part, nparts, stride, count, out, KT, C, accumulate);
}

// ------------------------------------------------------------------------------------------
// masked max pooling (kernel 3, stride 2, padding 1)
// ------------------------------------------------------------------------------------------
// per (sequence, row slice): the minimum of every channel over the slice's rows (all rows, padded ones too: blocks.py:38 is taken
// before the mask is applied)
__global__ __launch_bounds__(256) void k_colmin_part(const float* __restrict__ X, float* __restrict__ part, int T, int C, int slice_rows, int S) {
  __shared__ __attribute__((aligned(16))) float s_min[4 * 256];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.x / S, s = blockIdx.x - b * S;
  const int t_begin = s * slice_rows, t_end = t_begin + slice_rows < T ? t_begin + slice_rows : T;
  const int c = 256 * blockIdx.y + 4 * lane;
  const bool act = c < C;
  f32x4 m = f32x4{INFINITY, INFINITY, INFINITY, INFINITY};
  if (act) {
    for (int t = t_begin + wave; t < t_end; t += 4) {
      const f32x4 v = ld4(X + ((int64_t)b * T + t) * C + c);
      m.x = fminf(m.x, v.x); m.y = fminf(m.y, v.y); m.z = fminf(m.z, v.z); m.w = fminf(m.w, v.w);
    }
  }
  st4(s_min + wave * 256 + 4 * lane, m);
  __syncthreads();
  const int i = threadIdx.x, cg = 256 * blockIdx.y + i;
  if (cg < C) part[(int64_t)blockIdx.x * C + cg] = fminf(fminf(s_min[i], s_min[256 + i]), fminf(s_min[512 + i], s_min[768 + i]));
}

__global__ __launch_bounds__(256) void k_colmin_final(const float* __restrict__ part, float* __restrict__ xmin, int B, int C, int S) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * C) return;
  const int b = i / C, c = i - b * C;
  float m = INFINITY;
  for (int s = 0; s < S; ++s) m = fminf(m, part[((int64_t)b * S + s) * C + c]);
  xmin[i] = m;
}

__global__ __launch_bounds__(256) void k_pool_fwd(const float* __restrict__ X, const uint8_t* __restrict__ mask, const float* __restrict__ xmin,
                                                  float* __restrict__ Y, uint8_t* __restrict__ mask_out, int B, int T, int C) {
  const int c4n = C / 4, To = T / 2;
  const int64_t total = (int64_t)B * To * c4n;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t ro = i / c4n;
    const int c = (int)(i - ro * c4n) * 4;
    const int b = (int)(ro / To), o = (int)(ro - (int64_t)b * To);
    const f32x4 fill = mask ? ld4(xmin + (int64_t)b * C + c) : zero4();
    f32x4 best = zero4();
    bool any = false, first = true;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int u = 2 * o - 1 + j;                       // u <= 2 To - 1 = T - 1
      if (u < 0) continue;
      const int64_t r = (int64_t)b * T + u;
      const bool m = !mask || mask[r];
      const f32x4 v = m ? ld4(X + r * C + c) : fill;
      any |= m;
      if (first) { best = v; first = false; }
      else {
        best.x = v.x > best.x ? v.x : best.x; best.y = v.y > best.y ? v.y : best.y;
        best.z = v.z > best.z ? v.z : best.z; best.w = v.w > best.w ? v.w : best.w;
      }
    }
    st4(Y + ro * C + c, any ? best : zero4());
    if (mask_out && c == 0) mask_out[ro] = any ? 1 : 0;
  }
}

// a thread owns window o and the input rows 2 o, 2 o + 1 of four channels: row 2 o lies in window o alone, row 2 o + 1 in windows o
// (last slot) and o + 1 (first slot)
__global__ __launch_bounds__(256) void k_pool_bwd(const float* __restrict__ X, const uint8_t* __restrict__ mask, const float* __restrict__ xmin,
                                                  const float* __restrict__ dY, float* __restrict__ dX, int B, int T, int C) {
  const int c4n = C / 4, To = T / 2;
  const int64_t total = (int64_t)B * To * c4n;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t ro = i / c4n;
    const int c = (int)(i - ro * c4n) * 4;
    const int b = (int)(ro / To), o = (int)(ro - (int64_t)b * To);
    const bool ex0 = o > 0, ex1 = o + 1 < To;            // slot 2 o - 1 exists; window o + 1 (rows 2 o + 1 .. 2 o + 3 <= T - 1) exists
    const f32x4 fill = mask ? ld4(xmin + (int64_t)b * C + c) : zero4();
    f32x4 f[5];
    bool m[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const int u = 2 * o - 1 + k;
      const bool ex = k == 0 ? ex0 : (k >= 3 ? ex1 : true);
      const int64_t r = (int64_t)b * T + u;
      m[k] = ex && (!mask || mask[r]);
      f[k] = m[k] ? ld4(X + r * C + c) : fill;           // (a slot that does not exist is never compared)
    }
    const bool mo0 = m[0] || m[1] || m[2], mo1 = ex1 && (m[2] || m[3] || m[4]);
    const f32x4 g0 = mo0 ? ld4(dY + ro * C + c) : zero4();
    const f32x4 g1 = mo1 ? ld4(dY + (ro + 1) * C + c) : zero4();
    f32x4 de, dod;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      int s0;
      float bst;
      if (ex0) { s0 = 0; bst = f[0][e]; if (f[1][e] > bst) { s0 = 1; bst = f[1][e]; } }
      else { s0 = 1; bst = f[1][e]; }
      if (f[2][e] > bst) s0 = 2;
      int s1 = 0;
      bst = f[2][e];
      if (f[3][e] > bst) { s1 = 1; bst = f[3][e]; }
      if (f[4][e] > bst) s1 = 2;
      de[e] = (m[1] && s0 == 1) ? g0[e] : 0.f;
      dod[e] = m[2] ? ((s0 == 2 ? g0[e] : 0.f) + ((ex1 && s1 == 0) ? g1[e] : 0.f)) : 0.f;
    }
    st4(dX + ((int64_t)b * T + 2 * o) * C + c, de);
    st4(dX + ((int64_t)b * T + 2 * o + 1) * C + c, dod);
  }
}

// ------------------------------------------------------------------------------------------
// GELU
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gelu_fwd(const float* __restrict__ X, float* __restrict__ Y, int64_t n) {
  const int64_t n4 = n / 4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const f32x4 x = ld4(X + 4 * i);
    st4(Y + 4 * i, f32x4{gelu_exact(x.x), gelu_exact(x.y), gelu_exact(x.z), gelu_exact(x.w)});
  }
  const int64_t tail = 4 * n4 + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x < 4 && tail < n) Y[tail] = gelu_exact(X[tail]);
}

__global__ __launch_bounds__(256) void k_gelu_bwd(const float* __restrict__ X, const float* __restrict__ dY, float* __restrict__ dX, int64_t n) {
  const int64_t n4 = n / 4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const f32x4 x = ld4(X + 4 * i), g = ld4(dY + 4 * i);
    st4(dX + 4 * i, f32x4{g.x * gelu_slope(x.x), g.y * gelu_slope(x.y), g.z * gelu_slope(x.z), g.w * gelu_slope(x.w)});
  }
  const int64_t tail = 4 * n4 + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x < 4 && tail < n) dX[tail] = dY[tail] * gelu_slope(X[tail]);
}

// ------------------------------------------------------------------------------------------
// LayerScale residual
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ls_fwd(const float* __restrict__ R, const uint8_t* __restrict__ mR, const float* __restrict__ H,
                                                const uint8_t* __restrict__ mH, const float* __restrict__ ls, float* __restrict__ Y, int64_t rows,
                                                int C) {
  const int c4n = C / 4;
  const int64_t total = rows * c4n;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / c4n;
    const int c = (int)(i - r * c4n) * 4;
    f32x4 y = (!mR || mR[r]) ? ld4(R + r * C + c) : zero4();
    if (H && (!mH || mH[r])) y = fma4(ld4(ls + c), ld4(H + r * C + c), y);
    st4(Y + r * C + c, y);
  }
}

__global__ __launch_bounds__(256) void k_ls_bwd(LsGradArgs p) {
  __shared__ __attribute__((aligned(16))) float s_ls[4 * 256];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int C = p.C;
  const int c = 256 * blockIdx.y + 4 * lane;
  const bool act = c < C;
  const int64_t r_begin = ((int64_t)blockIdx.x * 4 + wave) * p.rows_per_wave;
  const int64_t r_end = r_begin + p.rows_per_wave < p.rows ? r_begin + p.rows_per_wave : (int64_t)p.rows;
  const bool want_h = p.H != nullptr && (p.part != nullptr);
  const f32x4 ls = (act && p.dH) ? ld4(p.ls + c) : zero4();
  f32x4 acc = zero4();
  f32x4 gn = zero4(), hn = zero4();
  if (act && r_begin < r_end) {
    gn = ld4(p.dY + r_begin * C + c);
    if (want_h) hn = ld4(p.H + r_begin * C + c);
  }
  for (int64_t r = r_begin; r < r_end; ++r) {
    const f32x4 g = gn, h = hn;
    if (act && r + 1 < r_end) {                          // the next row travels while this one is used
      gn = ld4(p.dY + (r + 1) * C + c);
      if (want_h) hn = ld4(p.H + (r + 1) * C + c);
    }
    const bool mr = !p.mR || p.mR[r], mh = !p.mH || p.mH[r];
    if (act) {
      if (p.dR) st4(p.dR + r * C + c, mr ? g : zero4());
      if (p.dH) st4(p.dH + r * C + c, mh ? ls * g : zero4());
      if (want_h && mh) acc = fma4(g, h, acc);
    }
  }
  if (!p.part) return;
  st4(s_ls + wave * 256 + 4 * lane, acc);
  __syncthreads();
  const int i = threadIdx.x, cg = 256 * blockIdx.y + i;
  if (cg < C) p.part[(int64_t)blockIdx.x * C + cg] = (s_ls[i] + s_ls[256 + i]) + (s_ls[512 + i] + s_ls[768 + i]);
}

}  // namespace dcf

using namespace dcf;

#define EG_LAUNCHED(what)                                                            \
  do {                                                                               \
    if (hipGetLastError() != hipSuccess) { set_error(what ": launch failed"); rc = -1; } \
  } while (0)

static int dw_check(const char* what, int B, int T, int C, int n, int stride) {
  DCF_CHECK(B > 0 && T > 0, "%s: empty batch (B = %d, T = %d)", what, B, T);
  DCF_CHECK(stride == 1 || stride == 2, "%s: stride = %d (1 or 2)", what, stride);
  DCF_CHECK(T % stride == 0, "%s: T = %d is not a multiple of the stride %d", what, T, stride);
  DCF_CHECK(C > 0 && C % 4 == 0 && C <= 1024, "%s: C = %d must be a multiple of 4 up to 1024", what, C);
  DCF_CHECK(n >= 1 && n <= 3, "%s: n = %d convolutions (1 to 3)", what, n);
  DCF_CHECK((int64_t)B * T < (1ll << 31) - 64, "%s: %lld rows (< 2^31)", what, (long long)B * T);
  return 0;
}

extern "C" {

int dcf_op_dwconv3(const float* X, const uint8_t* mask, const float* W, float* Y, int32_t B, int32_t T, int32_t C, int32_t n,
                   int32_t stride, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  DCF_CHECK(X && W && Y, "dcf_op_dwconv3: null argument");
  if (dw_check("dcf_op_dwconv3", B, T, C, n, stride)) return -1;
  DCF_CHECK(aligned16(X) && aligned16(W) && aligned16(Y), "dcf_op_dwconv3: pointers must be 16-byte aligned");
  const int To = T / stride;
  const dim3 grid(eg_grid((int64_t)B * To * (C / 4), 256));
  if (n == 1) hipLaunchKernelGGL(k_dw_fwd<1>, grid, dim3(256), 0, st, X, mask, W, Y, B, T, To, C, stride);
  else if (n == 2) hipLaunchKernelGGL(k_dw_fwd<2>, grid, dim3(256), 0, st, X, mask, W, Y, B, T, To, C, stride);
  else hipLaunchKernelGGL(k_dw_fwd<3>, grid, dim3(256), 0, st, X, mask, W, Y, B, T, To, C, stride);
  DCF_HIP(hipGetLastError());
  return 0;
}

int dcf_op_dwconv3_bwd(const float* X, const uint8_t* mask, const float* W, const float* dY, float* dX, float* dW, int32_t B, int32_t T,
                       int32_t C, int32_t n, int32_t stride, int32_t accumulate, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  DCF_CHECK(dY, "dcf_op_dwconv3_bwd: null dY");
  DCF_CHECK(!dX || W, "dcf_op_dwconv3_bwd: dX needs W");
  DCF_CHECK(!dW || X, "dcf_op_dwconv3_bwd: dW needs X");
  if (dw_check("dcf_op_dwconv3_bwd", B, T, C, n, stride)) return -1;
  DCF_CHECK(aligned16(X) && aligned16(W) && aligned16(dY) && aligned16(dX), "dcf_op_dwconv3_bwd: pointers must be 16-byte aligned");
  const int To = T / stride;
  int rc = 0;
  if (dX) {
    const dim3 grid(eg_grid((int64_t)B * T * (C / 4), 256));
    if (n == 1) hipLaunchKernelGGL(k_dw_bwd_x<1>, grid, dim3(256), 0, st, dY, mask, W, dX, B, T, To, C, stride);
    else if (n == 2) hipLaunchKernelGGL(k_dw_bwd_x<2>, grid, dim3(256), 0, st, dY, mask, W, dX, B, T, To, C, stride);
    else hipLaunchKernelGGL(k_dw_bwd_x<3>, grid, dim3(256), 0, st, dY, mask, W, dX, B, T, To, C, stride);
    DCF_HIP(hipGetLastError());
  }
  if (dW) {
    DwGradArgs a{};
    a.X = X; a.mask = mask; a.dY = dY; a.B = B; a.T = T; a.To = To; a.C = C; a.stride = stride;
    const int64_t rows_out = (int64_t)B * To;
    a.rows_per_wave = (int)((rows_out + 4 * EG_MAX_WG - 1) / (4 * EG_MAX_WG));       // a fixed function of the row count
    const int nwg = (int)((rows_out + 4 * a.rows_per_wave - 1) / (4 * a.rows_per_wave));
    const int count = n * 3 * C;
    StreamScratch sc(st);
    float* part = nullptr;
    if (sc.take(&part, (size_t)nwg * count)) return -1;
    a.part = part;
    const dim3 grid(nwg, (C + 255) / 256);
    const size_t lds = (size_t)4 * n * 3 * 256 * sizeof(float);
    if (n == 1) hipLaunchKernelGGL(k_dw_bwd_w<1>, grid, dim3(256), lds, st, a);
    else if (n == 2) hipLaunchKernelGGL(k_dw_bwd_w<2>, grid, dim3(256), lds, st, a);
    else hipLaunchKernelGGL(k_dw_bwd_w<3>, grid, dim3(256), lds, st, a);
    hipLaunchKernelGGL(k_eg_reduce, dim3((count + 255) / 256), dim3(256), 0, st, part, nwg, (int64_t)count, count, dW, 3, C, accumulate);
    EG_LAUNCHED("dcf_op_dwconv3_bwd");
    rc = sc.end(rc);
  }
  return rc;
}

static int pool_check(const char* what, int B, int T, int C) {
  DCF_CHECK(B > 0 && T > 0, "%s: empty batch (B = %d, T = %d)", what, B, T);
  DCF_CHECK(T % 2 == 0, "%s: T = %d is not a multiple of the stride 2", what, T);
  DCF_CHECK(C > 0 && C % 4 == 0 && C <= 1024, "%s: C = %d must be a multiple of 4 up to 1024", what, C);
  DCF_CHECK((int64_t)B * T < (1ll << 31) - 64, "%s: %lld rows (< 2^31)", what, (long long)B * T);
  return 0;
}

// xmin (B, C): the fill value of padded slots, on `st`; *out lives in the caller's scratch `sc`
static int pool_fill(const float* X, int B, int T, int C, float** out, StreamScratch& sc, hipStream_t st) {
  int slice_rows = (T + EG_MIN_SLICES - 1) / EG_MIN_SLICES;
  slice_rows = slice_rows < 256 ? 256 : slice_rows;
  const int S = (T + slice_rows - 1) / slice_rows;
  float *part = nullptr, *xmin = nullptr;
  if (sc.take(&part, (size_t)B * S * C) || sc.take(&xmin, (size_t)B * C)) return -1;
  hipLaunchKernelGGL(k_colmin_part, dim3(B * S, (C + 255) / 256), dim3(256), 0, st, X, part, T, C, slice_rows, S);
  hipLaunchKernelGGL(k_colmin_final, dim3((B * C + 255) / 256), dim3(256), 0, st, (const float*)part, xmin, B, C, S);
  if (hipGetLastError() != hipSuccess) {
    set_error("masked max pooling: launch failed");
    return -1;
  }
  *out = xmin;
  return 0;
}

int dcf_op_masked_maxpool(const float* X, const uint8_t* mask, float* Y, uint8_t* mask_out, int32_t B, int32_t T, int32_t C, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  DCF_CHECK(X && Y, "dcf_op_masked_maxpool: null argument");
  if (pool_check("dcf_op_masked_maxpool", B, T, C)) return -1;
  DCF_CHECK(aligned16(X) && aligned16(Y), "dcf_op_masked_maxpool: pointers must be 16-byte aligned");
  StreamScratch sc(st);
  float* xmin = nullptr;                                 // without a mask no slot is padded: nothing to fill
  if (mask && pool_fill(X, B, T, C, &xmin, sc, st)) return -1;
  int rc = 0;
  hipLaunchKernelGGL(k_pool_fwd, dim3(eg_grid((int64_t)B * (T / 2) * (C / 4), 256)), dim3(256), 0, st, X, mask, (const float*)xmin, Y, mask_out, B,
                     T, C);
  EG_LAUNCHED("dcf_op_masked_maxpool");
  return sc.end(rc);
}

int dcf_op_masked_maxpool_bwd(const float* X, const uint8_t* mask, const float* dY, float* dX, int32_t B, int32_t T, int32_t C,
                              void* stream) {
  hipStream_t st = (hipStream_t)stream;
  DCF_CHECK(X && dY && dX, "dcf_op_masked_maxpool_bwd: null argument");
  if (pool_check("dcf_op_masked_maxpool_bwd", B, T, C)) return -1;
  DCF_CHECK(aligned16(X) && aligned16(dY) && aligned16(dX), "dcf_op_masked_maxpool_bwd: pointers must be 16-byte aligned");
  StreamScratch sc(st);
  float* xmin = nullptr;
  if (mask && pool_fill(X, B, T, C, &xmin, sc, st)) return -1;
  int rc = 0;
  hipLaunchKernelGGL(k_pool_bwd, dim3(eg_grid((int64_t)B * (T / 2) * (C / 4), 256)), dim3(256), 0, st, X, mask, (const float*)xmin, dY, dX, B, T,
                     C);
  EG_LAUNCHED("dcf_op_masked_maxpool_bwd");
  return sc.end(rc);
}

int dcf_op_gelu(const float* X, float* Y, int64_t n, void* stream) {
  DCF_CHECK(X && Y && n > 0, "dcf_op_gelu: null argument or no elements");
  DCF_CHECK(aligned16(X) && aligned16(Y), "dcf_op_gelu: pointers must be 16-byte aligned");
  hipLaunchKernelGGL(k_gelu_fwd, dim3(eg_grid(n / 4, 256)), dim3(256), 0, (hipStream_t)stream, X, Y, n);
  DCF_HIP(hipGetLastError());
  return 0;
}

int dcf_op_gelu_bwd(const float* X, const float* dY, float* dX, int64_t n, void* stream) {
  DCF_CHECK(X && dY && dX && n > 0, "dcf_op_gelu_bwd: null argument or no elements");
  DCF_CHECK(aligned16(X) && aligned16(dY) && aligned16(dX), "dcf_op_gelu_bwd: pointers must be 16-byte aligned");
  hipLaunchKernelGGL(k_gelu_bwd, dim3(eg_grid(n / 4, 256)), dim3(256), 0, (hipStream_t)stream, X, dY, dX, n);
  DCF_HIP(hipGetLastError());
  return 0;
}

int dcf_op_layerscale_residual(const float* R, const uint8_t* mR, const float* H, const uint8_t* mH, const float* ls, float* Y, int32_t rows,
                               int32_t C, void* stream) {
  DCF_CHECK(R && Y && rows > 0, "dcf_op_layerscale_residual: null argument or no rows");
  DCF_CHECK(!H || ls, "dcf_op_layerscale_residual: H without a scale");
  DCF_CHECK(C > 0 && C % 4 == 0 && C <= 1024, "dcf_op_layerscale_residual: C = %d must be a multiple of 4 up to 1024", C);
  DCF_CHECK(aligned16(R) && aligned16(H) && aligned16(ls) && aligned16(Y), "dcf_op_layerscale_residual: pointers must be 16-byte aligned");
  hipLaunchKernelGGL(k_ls_fwd, dim3(eg_grid((int64_t)rows * (C / 4), 256)), dim3(256), 0, (hipStream_t)stream, R, mR, H, mH, ls, Y, (int64_t)rows, C);
  DCF_HIP(hipGetLastError());
  return 0;
}

int dcf_op_layerscale_residual_bwd(const float* dY, const float* H, const uint8_t* mR, const uint8_t* mH, const float* ls, float* dR, float* dH,
                                   float* dls, int32_t rows, int32_t C, int32_t accumulate, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  DCF_CHECK(dY && rows > 0, "dcf_op_layerscale_residual_bwd: null argument or no rows");
  DCF_CHECK(!dH || ls, "dcf_op_layerscale_residual_bwd: dH needs the scale");
  DCF_CHECK(!dls || H, "dcf_op_layerscale_residual_bwd: dls needs H");
  DCF_CHECK(C > 0 && C % 4 == 0 && C <= 1024, "dcf_op_layerscale_residual_bwd: C = %d must be a multiple of 4 up to 1024", C);
  DCF_CHECK(aligned16(dY) && aligned16(H) && aligned16(ls) && aligned16(dR) && aligned16(dH),
            "dcf_op_layerscale_residual_bwd: pointers must be 16-byte aligned");
  if (!dR && !dH && !dls) return 0;
  LsGradArgs a{};
  a.dY = dY; a.H = H; a.mR = mR; a.mH = mH; a.ls = ls; a.dR = dR; a.dH = dH; a.rows = rows; a.C = C;
  a.rows_per_wave = (rows + 4 * EG_MAX_WG - 1) / (4 * EG_MAX_WG);                    // a fixed function of `rows`
  const int nwg = (rows + 4 * a.rows_per_wave - 1) / (4 * a.rows_per_wave);
  StreamScratch sc(st);
  float* part = nullptr;
  if (dls && sc.take(&part, (size_t)nwg * C)) return -1;
  a.part = part;
  int rc = 0;
  hipLaunchKernelGGL(k_ls_bwd, dim3(nwg, (C + 255) / 256), dim3(256), 0, st, a);
  if (dls) hipLaunchKernelGGL(k_eg_reduce, dim3((C + 255) / 256), dim3(256), 0, st, (const float*)part, nwg, (int64_t)C, C, dls, 1, 1, accumulate);
  EG_LAUNCHED("dcf_op_layerscale_residual_bwd");
  return sc.end(rc);
}

}  // extern "C"
