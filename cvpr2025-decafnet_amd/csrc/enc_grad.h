// Forward / backward pairs of the operators a TransformerEncoder block needs besides MaskedConv1D, the channel LayerNorm and the
// sliding-window attention (enc_grad.hip): the depthwise k3 convolutions, masked_max_pool1d, the exact GELU and the LayerScale
// residual.  Token-major (B*T, C) fp32 rows like the forward.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace dcf {

constexpr int EG_MAX_WG = 512;         // workgroups (of four waves) of a column reduction: rows per wave = ceil(rows / (4 * EG_MAX_WG)), as k_ln_bwd
constexpr int EG_MIN_SLICES = 64;      // row slices per sequence of the pooling's column minimum (at least 256 rows each)

struct DwGradArgs {
  const float* X;          // (B*T, C) forward input
  const uint8_t* mask;     // (B*T) or nullptr
  const float* dY;         // (n, B*To, C)
  float* part;             // (nwg, n, 3, C) per-workgroup sums
  int B, T, To, C, stride, rows_per_wave;
};

struct LsGradArgs {
  const float* dY; const float* H; const uint8_t* mR; const uint8_t* mH; const float* ls;
  float* dR; float* dH;
  float* part;             // (nwg, C) per-workgroup sums of dY * H * m_H, or nullptr
  int rows, C, rows_per_wave;
};

// k_eg_reduce on `st` for the column reductions of other files (drop_grad.hip): out[o(i)] (+)= sum_s part[s * stride + i], i < count
void launch_eg_reduce(const float* part, int nparts, int64_t stride, int count, float* out, int KT, int C, int accumulate, hipStream_t st);

// the exact GELU and its slope (accuracy: enc_grad.hip); shared so that a fused pass has the bits of dcf_op_gelu / dcf_op_gelu_bwd
__device__ __forceinline__ void gelu_terms(float x, float& Phi, float& xphi) {
  const float p = 0.5f * erfcf(fabsf(x) * 0.70710678118654752440f);      // Phi(-|x|) in (0, 0.5]
  Phi = x < 0.f ? p : 1.0f - p;
  const float t = x * x, res = __builtin_fmaf(x, x, -t);                 // x^2 = t + res exactly
  const float e = expf(-0.5f * t);
  xphi = x * (0.39894228040143267794f * __builtin_fmaf(e, -0.5f * res, e));
}
__device__ __forceinline__ float gelu_exact(float x) {
  float Phi, xphi;
  gelu_terms(x, Phi, xphi);
  return x * Phi;
}
__device__ __forceinline__ float gelu_slope(float x) {
  float Phi, xphi;
  gelu_terms(x, Phi, xphi);
  return Phi + xphi;
}

}  // namespace dcf
