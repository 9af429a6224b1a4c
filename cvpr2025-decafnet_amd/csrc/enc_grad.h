// Forward / backward pairs of the operators a TransformerEncoder block needs besides MaskedConv1D, the channel LayerNorm and the
// sliding-window attention (enc_grad.hip): the depthwise k3 convolutions, masked_max_pool1d, the exact GELU and the LayerScale
// residual.  Token-major (B*T, C) fp32 rows like the forward.
#pragma once
#include <hip/hip_runtime.h>
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

}  // namespace dcf
