// Backward of what a fusion decoder layer (TransformerDecoder, libs/modeling/blocks.py:594-650) needs besides the operators of
// conv_grad.hip and enc_grad.hip (xattn_grad.hip): the global cross-attention core and the AdaLN modulation with its backward.
// Token-major fp32 rows like the forward.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dcf {

constexpr int XG_SLICE_ROWS = 512;     // query rows of a sequence whose dK / dV one workgroup accumulates: a constant, so the summation
                                       // order depends on (B, T, Lk, C, heads) alone
constexpr int XG_MAX_LK = 64;          // a lane owns a key

struct XAttnGradArgs {
  const float* Q; const float* K; const float* V;    // (B*T, C), (B*Lk, C), (B*Lk, C)
  const uint8_t* kvmask;                              // (B*Lk) or nullptr
  const float* dO;                                    // (B*T, C)
  float* dQ;                                          // (B*T, C) or nullptr
  float* partK; float* partV;                         // (B, S, Lk, C) per-slice sums, or nullptr (the output is not wanted)
  int B, T, Lk, C, heads, S;
};

struct AdaLnArgs {
  const float* X;          // (rows, C)
  const uint8_t* mask;     // (rows) or nullptr
  const float* H;          // (rows, 2C): scale | shift
  const float* dY;         // (rows, C), backward only
  float* Y;                // forward only
  float* dX; float* dH;    // backward, either may be nullptr
  int rows, C, norm;
};

}  // namespace dcf
