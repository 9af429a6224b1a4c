// Dropout on the attention map (nn.Dropout(attn_pdrop) on the softmax map, blocks.py:368 / :388) inside the attention cores, forward
// and backward, and channel dropout (nn.Dropout1d, model.py:614): attn_drop.hip.  The stream contract is dropout.h's; the element
// index of a map element is its flat index in the reference's (bs, H, T, W) resp. (bs, H, T, Lk) tensor
// (include/decafnet_hip_attn_drop.h).  This header is the sliding-window form's; the global and cross forms (DenseAttnDropArgs) are
// local to attn_drop.hip and reached through its exports.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dcf {

struct LocalAttnDropArgs {
  const float* Q; const float* K; const float* V;   // [B*T][C]
  const uint8_t* mask;                               // [B*T]; the backward takes nullptr = every row valid
  float* O;                                          // forward: [B*T][C]
  const float* dO;                                   // backward: [B*T][C]
  float* dQ; float* dK; float* dV;                   // backward: [B*T][C], each may be nullptr
  float* stats;                                      // backward: [B*T][heads][4]: m, 1 / l, delta, the row's keep bits (window <= 32)
  int B, T, C, heads, window;                        // window odd, >= 1
  int b0;                                            // the first sequence is sequence b0 of the reference's batch
  uint64_t seed;
  uint32_t site;
  float p, scale;                                    // scale = 1 / (1 - p), fp32, computed on the host
};

int launch_local_attn_drop(const LocalAttnDropArgs& a, hipStream_t st);
int launch_local_attn_drop_bwd(const LocalAttnDropArgs& a, hipStream_t st);

}  // namespace dcf
