// Gradient of the global self-attention core (global_attn_grad.hip): dQ, dK, dV of k_global_attn's O given dO.  Token-major (B*T, C)
// fp32 rows, heads concatenated along C, like the forward.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dcf {

struct GlobalAttnGradArgs {
  const float* Q; const float* K; const float* V;   // [B*T][C] the forward's operands
  const uint8_t* mask;                               // [B*T] or nullptr = every row valid; it masks KEYS only
  const float* dO;                                   // [B*T][C]
  float* dQ; float* dK; float* dV;                   // [B*T][C], each may be nullptr
  float* stats;                                      // [B*T][heads][4]: row maximum m, 1 / sum exp(s - m), delta, unused; nullptr when
                                                     // neither dK nor dV is wanted
  int B, T, C, heads;
};

// floats of the row statistics the key-side kernel reads (library-owned scratch, allocated and freed on the caller's stream)
inline size_t global_attn_grad_stats_floats(int64_t rows, int heads) { return (size_t)rows * heads * 4; }

int launch_global_attn_bwd(const GlobalAttnGradArgs& a, hipStream_t st);

}  // namespace dcf
