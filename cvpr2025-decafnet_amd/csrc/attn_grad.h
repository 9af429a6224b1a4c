// Gradient of the sliding-window attention core (attn_grad.hip): dQ, dK, dV of k_local_attn's O given dO.  Token-major (B*T, C)
// fp32 rows, heads concatenated along C, like the forward.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dcf {

struct LocalAttnGradArgs {
  const float* Q; const float* K; const float* V;   // [B*T][C] the forward's operands
  const uint8_t* mask;                               // [B*T] or nullptr = every row valid
  const float* dO;                                   // [B*T][C]
  float* dQ; float* dK; float* dV;                   // [B*T][C], each may be nullptr
  float* stats;                                      // [B*T][heads][4]: row maximum m, 1 / sum exp(s - m), delta, unused; nullptr when
                                                     // neither dK nor dV is wanted
  int B, T, C, heads, window;                        // window odd, >= 1
};

// floats of the row statistics the key-side gather reads (library-owned scratch, allocated and freed on the caller's stream)
inline size_t local_attn_grad_stats_floats(int64_t rows, int heads) { return (size_t)rows * heads * 4; }

int launch_local_attn_bwd(const LocalAttnGradArgs& a, hipStream_t st);

// the geometry check of the sliding-window gradient kernels, which the launchers with dropout on the map share (attn_drop.hip);
// `window0`: what the message says of window = 0.  0, or -1 with the error set.
int local_attn_geometry_check(const char* who, int B, int T, int C, int heads, int window, const char* window0);

}  // namespace dcf
