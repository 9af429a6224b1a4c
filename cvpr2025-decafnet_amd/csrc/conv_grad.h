// Gradients of the two operators every differentiable block of the network is built from: MaskedConv1D (k = 1 / 3, dense) and the
// channel LayerNorm (conv_grad.hip).  Token-major (B*T, C) fp32 rows like the forward.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dcf {

// dY enters the fp16 planes of the matrix-core kernels multiplied by 2^(CG_TARGET_EXP - floor(log2 max|dY|)): its largest element
// lands in [2^14, 2^15) whatever the loss normaliser made of it, every element within 2^-18 of the largest keeps all 22 bits of
// the two planes, and the absolute representation error below that is 2^-40 of the largest element.
constexpr int CG_TARGET_EXP = 14;
constexpr int CG_MAX_SLICES = 64;       // row slices of the matrix-core weight gradient (fp32 partials per slice, summed in order)
constexpr int CG_SMALL_SLICE = 256;     // rows per slice of the vector-ALU weight gradient (N = 1, 2)

struct ConvGradArgs {
  const float* X;          // (rows, Cin) forward input (weight gradient)
  const float* dY;         // (rows, N)
  const uint8_t* flags;    // (rows) bit0 = row valid (mask), bit1 = a left neighbour exists in the sequence, bit2 = a right one
  const unsigned* absmax;  // device word: bits of max |dY|
  float* part;             // (nslices, N, k, Cin) partial sums in the scaled domain
  float* dbpart;           // (nslices, N) or nullptr
  int rows, Cin, N, k, slice_rows, nslices;
};

struct LnBwdArgs {
  const float* X; const float* w; const float* b; const float* dOut;
  float* dX;
  float* part;             // (nwg, 2, C): per-workgroup sums of (dy * xhat, dy), or nullptr when neither is wanted
  int rows, C, relu, rows_per_wave;
};

// power-of-two operand scale of dY from the bits of max |dY|; inv = its exact inverse.  An all-zero or non-finite dY takes 1 (the
// latter surfaces as a non-finite sum).
__device__ __forceinline__ float cg_scale(unsigned bits, float& inv) {
  const int e = (int)((bits >> 23) & 0xffu);
  if (bits == 0u || e == 255) { inv = 1.f; return 1.f; }
  int sf = 254 + CG_TARGET_EXP - e;              // biased exponent of 2^(CG_TARGET_EXP - (e - 127))
  sf = sf < 1 ? 1 : (sf > 253 ? 253 : sf);
  inv = __uint_as_float((unsigned)(254 - sf) << 23);
  return __uint_as_float((unsigned)sf << 23);
}

// The sticky numerics word of the conv-gradient exports (conv_grad.hip): cg_begin fails with the message if an earlier call of the
// process raised it and hands out the device word otherwise; cg_end queues its copy to the host mirror.  front_grad.hip shares it.
int cg_begin(const char* what, hipStream_t st, unsigned** word);
int cg_end(hipStream_t st);
// The word under a step guard (include/decafnet_hip_guard.h, optim_guard.hip).  While a guard is armed cg_begin never fails for the
// word and cg_end leaves the host mirror alone; cg_guard_word hands the device word to the guarded norm of the armed state (nullptr
// for any other state or when disarmed), whose final pass reads and clears it.  cg_guard_disarm queues the mirror copy on `st`.
int cg_guard_arm(const void* state);
int cg_guard_disarm(hipStream_t st);
unsigned* cg_guard_word(const void* state);

int launch_absmax(const float* x, int64_t n, unsigned* word, hipStream_t st);
int launch_wgrad(const ConvGradArgs& a, hipStream_t st);
int launch_ln_bwd(const LnBwdArgs& a, int nwg, hipStream_t st);

}  // namespace dcf
