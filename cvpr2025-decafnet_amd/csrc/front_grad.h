// vid_map of the training step on shared products (front_grad.hip): the arguments of the weight-gradient kernel whose X operand is
// channel-major.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dcf {

constexpr int FG_TILE = 64;             // clips per gate tile: the row tile of the forward's channel-major GEMM (GemmArgs::tile_skip)
constexpr int FG_NQ_CHUNK = 64;         // videos whose query counts one table launch carries by value

// dW[n][c] = sum_b sum_t R[b][t][n] X[b][c][t] for up to two (R, X) pairs (blockIdx.z): the expert half and the shallow half
struct FrontWgradArgs {
  const float* R[2];          // (nvid, T, N) token-major row sums of the upstream gradient
  const void* X[2];           // (nvid, C, T) channel-major features: fp32, or binary16 for the half form of the kernel
  const unsigned* absmax[2];  // device word per pair: bits of max |R|
  const uint8_t* skip[2];     // (nvid, ntiles) or nullptr: tile f of video b holds a clip some query keeps; 0 = no K step
  float* part[2];             // (nslices, N, C) partial sums in the scaled domain
  int nvid, T, N, C;
  int slice_t, slices_per_video, ntiles;     // slice_t is a multiple of FG_TILE
};

// half: X holds binary16 values (any alignment), read as stored: one X plane and two products per k-step instead of two and three
int launch_front_wgrad(const FrontWgradArgs& a, int pairs, hipStream_t st, bool half = false);

// The pieces the selected-clip form of the operators (front_select.hip) shares with front_grad.hip.
// qoff[v] = first row of video v (qoff[nvid] = B'), vtab[q] = video of row q; nq is a host array, read before the call returns
int launch_front_qtables(int nvid, const int32_t* nq, int* qoff, int* vtab, hipStream_t st);
// the column groups of W (E, Cin) as compact matrices W1c / W2c (E, D) and w3c (E); a null destination is not written
int launch_front_unpack_w(const float* W, int Cin, int D, int E, float* W1c, float* W2c, float* w3c, hipStream_t st);
// k_fg_reduce: out[(i / rowlen) pitch + i % rowlen] (+)= extra * inv_scale(absmax) * sum_s part[s stride + i], i < count, the parts in
// the blocked order of grad_common.h; a non-finite value raises bit 0 of *status
int launch_front_reduce(const float* part, int nparts, int64_t stride, int count, int rowlen, int pitch, const unsigned* absmax, float extra,
                        float* out, int accumulate, unsigned* status, hipStream_t st);

}  // namespace dcf
