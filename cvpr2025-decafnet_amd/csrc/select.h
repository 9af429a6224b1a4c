// The device code the one-video and the several-video operators of selected-clip inference share (select.hip, select_videos.hip):
// the compaction of a video's gates into a clip list, and one tile of the transposing gather.
//
// select_clips_body is a stream compaction by ONE workgroup of 16 waves.  A strip is 4 sub-strips of 1024 clips, thread i takes clip
// i of each: its gate loads are coalesced, and a sub-strip's order is the lane order, so a wave's ballot and a popcount below the
// lane give the rank inside the wave.  The 4 x 16 wave counts go through LDS (double buffered: one barrier per strip), every thread
// adds up the ones in front of its own, and the count of all strips before rides in a register.  The flags of the next strip are
// loaded before the scan of the current one.  No atomics: the list is ascending by construction.
#pragma once
#include "common.h"

namespace dcf {

constexpr int SEL_NT = 1024, SEL_WAVES = SEL_NT / DCF_WAVE, SEL_SUB = 4;
constexpr int SEL_STRIP = SEL_NT * SEL_SUB;

// gate (nq, T), mask (T), clips / pos (T), count (1): of ONE video; the whole workgroup of SEL_NT threads calls it
__device__ __forceinline__ void select_clips_body(const float* __restrict__ gate, const uint8_t* __restrict__ mask, int T, int nq,
                                                  int* __restrict__ clips, int* __restrict__ pos, int* __restrict__ count) {
  __shared__ int tot[2][SEL_SUB * SEL_WAVES];
  const int tid = threadIdx.x, lane = tid & (DCF_WAVE - 1), wave = tid / DCF_WAVE;
  // bit j: clip t0 + j * SEL_NT + tid is needed
  auto flags = [&](long long t0) -> unsigned {
    unsigned f = 0;
#pragma unroll
    for (int j = 0; j < SEL_SUB; ++j) {
      const long long t = t0 + j * SEL_NT + tid;
      if (t < T) {
        // the mask byte and every query's gate are loaded side by side: no load waits for the value of another
        unsigned any = 0;
        for (int q = 0; q < nq; ++q) any |= gate[(long long)q * T + t] != 0.f ? 1u : 0u;
        f |= (mask[t] ? any : 0u) << j;
      }
    }
    return f;
  };
  int carry = 0;
  unsigned cur = flags(0);
  int s = 0;
  for (long long t0 = 0; t0 < T; t0 += SEL_STRIP, ++s) {
    const unsigned nxt = t0 + SEL_STRIP < T ? flags(t0 + SEL_STRIP) : 0u;
    int* tt = tot[s & 1];
    unsigned long long bal[SEL_SUB];
#pragma unroll
    for (int j = 0; j < SEL_SUB; ++j) {
      bal[j] = __ballot((cur >> j) & 1u);
      if (lane == 0) tt[j * SEL_WAVES + wave] = __popcll(bal[j]);
    }
    __syncthreads();
    int run = carry, base[SEL_SUB] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < SEL_SUB * SEL_WAVES; ++i) {
      if ((i % SEL_WAVES) == wave) base[i / SEL_WAVES] = run;
      run += tt[i];
    }
    carry = run;
#pragma unroll
    for (int j = 0; j < SEL_SUB; ++j) {
      const long long t = t0 + j * SEL_NT + tid;
      if (t < T) {
        const bool need = (cur >> j) & 1u;
        const int k = base[j] + __popcll(bal[j] & ((1ull << lane) - 1ull));
        pos[t] = need ? k : -1;
        if (need) clips[k] = (int)t;
      }
    }
    cur = nxt;
  }
  if (tid == 0) *count = carry;
}

// rows[i][d] = X[d * ldx + clips[i]]: a 64 x 64 tile through LDS, clips i0 .. i0 + 63 of the list and channels d0 .. d0 + 63.  Load
// phase: lane = clip of the tile, the waves walk the channels (a wave reads 64 entries of one channel row: contiguous wherever the
// clip list is); the image is [channel][clip] at a pitch of 65 elements.  Store phase: lane = channel, the waves walk the clips (a
// wave writes 64 contiguous elements of one output row and reads LDS at a stride of 65: conflict free for fp32).
constexpr int GAT_NT = 256, GAT_WAVES = GAT_NT / DCF_WAVE, GAT_SIDE = DCF_WAVE;
template <typename E>
__device__ __forceinline__ void gather_clip_rows_tile(const E* __restrict__ X, long long ldx, const int* __restrict__ clips, int n, int D,
                                                      E* __restrict__ rows, int i0, int d0) {
  __shared__ E tile[GAT_SIDE * (GAT_SIDE + 1)];
  const int lane = threadIdx.x & (DCF_WAVE - 1), wave = threadIdx.x / DCF_WAVE;
  {
    const int i = i0 + lane;
    long long c = i < n ? clips[i] : 0;
    c = c < 0 ? 0 : (c >= ldx ? ldx - 1 : c);      // no read outside the matrix, whatever the list holds
#pragma unroll 4
    for (int r = wave; r < GAT_SIDE; r += GAT_WAVES) {
      const int d = d0 + r;
      if (i < n && d < D) tile[r * (GAT_SIDE + 1) + lane] = X[(long long)d * ldx + c];
    }
  }
  __syncthreads();
  const int d = d0 + lane;
  if (d >= D) return;
#pragma unroll 4
  for (int r = wave; r < GAT_SIDE; r += GAT_WAVES) {
    const int i = i0 + r;
    if (i >= n) break;
    rows[(long long)i * D + d] = tile[lane * (GAT_SIDE + 1) + r];
  }
}

}  // namespace dcf
