// The selected-clip extension (include/decafnet_hip_select.h): the union of the queries' gates as an ascending clip list
// (dcf_op_select_clips) and the transposing gather that makes clip-major rows of dense channel-major features
// (dcf_op_gather_clip_rows, _h).  The two forwards of the extension live in engine.hip beside the forwards they are a form of.
//
// k_select_clips is a stream compaction by ONE workgroup of 16 waves.  A strip is 4 sub-strips of 1024 clips, thread i takes clip
// i of each: its gate loads are coalesced, and a sub-strip's order is the lane order, so a wave's ballot and a popcount below the
// lane give the rank inside the wave.  The 4 x 16 wave counts go through LDS (double buffered: one barrier per strip), every thread
// adds up the ones in front of its own, and the count of all strips before rides in a register.  The flags of the next strip are
// loaded before the scan of the current one.  No atomics: the list is ascending by construction.
#include "../../include/decafnet_hip_select.h"
#include "common.h"

namespace dcf {

constexpr int SEL_NT = 1024, SEL_WAVES = SEL_NT / DCF_WAVE, SEL_SUB = 4;
constexpr int SEL_STRIP = SEL_NT * SEL_SUB;

__global__ __launch_bounds__(SEL_NT) void k_select_clips(const float* __restrict__ gate, const uint8_t* __restrict__ mask, int T, int nq,
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

// rows[i][d] = X[d * ldx + clips[i]]: a 64 x 64 tile through LDS.  Load phase: lane = clip of the tile, the waves walk the channels
// (a wave reads 64 entries of one channel row: contiguous wherever the clip list is); the image is [channel][clip] at a pitch of 65
// elements.  Store phase: lane = channel, the waves walk the clips (a wave writes 64 contiguous elements of one output row and reads
// LDS at a stride of 65: conflict free for fp32).
constexpr int GAT_NT = 256, GAT_WAVES = GAT_NT / DCF_WAVE, GAT_SIDE = DCF_WAVE;
template <typename E>
__global__ __launch_bounds__(GAT_NT) void k_gather_clip_rows(const E* __restrict__ X, long long ldx, const int* __restrict__ clips, int n,
                                                             int D, E* __restrict__ rows) {
  __shared__ E tile[GAT_SIDE * (GAT_SIDE + 1)];
  const int lane = threadIdx.x & (DCF_WAVE - 1), wave = threadIdx.x / DCF_WAVE;
  const int i0 = blockIdx.x * GAT_SIDE, d0 = blockIdx.y * GAT_SIDE;
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

template <typename E>
static int launch_gather(const char* who, const void* X, long long ldx, const int32_t* clips, int n, int D, void* rows, hipStream_t st) {
  DCF_CHECK(X && clips && rows, "%s: null %s", who, !X ? "X_cm" : (!clips ? "clips" : "rows"));
  DCF_CHECK(n >= 1 && D >= 1 && ldx >= 1, "%s: n %d, D %d, ldx %lld (all >= 1)", who, n, D, ldx);
  DCF_CHECK(reinterpret_cast<uintptr_t>(X) % sizeof(E) == 0 && reinterpret_cast<uintptr_t>(rows) % sizeof(E) == 0 &&
                reinterpret_cast<uintptr_t>(clips) % 4 == 0,
            "%s: X_cm / rows not aligned to their %d-byte elements, or clips not to 4 bytes", who, (int)sizeof(E));
  const long long gy = ((long long)D + GAT_SIDE - 1) / GAT_SIDE;
  DCF_CHECK(gy <= 65535, "%s: D %d exceeds one grid", who, D);
  ProfScope prof("gather_clip_rows", st, 0.0, 2.0 * sizeof(E) * (double)n * D + 4.0 * n);
  hipLaunchKernelGGL(k_gather_clip_rows<E>, dim3((unsigned)((n + GAT_SIDE - 1) / GAT_SIDE), (unsigned)gy), dim3(GAT_NT), 0, st,
                     static_cast<const E*>(X), ldx, clips, n, D, static_cast<E*>(rows));
  DCF_HIP(hipGetLastError());
  return 0;
}

}  // namespace dcf

extern "C" {

int dcf_op_select_clips(const float* gate, const uint8_t* vid_mask, int32_t T, int32_t nq, int32_t* clips, int32_t* pos, int32_t* count,
                        void* stream) {
  const char* who = "dcf_op_select_clips";
  DCF_CHECK(gate && vid_mask && clips && pos && count, "%s: null argument", who);
  DCF_CHECK(T >= 1 && nq >= 1, "%s: T %d, nq %d (both >= 1)", who, (int)T, (int)nq);
  DCF_CHECK((reinterpret_cast<uintptr_t>(gate) | reinterpret_cast<uintptr_t>(clips) | reinterpret_cast<uintptr_t>(pos) |
             reinterpret_cast<uintptr_t>(count)) % 4 == 0, "%s: gate / clips / pos / count not aligned to 4 bytes", who);
  hipStream_t st = (hipStream_t)stream;
  dcf::ProfScope prof("select_clips", st, 0.0, (4.0 * nq + 1.0 + 8.0) * (double)T);
  hipLaunchKernelGGL(dcf::k_select_clips, dim3(1), dim3(dcf::SEL_NT), 0, st, gate, vid_mask, (int)T, (int)nq, clips, pos, count);
  DCF_HIP(hipGetLastError());
  return 0;
}

int dcf_op_gather_clip_rows(const float* X_cm, int64_t ldx, const int32_t* clips, int32_t n, int32_t D, float* rows, void* stream) {
  return dcf::launch_gather<uint32_t>("dcf_op_gather_clip_rows", X_cm, (long long)ldx, clips, n, D, rows, (hipStream_t)stream);
}

int dcf_op_gather_clip_rows_h(const uint16_t* X_cm, int64_t ldx, const int32_t* clips, int32_t n, int32_t D, uint16_t* rows, void* stream) {
  return dcf::launch_gather<uint16_t>("dcf_op_gather_clip_rows_h", X_cm, (long long)ldx, clips, n, D, rows, (hipStream_t)stream);
}

}  // extern "C"
