// The selected-clip extension (include/decafnet_hip_select.h): the union of the queries' gates as an ascending clip list
// (dcf_op_select_clips) and the transposing gather that makes clip-major rows of dense channel-major features
// (dcf_op_gather_clip_rows, _h).  The two forwards of the extension live in engine.hip beside the forwards they are a form of.
//
// The device code of both kernels is in select.h, which the several-video forms (select_videos.hip) call too.
#include "../../include/decafnet_hip_select.h"
#include "select.h"

namespace dcf {

__global__ __launch_bounds__(SEL_NT) void k_select_clips(const float* __restrict__ gate, const uint8_t* __restrict__ mask, int T, int nq,
                                                         int* __restrict__ clips, int* __restrict__ pos, int* __restrict__ count) {
  select_clips_body(gate, mask, T, nq, clips, pos, count);
}

template <typename E>
__global__ __launch_bounds__(GAT_NT) void k_gather_clip_rows(const E* __restrict__ X, long long ldx, const int* __restrict__ clips, int n,
                                                             int D, E* __restrict__ rows) {
  gather_clip_rows_tile<E>(X, ldx, clips, n, D, rows, blockIdx.x * GAT_SIDE, blockIdx.y * GAT_SIDE);
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
