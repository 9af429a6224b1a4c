// Recall@k at temporal-IoU thresholds on the device (include/decafnet_hip_eval.h): what evaluator.finish_proposals and
// RecallCounter.update do per video on the host -- grid units to seconds, IoU of the kept rows with the ground truth, the best of
// the first k, a comparison per threshold -- for the rows batched NMS left in device memory, added to a table that is read once.
//
// One lane per query.  A query's rows are few (max_num_segs) and its arithmetic is a handful of fp32 operations, each rounded on its
// own as torch's CPU kernels round them: this file is compiled with -ffp-contract=off, the division is __fdiv_rn, and max / min are
// compare-selects with the NaN rule of torch written out.  The hit bits of a lane (<= 8 x 8 cells) sit in one 64-bit word; a cell is
// counted with __ballot and a popcount per wave, the waves' counts meet in LDS, and the workgroup adds each non-zero cell with ONE
// 64-bit integer atomicAdd.  Integer sums are exact in any order, so the table does not depend on the schedule.  No scratch.
#include "../../include/decafnet_hip_eval.h"
#include "common.h"

namespace dcf {

constexpr int REC_NT = 256;
constexpr int REC_WAVES = REC_NT / DCF_WAVE;
constexpr int REC_MAX = 8;                       // ranks and thresholds of one call

__device__ __forceinline__ bool rec_nan(float x) { return x != x; }
__device__ __forceinline__ float rec_qnan() { return __uint_as_float(0x7fc00000u); }
// torch.maximum / torch.minimum: a NaN operand gives NaN
__device__ __forceinline__ float rec_max(float a, float b) { return (rec_nan(a) || rec_nan(b)) ? rec_qnan() : (a > b ? a : b); }
__device__ __forceinline__ float rec_min(float a, float b) { return (rec_nan(a) || rec_nan(b)) ? rec_qnan() : (a < b ? a : b); }
// torch.clamp with scalar bounds: a NaN stays
__device__ __forceinline__ float rec_clamp(float x, float lo, float hi) { return rec_nan(x) ? x : (x < lo ? lo : (x > hi ? hi : x)); }

__device__ __forceinline__ float rec_seconds(float x, const float* m) {
  x = __fmul_rn(x, m[2]);                        // vid_stride
  x = __fmul_rn(x, m[3]);                        // clip_stride
  x = __fadd_rn(x, m[4]);                        // half_clip
  x = __fdiv_rn(x, m[5]);                        // fps
  return rec_clamp(x, 0.f, m[6]);                // duration
}

__global__ __launch_bounds__(REC_NT) void k_recall_update(const float* __restrict__ segs, const int32_t* __restrict__ counts,
                                                          const float* __restrict__ meta, int nq, int M, const int32_t* __restrict__ ranks,
                                                          int n_ranks, const double* __restrict__ threshs, int n_threshs,
                                                          unsigned long long* __restrict__ hits, unsigned long long* __restrict__ n_queries,
                                                          float* __restrict__ best_out) {
  __shared__ int s_rank[REC_MAX];
  __shared__ double s_thr[REC_MAX];
  __shared__ int s_cnt[REC_WAVES][REC_MAX * REC_MAX];
  const int tid = threadIdx.x, lane = tid & (DCF_WAVE - 1), wave = tid / DCF_WAVE;
  if (tid < n_ranks) s_rank[tid] = ranks[tid];
  if (tid < n_threshs) s_thr[tid] = threshs[tid];
  __syncthreads();
  const long long q = (long long)blockIdx.x * REC_NT + tid;
  unsigned long long bits = 0ull;                // cell i * n_threshs + j of this lane's query
  if (q < nq) {
    int count = counts[q];
    count = count < 0 ? 0 : (count > M ? M : count);
    float m[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) m[i] = meta[q * 8 + i];
    const float g0 = m[0], g1 = m[1];
    const bool convert = m[7] != 0.f;
    float best[REC_MAX];
    int kmax = 0;
#pragma unroll
    for (int i = 0; i < REC_MAX; ++i) {
      int k = i < n_ranks ? s_rank[i] : 0;
      k = k < 0 ? 0 : (k > count ? count : k);   // the rows rank i looks at
      best[i] = k == 0 ? 0.f : -INFINITY;
      kmax = k > kmax ? k : kmax;
    }
    const float* row = segs + q * (long long)M * 2;
    for (int r = 0; r < kmax; ++r) {             // kmax <= count <= M: nothing beyond counts[q] is read
      float p0 = row[2 * r], p1 = row[2 * r + 1];
      if (convert) {
        p0 = rec_seconds(p0, m);
        p1 = rec_seconds(p1, m);
      }
      const float lo = rec_max(p0, g0), hi = rec_min(p1, g1);
      const float d = __fsub_rn(hi, lo);
      const float inter = rec_nan(d) ? d : (d > 0.f ? d : 0.f);
      const float total = __fadd_rn(__fsub_rn(p1, p0), __fsub_rn(g1, g0));
      const float v = __fdiv_rn(inter, __fsub_rn(total, inter));
#pragma unroll
      for (int i = 0; i < REC_MAX; ++i)
        if (i < n_ranks && r < s_rank[i]) best[i] = rec_max(best[i], v);
    }
#pragma unroll
    for (int i = 0; i < REC_MAX; ++i) {
      if (i >= n_ranks) break;
      const float b = rec_nan(best[i]) ? rec_qnan() : best[i];
      if (best_out != nullptr) best_out[q * n_ranks + i] = b;
      const double bd = (double)b;
      for (int j = 0; j < n_threshs; ++j)
        if (bd >= s_thr[j]) bits |= 1ull << (i * n_threshs + j);      // false for NaN
    }
  }
  const int cells = n_ranks * n_threshs;
  for (int c = 0; c < cells; ++c) {
    const unsigned long long b = __ballot((int)((bits >> c) & 1ull));
    if (lane == 0) s_cnt[wave][c] = __popcll(b);
  }
  __syncthreads();
  if (tid < cells) {
    int n = 0;
#pragma unroll
    for (int w = 0; w < REC_WAVES; ++w) n += s_cnt[w][tid];
    if (n > 0) atomicAdd(&hits[tid], (unsigned long long)n);
  }
  if (blockIdx.x == 0 && tid == 0) atomicAdd(n_queries, (unsigned long long)nq);
}

}  // namespace dcf

extern "C" {

int dcf_eval_ext_version(void) { return DCF_EVAL_EXT_VERSION; }

int32_t dcf_op_recall_update(const float* segs, const int32_t* counts, const float* meta, int32_t nq, int32_t M, const int32_t* ranks,
                             int32_t n_ranks, const double* threshs, int32_t n_threshs, int64_t* hits, int64_t* n_queries, float* best,
                             void* stream) {
  const char* who = "dcf_op_recall_update";
  DCF_CHECK(segs && counts && meta && ranks && threshs && hits && n_queries, "%s: null %s", who,
            !segs ? "segs" : !counts ? "counts" : !meta ? "meta" : !ranks ? "ranks" : !threshs ? "threshs" : !hits ? "hits" : "n_queries");
  DCF_CHECK(nq >= 0 && M >= 1, "%s: nq %d (>= 0), M %d (>= 1)", who, (int)nq, (int)M);
  DCF_CHECK(n_ranks >= 1 && n_ranks <= dcf::REC_MAX && n_threshs >= 1 && n_threshs <= dcf::REC_MAX, "%s: n_ranks %d, n_threshs %d (1 to %d each)",
            who, (int)n_ranks, (int)n_threshs, dcf::REC_MAX);
  DCF_CHECK(reinterpret_cast<uintptr_t>(hits) % 8 == 0 && reinterpret_cast<uintptr_t>(n_queries) % 8 == 0,
            "%s: hits / n_queries not aligned to 8 bytes", who);
  if (nq == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  // the algorithmic traffic: at most M rows, the count and the meta record per query, best once (the live rows are known on the device only)
  dcf::ProfScope prof("recall_update", st, 0.0, (double)nq * (8.0 * M + 36.0 + (best ? 4.0 * n_ranks : 0.0)));
  const unsigned grid = (unsigned)(((long long)nq + dcf::REC_NT - 1) / dcf::REC_NT);
  hipLaunchKernelGGL(dcf::k_recall_update, dim3(grid), dim3(dcf::REC_NT), 0, st, segs, counts, meta, (int)nq, (int)M, ranks, (int)n_ranks, threshs,
                     (int)n_threshs, reinterpret_cast<unsigned long long*>(hits), reinterpret_cast<unsigned long long*>(n_queries), best);
  DCF_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
