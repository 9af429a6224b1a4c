/* decafnet_hip_eval.h -- the evaluation-metric extension of libdecafnet_hip.so.
 *
 * include/decafnet_hip.h is ABI version 12 and frozen.  What a training run needs to judge its EMA model on the validation split
 * without a host read per video is declared here, lives in the same shared object and carries a version of its own,
 * dcf_eval_ext_version().  A caller that counts Recall@k on the host (evaluator.RecallCounter) never includes this file.
 *
 * Version 1: Recall@k at temporal-IoU thresholds of the rows batched NMS keeps, accumulated in device memory (csrc/eval_metric.hip).
 *
 * Conventions: everything on `stream` without a host wait, no scratch, 0 on success and -1 with dcf_last_error() otherwise.  The
 * only atomics are 64-bit INTEGER adds, whose sum is exact in any order: equal inputs give equal tables. */
#ifndef DECAFNET_HIP_EVAL_H
#define DECAFNET_HIP_EVAL_H

#include <stdint.h>

#include "decafnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCF_EVAL_EXT_VERSION 1
int dcf_eval_ext_version(void);

/* Recall@k at IoU thresholds for the nq queries of a video (or of several), added to a table in device memory.
 *
 * All operands are device memory.
 *   segs   (nq, M, 2) fp32, counts (nq) int32: what batched NMS returns, rows in non-increasing score order, row r is rank r + 1.
 *          counts[q] is clamped to [0, M] on the device; nothing of a row >= counts[q] is read.
 *   meta   (nq, 8) fp32 per query: gt_start, gt_end, vid_stride, clip_stride, half_clip, fps, duration, convert.
 *   ranks  (n_ranks) int32, each >= 1 and possibly > M (a rank < 1 looks at no row); threshs (n_threshs) float64.
 *   hits   (n_ranks, n_threshs) int64 and n_queries (1) int64: ACCUMULATED into, never overwritten.
 *   best   (nq, n_ranks) fp32 or NULL: the best IoU among the first k rows, written for every query.
 *
 * Per query, every step one fp32 operation rounded on its own (no fused multiply-add, a true division):
 *   1. where convert != 0, both ends x of every live row become seconds:
 *        x = x * vid_stride;  x = x * clip_stride;  x = x + half_clip;  x = x / fps;  x = min(max(x, 0), duration)  (a NaN stays)
 *   2. lo = max(p0, g0); hi = min(p1, g1); inter = max(hi - lo, 0); v = inter / (((p1 - p0) + (g1 - g0)) - inter), a NaN operand
 *      giving NaN in max / min
 *   3. for each k of ranks: best_k = the maximum of v over the first min(k, count) rows, NaN if one of them is NaN (written as the
 *      quiet NaN 0x7fc00000), 0 if there is none
 *   4. hits[i, j] += ((double)best_k >= threshs[j]), false for NaN; n_queries += nq
 *
 * Two calls on one stream accumulate in stream order; calls on several streams into one table are safe as well (integer atomics).
 *
 * Refused before any launch: a null segs, counts, meta, ranks, threshs, hits or n_queries; nq < 0; M < 1; n_ranks or n_threshs
 * outside [1, 8]; hits or n_queries not aligned to 8 bytes.  nq == 0 returns 0 and launches nothing. */
int32_t dcf_op_recall_update(const float* segs, const int32_t* counts, const float* meta, int32_t nq, int32_t M, const int32_t* ranks,
                             int32_t n_ranks, const double* threshs, int32_t n_threshs, int64_t* hits, int64_t* n_queries, float* best,
                             void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DECAFNET_HIP_EVAL_H */
