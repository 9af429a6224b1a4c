/* decafnet_hip_fit.h -- the multi-rank-fit extension of libdecafnet_hip.so.
 *
 * include/decafnet_hip.h is ABI version 12 and frozen; include/decafnet_hip_guard.h is an extension of version 1 and frozen too.  The two
 * small device-side pieces a training run on several ranks needs around its evaluation and its guarded step are declared here, live
 * in the same shared object and carry a version of their own, dcf_fit_ext_version().
 *
 * Version 1 (csrc/fit.hip):
 *   dcf_op_loss_table_mean                             the validation loss of Evaluator.run from a table of per-query rows
 *   dcf_guard_word_publish, dcf_guard_word_merge       the conv-gradient word of the step guard made known to the other ranks
 *
 * Conventions: everything on `stream` without a host wait, 0 on success and -1 with dcf_last_error() otherwise.  No floating-point
 * atomics anywhere: equal inputs give equal bits. */
#ifndef DECAFNET_HIP_FIT_H
#define DECAFNET_HIP_FIT_H

#include <stdint.h>

#include "decafnet_hip.h"
#include "decafnet_hip_guard.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCF_FIT_EXT_VERSION 1
int dcf_fit_ext_version(void);

/* The validation loss (Evaluator._calc_loss per video, then the mean over the videos, worker_v2.py:1029-1061, 903) of a table of
 * per-query rows as dcf_point_objective writes them.
 *
 * All operands are device memory.
 *   rows       (N, 4) fp32 per query: focal1, focal2, iou, n_pos (focal1 is not read).
 *   offsets    (V + 1) int64, non-decreasing, offsets[0] >= 0: video v owns the rows offsets[v] <= q < offsets[v + 1].  The caller
 *              vouches for them: they are read on the device and nothing checks them against N.
 *   per_video  (V, 2) float64 or NULL: the per-video (cls_loss, reg_loss).  NULL: library scratch takes its place.
 *   out2       (2) float64: (cls_loss, reg_loss).
 *
 * Per query, in fp32, every step one operation rounded on its own (a true division, no fused multiply-add):
 *     norm = n_pos < 1 ? 1 : n_pos  (a NaN stays);  cls = focal2 / norm;  reg = iou / norm
 * and both are widened to double, which is exact.
 * Per video and key (easy_reduce(stats, 'mean', skip_nan=True)): s = +0; for q ascending: if the value is not NaN, s = s + value and
 *     n = n + 1; the result is s / n, and NaN (0x7ff8000000000000) where n == 0 -- a video without a query or with NaN values only.
 *     An inf is a value like any other.
 * Over the videos (easy_reduce(loss_list, 'mean'), NaN propagating), an order that depends on V alone:
 *     lane t of 256: a_t = +0; for v = t, t + 256, t + 512, ... < V ascending: a_t = a_t + per_video[v]
 *     then for h = 128, 64, 32, 16, 8, 4, 2, 1 in turn: a_t = a_t + a_(t + h) for every t < h
 *     out = a_0 / V
 * One lane per video in the first launch, one workgroup in the second.
 *
 * Refused before any launch: a null rows, offsets or out2; V < 1; rows not aligned to 4 bytes; offsets, per_video or out2 not
 * aligned to 8 bytes. */
int dcf_op_loss_table_mean(const float* rows, const int64_t* offsets, int32_t V, double* per_video, double* out2, void* stream);

/* The conv-gradient word of the ARMED guard (dcf_guard_arm, decafnet_hip_guard.h) is local to its process.  Under data parallelism a
 * word raised on one rank whose non-finite sum a later mask multiplies away makes that rank alone skip.  The pair below lets the
 * step's existing loss-norm all-reduce carry the word: publish before it, merge after it.
 *
 * The conv-gradient operators raise bit 0 of the word and no other.  DCF_GUARD_REMOTE is the bit that says "some rank raised its
 * word"; after a merge the guarded norm skips and dcf_guard_state.conv_flag records the bit like any other of the word.
 *
 * dcf_guard_word_publish: *slot = 1.0f if the word is non-zero, else 0.0f.  The word keeps its value.
 * dcf_guard_word_merge:   if !(*slot == 0) -- any non-zero sum over the ranks, a NaN included -- the word gets DCF_GUARD_REMOTE ORed
 *                         into it; otherwise nothing is written.
 * Each is one thread of plain C++ on `stream`.  `slot` is one fp32 in device memory, 4-byte aligned.
 *
 * Refused before any launch: a null state or slot; a slot not aligned to 4 bytes; a state that is not the armed one (the word belongs
 * to the armed guard alone). */
#define DCF_GUARD_REMOTE 0x100
int dcf_guard_word_publish(const dcf_guard_state* state, float* slot, void* stream);
int dcf_guard_word_merge(const dcf_guard_state* state, const float* slot, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DECAFNET_HIP_FIT_H */
