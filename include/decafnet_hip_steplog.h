/* decafnet_hip_steplog.h -- the training-log extension of libdecafnet_hip.so.
 *
 * include/decafnet_hip.h is ABI version 12 and frozen.  The meters of the Trainer's log (worker_v2.py:326-335, AverageMeter of
 * libs/train_utils.py) are kept in device memory: the step adds its loss scalars with one launch and never reads them back; once per
 * log interval one launch turns the tables into the row of numbers a log line needs and empties them.  The two exports are declared
 * here, live in the same shared object and carry a version of their own, dcf_steplog_ext_version().
 *
 * Version 1 (csrc/steplog.hip):
 *   dcf_op_steplog_add      K fp32 scalars, each in an allocation of its own, added to a table of K meters
 *   dcf_op_steplog_flush    the table read out into (K + 1, 6) doubles and reset, in one launch
 *
 * Conventions: everything on `stream` without a host wait, no scratch, 0 on success and -1 with dcf_last_error() otherwise.  No
 * floating-point atomics anywhere: equal inputs give equal bits.  Every refusal comes before any launch.
 *
 * The tables.  `stats` is (K, 6) float64 and `counts` is (K + 1) int64, both device memory, both all zero when empty (the caller
 * allocates them so; a flush leaves them so).  Row k of `stats` is
 *     [0] sum          AverageMeter.sum: every value added, a NaN or inf included
 *     [1] finite_sum   the finite values only
 *     [2] min          the smallest finite value  (meaningful when counts[k] > 0)
 *     [3] max          the largest finite value   (meaningful when counts[k] > 0)
 *     [4] last         the value added last, AverageMeter.val
 *     [5] reserved     neither export reads or writes it
 * counts[k] is the number of finite values of key k, counts[K] the number of adds: the steps.
 * Every NaN the exports store is the quiet NaN 0x7ff8000000000000, whatever the sign and payload of the NaN that came in or that
 * inf + -inf made: IEEE 754 leaves those to the implementation, and the tables are meant to compare equal across them.
 *
 * One table belongs to one stream: adds and flushes on one stream happen in stream order, so `sum` is the value of Python's
 * `sum += float(v)` over the same values, bit for bit.  Calls on several streams into one table are NOT supported: the updates are
 * plain loads and stores, and nothing orders them across streams. */
#ifndef DECAFNET_HIP_STEPLOG_H
#define DECAFNET_HIP_STEPLOG_H

#include <stdint.h>

#include "decafnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCF_STEPLOG_EXT_VERSION 1
int dcf_steplog_ext_version(void);

#define DCF_STEPLOG_MAX_KEYS 16
#define DCF_STEPLOG_COLS 6

/* One step's values into the table.
 *   vals    a HOST array of K device pointers, read at call time (the array may be reused as soon as the call returns).  Each points
 *           to one fp32 scalar, 4-byte aligned: the loss tensors of a step live in K separate allocations, and this is the one launch
 *           that gathers them.
 *   stats   (K, 6) float64, counts (K + 1) int64: accumulated into.
 * One launch of one workgroup, one lane per key.  Lane k widens v = *vals[k] to double (exact) and does
 *     sum = sum + v;  last = v                                  (a NaN is stored as the quiet NaN above)
 *     if v is finite:  finite_sum = finite_sum + v
 *                      min = v if counts[k] == 0 or v < min;  max = v if counts[k] == 0 or v > max
 *                      counts[k] = counts[k] + 1
 * The first value seen wins a tie, so -0.0 and 0.0 are ordered by arrival.  One more lane does counts[K] = counts[K] + 1.
 *
 * Refused before any launch: K outside [1, 16]; a null vals, stats or counts; a null entry of vals; an entry of vals not aligned to
 * 4 bytes; stats or counts not aligned to 8 bytes. */
int dcf_op_steplog_add(const float* const* vals, int32_t K, double* stats, int64_t* counts, void* stream);

/* The table read out and reset, in one launch: a flush is read-and-reset in stream order.
 *   out     (K + 1, 6) float64 in device memory; every element of it is written.
 * With steps = counts[K] and n = counts[k], row k < K of `out` is
 *     [0] mean         sum / (double)steps, one IEEE double division; 0.0 when steps == 0 (AverageMeter.reset's value)
 *     [1] finite_mean  finite_sum / (double)n; NaN (0x7ff8000000000000) when n == 0
 *     [2] min          NaN when n == 0
 *     [3] max          NaN when n == 0
 *     [4] last
 *     [5] (double)n
 * and row K is (double)steps followed by five zeros.  Then columns 0 to 4 of every row of `stats` and all of `counts` are set to
 * zero, the empty state.
 *
 * Refused before any launch: K outside [1, 16]; a null stats, counts or out; stats, counts or out not aligned to 8 bytes. */
int dcf_op_steplog_flush(double* stats, int64_t* counts, int32_t K, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DECAFNET_HIP_STEPLOG_H */
