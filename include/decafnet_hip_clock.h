/* decafnet_hip_clock.h -- the step-count extension of libdecafnet_hip.so.
 *
 * include/decafnet_hip.h is ABI version 12 and frozen; include/decafnet_hip_train.h, include/decafnet_hip_dist.h,
 * include/decafnet_hip_attn.h, include/decafnet_hip_front.h and include/decafnet_hip_guard.h are extensions of version 1 each and
 * frozen too.  The Adam / AdamW / EMA update whose step counts live on the device is declared here, lives in the same shared object
 * and carries a version of its own, dcf_clock_ext_version().
 *
 * Version 1: dcf_clock_adam_step (csrc/optim_clock.hip).
 *
 * Why.  dcf_optim_adam_step and dcf_guard_adam_step take the bias corrections 1 - b1^t and sqrt(1 - b2^t) by value, in the
 * dcf_optim_group of every (parameter group, step count) pair: the count t is the host's.  The host does not learn whether a guarded
 * update was applied, so its count follows attempted steps; and a launch holds DCF_OPTIM_MAX_GROUPS pairs, so the counts of one step
 * may take few distinct values.  Here the count of every row sits in device memory next to the data it governs: it advances where the
 * update is applied and nowhere else, and every row may have a count of its own.
 *
 * Conventions are those of the dcf_optim_* family (decafnet_hip.h): the dcf_optim_row table and its chunk map, 4-byte-aligned fp32
 * tensors, the dcf_optim_group array by value, everything on `stream`, no host wait, no floating-point atomics, 0 on success and -1
 * with dcf_last_error() otherwise.
 *
 * dcf_clock_adam_step(table, chunk_map, n_tensors, n_chunks, groups, n_groups, bc_tables, bc_len, steps, coef, guard_state, with_ema,
 *                     ema_beta, stream)
 *   steps        n_tensors int64 in DEVICE memory, 8-byte aligned, owned by the caller: steps[r] is the number of updates that were
 *                applied to table row r so far.
 *   groups       a HOST array of n_groups records, read by value during the call, as in dcf_optim_adam_step.  lr, weight_decay, b1,
 *                b2, one_minus_b1, one_minus_b2, eps and mode are used; bc1 and sqrt_bc2 are IGNORED.  row.group is the index of the
 *                parameter group alone (in dcf_optim_adam_step it names a (group, count) pair).
 *   bc_tables    a HOST array of n_groups DEVICE pointers, read by value during the call (they travel with the launch as kernel
 *                arguments, like the groups).  bc_tables[k] addresses bc_len[k] pairs {float bc1, float sqrt_bc2}, 4-byte aligned;
 *                pair t - 1 belongs to the count t.  For a count t > bc_len[k] both corrections are 1.0f (so is, by definition, a
 *                count t < 1, which no caller produces from counts that start at 0).  Several groups may name one table.  A table
 *                with bc_len[k] == 0 may be NULL.  The tables are only read and must stay as they are until the launch has run.
 *   bc_len       a HOST array of n_groups int32, each >= 0.
 *   coef         one float in device memory, or NULL for 1: the clip coefficient, as in dcf_optim_adam_step.
 *   guard_state  a dcf_guard_state in device memory (decafnet_hip_guard.h), or NULL: always apply.
 *
 * One row r, when the launch is applied (guard_state NULL, or its verdict DCF_GUARD_APPLY):
 *  - without DCF_OPTIM_NO_GRAD: the update of dcf_optim_adam_step with t = steps[r] + 1 and the corrections of pair t - 1 of its
 *    group's table -- the same element arithmetic (csrc/optim.h), so a caller that stores in the table the floats it would have passed
 *    by value gets the bits of dcf_optim_adam_step.  Afterwards steps[r] = t, also for a row with n == 0.
 *  - with DCF_OPTIM_NO_GRAD: steps[r], p and both moments keep their bits; its EMA copy moves as in dcf_optim_adam_step.
 * Under verdict DCF_GUARD_SKIP nothing is written: no tensor, no EMA copy, no count.
 *
 * Two kernels on `stream`: the chunk kernel (one workgroup per chunk; it reads steps and writes none), then one thread per row that
 * advances the counts with ordinary stores.  No workgroup reads a count that the same launch writes.  With n_chunks == 0 the second
 * kernel still runs over the n_tensors rows (rows with n == 0 advance).
 *
 * Refused with -1 and a message, before anything is launched: what dcf_optim_adam_step refuses; n_tensors > 0 with a null table or
 * null steps; steps not 8-byte aligned; null bc_tables or null bc_len with n_chunks > 0; a negative bc_len[k]; a null bc_tables[k]
 * with bc_len[k] > 0.
 */
#ifndef DECAFNET_HIP_CLOCK_H
#define DECAFNET_HIP_CLOCK_H

#include <stdint.h>

#include "decafnet_hip.h"
#include "decafnet_hip_guard.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCF_CLOCK_EXT_VERSION 1

int dcf_clock_ext_version(void);

int dcf_clock_adam_step(const dcf_optim_row* table, const int32_t* chunk_map, int32_t n_tensors, int64_t n_chunks,
                        const dcf_optim_group* groups, int32_t n_groups, const float* const* bc_tables, const int32_t* bc_len,
                        int64_t* steps, const float* coef, const dcf_guard_state* guard_state, int32_t with_ema, float ema_beta,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DECAFNET_HIP_CLOCK_H */
