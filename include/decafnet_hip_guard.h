/* decafnet_hip_guard.h -- the step-guard extension of libdecafnet_hip.so.
 *
 * include/decafnet_hip.h is ABI version 12 and frozen; include/decafnet_hip_train.h, include/decafnet_hip_dist.h,
 * include/decafnet_hip_attn.h and include/decafnet_hip_front.h are extensions of version 1 each and frozen too.  The guarded
 * training update -- the gradient norm that also decides, on the device, whether the step may be applied, and the Adam / AdamW / EMA
 * update that obeys the decision -- is declared here, lives in the same shared object and carries a version of its own,
 * dcf_guard_ext_version().
 *
 * Version 1: dcf_guard_grad_norm, dcf_guard_adam_step, dcf_guard_arm, dcf_guard_disarm (csrc/optim_guard.hip).
 *
 * Why.  dcf_optim_grad_norm turns one NaN gradient into a NaN coefficient, and dcf_optim_adam_step then writes it into every
 * parameter, both moments and the EMA copy in one launch; no host read happens in a training step that could notice.  The pair below
 * makes the decision where the norm is made and needs no host read either.
 *
 * Conventions are those of the dcf_optim_* family (decafnet_hip.h): the dcf_optim_row table and its chunk map, 4-byte-aligned fp32
 * tensors, the dcf_optim_group array by value, everything on `stream`, no host wait, no floating-point atomics, 0 on success and -1
 * with dcf_last_error() otherwise.
 *
 * dcf_guard_state: a 48-byte device record, 8-byte aligned, owned by the caller.  The caller initialises it (all zero except
 * first_bad_row = last_skipped_attempt = -1) and may read it whenever it is willing to wait for the stream.  It is written by thread 0
 * of the one-workgroup final pass of dcf_guard_grad_norm alone, with ordinary stores.
 *   verdict               of the LAST dcf_guard_grad_norm: 0 = apply, 1 = skip
 *   applied, skipped      running counts of the two verdicts; applied + skipped numbers the attempts from 0
 *   last_skipped_attempt  the number of the last attempt that was skipped (applied + skipped before that call counted itself), or -1
 *   first_bad_row         of the last skipped attempt: the lowest table row with a non-finite chunk partial, or -1 (none; the
 *                         conv-gradient word alone caused the skip).  The row index is that of the NORM's table.
 *   n_bad_rows            of the last skipped attempt: how many rows had one
 *   conv_flag             of the last skipped attempt: the conv-gradient word it found (see dcf_guard_arm), 0 = clear
 * The last four keep their values through applied attempts, so that a log written now and then still names the last offender.
 *
 * dcf_guard_grad_norm: dcf_optim_grad_norm plus the verdict.
 *  - The same lane, wave and chunk sums in the same fixed order: with finite gradients *norm_out and *coef_out have the bits of the
 *    unguarded export.
 *  - A row is bad if one of its chunk partials (the fp64 value of a chunk's fp32 lane sums of squares) is not finite.  That is the
 *    case for a NaN, for +-inf, AND for finite elements whose squares overflow fp32 (|g| >= 1.85e19, or less where the sixteen
 *    squares one lane adds up pass 3.4e38): such a gradient has an infinite norm in fp32 and is refused like an infinite one.
 *  - A row with DCF_OPTIM_NO_GRAD or g == NULL is never read and is never bad.
 *  - verdict = skip if any row is bad or if the conv-gradient word of the armed guard is set.  On skip *coef_out is +0 and *norm_out
 *    keeps the norm as computed (non-finite if a row was bad).  Either output may be NULL.
 *  - The counters advance here and nowhere else: calling the norm alone is well defined, one attempt per call.
 *
 * dcf_guard_adam_step: dcf_optim_adam_step under the verdict in `state`.
 *  - verdict == 0: the arithmetic of dcf_optim_adam_step on the same operands; p, exp_avg, exp_avg_sq and ema get the same bits.
 *  - verdict == 1: every workgroup reads the verdict and returns.  No byte of any row is written; the EMA copy does not move either.
 *  - The verdict is one word read through the scalar cache: uniform over the grid, so the branch is wave-uniform.  The cost is the
 *    unguarded update plus that load.
 *
 * dcf_guard_arm(state, stream) / dcf_guard_disarm(stream): the sticky numerics word of the conv-gradient operators
 * (dcf_op_conv_bwd_*, dcf_op_conv5s2_bwd_*, dcf_op_layernorm_bwd, dcf_op_vidmap_shared_bwd) under the guard.  Disarmed -- the
 * default -- a non-finite sum in one of them makes the NEXT such call return -1 once.  While a guard is armed no call fails for the
 * word; it stays on the device, the final pass of dcf_guard_grad_norm on the ARMED state ORs it into the verdict, records it in
 * conv_flag and clears it there.  One guard is armed per process; arming another state replaces it.  dcf_guard_disarm restores the
 * default and queues the word's copy to the host on `stream`: a word raised while armed that no guarded norm consumed fails the next
 * call, as it would have without the guard.  A word that was already pending on the host when the guard was armed does the same
 * after the guard is disarmed.  The forward's numerics word (dcf_numerics_status) is not involved.
 */
#ifndef DECAFNET_HIP_GUARD_H
#define DECAFNET_HIP_GUARD_H

#include <stdint.h>

#include "decafnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCF_GUARD_EXT_VERSION 1
#define DCF_GUARD_APPLY 0
#define DCF_GUARD_SKIP 1

typedef struct dcf_guard_state {
  int32_t verdict;
  int32_t first_bad_row;
  int32_t n_bad_rows;
  int32_t reserved0;
  int64_t applied;
  int64_t skipped;
  int64_t last_skipped_attempt;
  int32_t conv_flag;
  int32_t reserved1;
} dcf_guard_state;

int dcf_guard_ext_version(void);

int dcf_guard_grad_norm(const dcf_optim_row* table, const int32_t* chunk_map, int32_t n_tensors, int64_t n_chunks, float max_norm,
                        float* norm_out, float* coef_out, dcf_guard_state* state, void* stream);

int dcf_guard_adam_step(const dcf_optim_row* table, const int32_t* chunk_map, int32_t n_tensors, int64_t n_chunks,
                        const dcf_optim_group* groups, int32_t n_groups, const float* coef, const dcf_guard_state* state,
                        int32_t with_ema, float ema_beta, void* stream);

int dcf_guard_arm(const dcf_guard_state* state, void* stream);

int dcf_guard_disarm(void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DECAFNET_HIP_GUARD_H */
