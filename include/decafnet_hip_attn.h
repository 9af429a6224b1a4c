/* decafnet_hip_attn.h -- the attention-gradient extension of libdecafnet_hip.so.
 *
 * include/decafnet_hip.h is ABI version 12 and frozen; include/decafnet_hip_train.h and include/decafnet_hip_dist.h are extensions
 * of version 1 each and frozen too.  The backward of GLOBAL self-attention (MaskedMHA with window_size = 0 over one sequence, the
 * forward of dcf_op_local_attn(..., window = 0)) is declared here, lives in the same shared object and carries a version of its own,
 * dcf_attn_ext_version().  dcf_op_local_attn_bwd of decafnet_hip.h keeps its contract: it fails for window = 0.
 *
 * Version 1: dcf_op_global_attn_bwd (csrc/global_attn_grad.hip).
 *
 * Conventions are those of the dcf_op_* family of decafnet_hip.h: token-major fp32 rows [B*T][C] at 16-byte alignment, heads
 * concatenated along C, one byte per row in a mask, everything on `stream` without a host wait, scratch allocated and freed on
 * `stream`, no atomics and one fixed summation order (equal inputs give equal bits), 0 on success and -1 with dcf_last_error()
 * otherwise. */
#ifndef DECAFNET_HIP_ATTN_H
#define DECAFNET_HIP_ATTN_H

#include <stdint.h>

#include "decafnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCF_ATTN_EXT_VERSION 1
int dcf_attn_ext_version(void);

/* Gradient of the global self-attention core.  Per sequence b, head h, d = C / heads, scale = d^-1/4 on q and on k:
 *   s[t,j]  = (scale q[t]) . (scale k[j])     over the keys j < T with mask[b,j] != 0; a masked key is excluded exactly (-inf)
 *   p[t,.]  = softmax_j s[t,j],   O[t] = sum_j p[t,j] v[j]
 *   dP[t,j] = dO[t] . v[j],   delta[t] = sum_j p[t,j] dP[t,j],   dS[t,j] = p[t,j] (dP[t,j] - delta[t])
 *   dV[j] = sum_t p[t,j] dO[t],   dQ[t] = scale^2 sum_j dS[t,j] k[j],   dK[j] = scale^2 sum_t dS[t,j] q[t]
 * Q, K, V, dO and the outputs are [B*T][C]; mask is [B*T] or NULL = every row valid.
 *  - The mask masks KEYS only.  A padded query row is an ordinary row: it has an output in the forward, it takes a dQ, and it feeds
 *    dK / dV with whatever dO holds there (a caller that wants no contribution from it zeroes dO at that row).
 *  - At a padded key row dK = dV = 0 exactly.
 *  - A sequence without a valid key gives O = 0 in the forward, where the reference gives NaN; its dQ = dK = dV = 0.  This is a
 *    defined deviation.
 *  - Any of dQ / dK / dV may be NULL: the work that only feeds it is skipped and the others keep their bits.  All three NULL is a
 *    no-op.
 *  - delta is formed from p and dP, not from a stored O; scaling dO by a power of two scales each output by exactly that.
 * Head dimension 32 or 64 (the forward's), C <= 1024, any T >= 1, B <= 65535; anything else fails with a message and launches
 * nothing.  fp32 on the vector ALU. */
int dcf_op_global_attn_bwd(const float* Q, const float* K, const float* V, const uint8_t* mask, const float* dO,
                           float* dQ, float* dK, float* dV, int32_t B, int32_t T, int32_t C, int32_t heads, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DECAFNET_HIP_ATTN_H */
