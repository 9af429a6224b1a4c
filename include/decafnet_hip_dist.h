/* decafnet_hip_dist.h -- the data-parallel extension of libdecafnet_hip.so.
 *
 * include/decafnet_hip.h is ABI version 12 and frozen, include/decafnet_hip_train.h is training-extension version 1 and frozen
 * too.  What a data-parallel training step needs on top of them is declared here, lives in the same shared object and carries a
 * version of its own, dcf_dist_ext_version().  A caller that trains on one rank never includes this file.
 *
 * Version 1: the gradient bucket pack (csrc/grad_bucket.hip).
 *
 * Conventions are those of the dcf_optim_* family of decafnet_hip.h: a device table of dcf_optim_row records (64 bytes each) and its
 * chunk map (chunk_map[c] = the row that chunk c belongs to, row.chunk0 = the first chunk of the row, DCF_OPTIM_CHUNK elements per
 * chunk), fp32 tensors at any 4-byte alignment, everything on `stream` without a host wait, no scratch, no atomics (equal inputs
 * give equal bits), 0 on success and -1 with dcf_last_error() otherwise. */
#ifndef DECAFNET_HIP_DIST_H
#define DECAFNET_HIP_DIST_H

#include <stdint.h>

#include "decafnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCF_DIST_EXT_VERSION 1
int dcf_dist_ext_version(void);

/* Pack the gradients of one bucket into their slices of the bucket arena, pre-divided for the sum over the ranks:
 *   dst = row.p (the slice), src = row.g (the gradient autograd left), dst[i] = src[i] * scale for i < row.n
 * One fp32 multiplication, one rounding; with scale == 1.0f the bits are copied and nothing is multiplied.  A row with
 * DCF_OPTIM_NO_GRAD in its flags or with g == NULL writes +0 to its slice.  exp_avg, exp_avg_sq, ema and group of a row are not
 * read.  dst may be src (the scaling then happens in place); otherwise the two do not overlap.  Nothing outside [dst, dst + n) of
 * any row is written.  n_chunks == 0 is a no-op.  One workgroup per chunk: 8 bytes of traffic per element. */
int dcf_dist_pack_grads(const dcf_optim_row* table, const int32_t* chunk_map, int32_t n_tensors, int64_t n_chunks, float scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DECAFNET_HIP_DIST_H */
