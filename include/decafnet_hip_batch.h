/* decafnet_hip_batch.h -- the batch-assembly extension of libdecafnet_hip.so.
 *
 * include/decafnet_hip.h is ABI version 12 and frozen.  What a training data path needs to make a batch out of a feature bank that
 * lives in device memory is declared here, lives in the same shared object and carries a version of its own,
 * dcf_batch_ext_version().  A caller that feeds the step from host tensors never includes this file.
 *
 * Version 1: the ragged transpose of feature rows into a padded channel-major batch (csrc/batch.hip).
 *
 * Conventions: everything on `stream` without a host wait, no scratch, no atomics (equal inputs give equal bits), 0 on success and
 * -1 with dcf_last_error() otherwise. */
#ifndef DECAFNET_HIP_BATCH_H
#define DECAFNET_HIP_BATCH_H

#include <stdint.h>

#include "decafnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCF_BATCH_EXT_VERSION 1
int dcf_batch_ext_version(void);

/* Assemble B windows of a feature bank into one padded channel-major batch.
 *
 * `bank` holds feature rows as the files store them, row-major (rows, C), of elements `elem_bytes` wide (2: IEEE binary16, 4: fp32
 * or any other 4-byte type; the operator moves bits and interprets nothing).  `desc` is a device array (B, 2) of int64: the ELEMENT
 * offset off_b of the first row of window b in `bank` (row index * C), and its number of rows n_b.
 *
 *   out[b, c, t]  = bank[off_b + t * C + c]   for t <  n_b
 *   out[b, c, t]  = 0 (all bits)              for n_b <= t < T_out
 *   mask[b, t]    = t < n_b (one byte, 0 / 1) where mask != NULL
 *
 * Every byte of `out` (B, C, T_out) and of `mask` (B, T_out) is written: no memset before the call.  NaN payloads and negative
 * zeros arrive unchanged.  n_b is clamped to [0, T_out] on the device, so no descriptor makes the operator write outside `out` or
 * `mask`; n_b = 0 is an all-padding window.  What the operator READS is bank[off_b, off_b + n_b * C): the caller keeps every
 * window inside its video.  Windows may overlap.  `bank` and `out` are aligned to `elem_bytes` and to nothing more: binary16 rows
 * of odd C or an odd first row are read through 2-byte loads where a 4-byte load would be misaligned.  `out` does not overlap
 * `bank`.
 *
 * Refused before any launch: elem_bytes other than 2 or 4; B, C or T_out < 1; a null bank, desc or out; bank or out not aligned to
 * elem_bytes; more than 65535 windows or channel tiles. */
int32_t dcf_op_assemble_rows(const void* bank, int32_t elem_bytes, const int64_t* desc, int32_t B, int32_t C, int64_t T_out, void* out,
                             uint8_t* mask, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DECAFNET_HIP_BATCH_H */
