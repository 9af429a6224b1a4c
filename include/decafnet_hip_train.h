/* decafnet_hip_train.h -- the training extension of libdecafnet_hip.so.
 *
 * include/decafnet_hip.h is ABI version 12 and frozen: its symbol list is what dcf_abi_version() == 12 promises.  Entry points
 * that only a training step needs and that came after it are declared here, live in the same shared object and carry a version of
 * their own, dcf_train_ext_version().  A caller that wants inference alone never includes this file.
 *
 * Version 1: dropout and drop-path of a block as differentiable operators (csrc/drop_grad.hip).
 *
 * Conventions are those of the dcf_op_* family of decafnet_hip.h: token-major fp32 rows [b][t] x C without padding, 16-byte
 * aligned pointers, masks of one byte per row (non-zero = valid, NULL = all valid), everything on `stream` without a host wait,
 * scratch allocated and freed on it, no floating-point atomics (equal inputs give equal bits), 0 on success and -1 with
 * dcf_last_error() otherwise; unsupported shapes fail with a message.
 *
 * The random stream is the one of dcf_model_set_dropout (decafnet_hip.h: Philox4x32-10, the site numbering
 * group << 16 | layer << 4 | sub, u = (word >> 8) * 2^-24, kept iff u >= p).  The rows are a (B, C, T) tensor of the reference
 * whose first sequence is sample b0 of the reference's batch, so the element index of row (b, t), column c is
 *     e = ((b0 + b) * C + c) * T + t                     and for drop-path (one decision per sample)   e = b0 + b.
 * `seed` carries the 64-bit key as dcf_debug_dropout_keep takes it.  Every p lies in [0, 1); p = 0 is the identity.  The keep
 * factor is k(e) = kept ? scale : 0 with scale = 1.0f / (1.0f - p) computed in fp32; a dropped element is +0.  No operator stores a
 * mask: a backward recomputes the keep bits from (seed, site, e).  B, T > 0, B * T < 2^31 - 64, b0 >= 0, C a multiple of 4. */
#ifndef DECAFNET_HIP_TRAIN_H
#define DECAFNET_HIP_TRAIN_H

#include <stdint.h>

#include "decafnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCF_TRAIN_EXT_VERSION 1
int dcf_train_ext_version(void);

/* Dropout: Y = k X, the kept values x * scale rounded once.  Y may alias X.  It is its own backward (dX = k dY: the same call on
 * dY).  The decoder's proj_drop acts on the (B', 2E, T) scale / shift tensor: C = 2E, sub 0 of group 1. */
int dcf_op_dropout(const float* X, float* Y, int32_t B, int32_t T, int32_t C, int32_t b0, int64_t seed, int32_t site, float p, void* stream);

/* The FFN's dropout(gelu(fc(x))) (blocks.py:535-536, sub 1) in one pass over the (B T, 4E) hidden tensor:
 *   Y  = k gelu(X)             the bits of dcf_op_dropout applied to dcf_op_gelu(X)
 *   dX = (k dY) gelu'(X)       the bits of dcf_op_gelu_bwd(X, dcf_op_dropout(dY)): the keep factor goes onto dY first
 * Y may alias X, dX may alias dY. */
int dcf_op_gelu_dropout(const float* X, float* Y, int32_t B, int32_t T, int32_t C, int32_t b0, int64_t seed, int32_t site, float p, void* stream);
int dcf_op_gelu_dropout_bwd(const float* X, const float* dY, float* dX, int32_t B, int32_t T, int32_t C, int32_t b0, int64_t seed, int32_t site,
                            float p, void* stream);

/* The residual update of a block with its dropouts (blocks.py:586 with subs 0 / 3, :589-590 with subs 2 / 4):
 *   Y = R m_R + ls[c] dp(b) k(e) (H m_H)
 * k from (drop_site, drop_p), dp(b) = kept ? 1 / (1 - path_p) : 0 from (path_site, path_p, e = b0 + b).  The kernel is the one the
 * training forward of dcf_forward_train_videos runs, evaluated per element in fp32 as
 *   v = H m_H;  v = kept ? v * scale : 0;  Y = fma(ls * v, dp, R m_R)
 * (a masked factor is a multiplication by 0.0f or 1.0f).  mR and mH, where both are given, are one array: a block has one mask.
 * With both probabilities 0 the call is dcf_op_layerscale_residual, bit for bit.  C <= 1024.  Y may alias R.
 *
 * Backward; dR, dH, dls are optional (NULL skips the work that only feeds it), dH needs ls, dls needs H; with f = dp(b) k(e):
 *   dR = dY m_R,   dH = ls (dY f) m_H,   dls[c] (+)= sum_rows (dY f) H m_H        (accumulate != 0: added to dls)
 * The column sum is dcf_op_layerscale_residual_bwd's: row runs that are a fixed function of B * T, partials in stream-ordered
 * scratch, one summation order.  The rows of a sample whose path was dropped get dH = +0 and read neither H nor the random stream.
 * With both probabilities 0 the three outputs have the bits of dcf_op_layerscale_residual_bwd. */
int dcf_op_drop_residual(const float* R, const uint8_t* mR, const float* H, const uint8_t* mH, const float* ls, float* Y, int32_t B, int32_t T,
                         int32_t C, int32_t b0, int64_t seed, int32_t drop_site, float drop_p, int32_t path_site, float path_p, void* stream);
int dcf_op_drop_residual_bwd(const float* dY, const float* H, const uint8_t* mR, const uint8_t* mH, const float* ls, float* dR, float* dH, float* dls,
                             int32_t B, int32_t T, int32_t C, int32_t b0, int64_t seed, int32_t drop_site, float drop_p, int32_t path_site,
                             float path_p, int32_t accumulate, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DECAFNET_HIP_TRAIN_H */
