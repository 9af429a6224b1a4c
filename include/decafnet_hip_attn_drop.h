/* decafnet_hip_attn_drop.h -- the attention-map-dropout extension of libdecafnet_hip.so.
 *
 * include/decafnet_hip.h is ABI version 12 and frozen, and so are the extension headers beside it.  nn.Dropout(attn_pdrop) of the
 * reference acts on the softmax map inside MaskedMHA (blocks.py:368).  The attention cores here never put that map into memory, so
 * the keep bits are drawn inside the kernels, forward and backward.  Those forms of the cores, and channel dropout (nn.Dropout1d,
 * model.py:614), are declared here, live in the same shared object and carry a version of their own, dcf_attn_drop_ext_version().
 * The dropout-free exports (dcf_op_local_attn, dcf_op_local_attn_bwd) keep their contract and their compiled code.
 *
 * Version 1 (csrc/attn_drop.hip):
 *   dcf_op_local_attn_drop        the sliding-window core (window odd and positive) and, with window = 0, global self attention,
 *                                 with dropout on the map
 *   dcf_op_local_attn_drop_bwd    the gradient of the sliding-window form
 *   dcf_op_global_attn_drop_bwd   the gradient of the global form
 *   dcf_op_xattn_drop, _bwd       cross attention with dropout on its map, and its gradient
 *   dcf_op_channel_dropout        one keep decision per (sample, channel); its own backward
 * At p = 0 every attention export runs its dropout-free export after its own checks: the same bits by construction.
 *
 * Conventions are those of the dcf_op_* family of decafnet_hip.h: token-major fp32 rows [B*T][C] at 16-byte alignment, heads
 * concatenated along C, one byte per row in a mask (non-zero = valid), everything on `stream` without a host wait, scratch allocated
 * and freed on `stream`, no floating-point atomics and one fixed summation order (equal inputs give equal bits), 0 on success and
 * -1 with dcf_last_error() otherwise.  An unsupported shape fails with a message before any launch or allocation.
 *
 * The random stream is the one of decafnet_hip_train.h, unchanged: Philox4x32-10 keyed by the 64-bit `seed`, counter
 * (j & 0xffffffff, j >> 32, site, 0) with j = e >> 2, element e takes word e & 3, u = (word >> 8) * 2^-24, kept iff u >= p, keep factor
 * k(e) = kept ? scale : 0 with scale = 1.0f / (1.0f - p) computed in fp32, a dropped element is +0, p in [0, 1), b0 >= 0.  No operator
 * stores a mask: a backward draws the same bits again from (seed, site, e).
 *
 * The element index is the flat index of the tensor the reference hands to its nn.Dropout, the sample index offset by b0.  e is a
 * 64-bit number.
 *   local window, W = window   the (bs, H, T, W) map of blocks.py:364-368    e = (((b0 + b) H + h) T + t) W + j
 *                              Slot j of row t is key t - W / 2 + j.  This is the order of the reference's chunked layout
 *                              (_query_key_matmul fills slot j with the product of query t and key t - W / 2 + j).  A slot whose key
 *                              lies outside the sequence takes an index like any other; its draw is not used.
 *   global self attention      the (bs, H, T, T) map of blocks.py:379-388         e = (((b0 + b) H + h) T + t) T + j,   j the key
 *   cross attention            the (B', H, T, Lk) map                             e = (((b0 + b) H + h) T + t) Lk + j,  j the key
 *   channel dropout            one decision per (b, c) of a (B', Cin, T) tensor  e = (b0 + b) Cin + c
 *
 * Sites are numbered site = group << 16 | layer << 4 | sub as before.  This extension adds
 *   sub 6    DROP_ATTN      the attention map of block `layer` of a group
 *   sub 7    DROP_CHANNEL   channel dropout; group 7 (DROP_G_INPUT), layer 0: the clip features before vid_map
 * The operators take any site word; the numbering is the caller's contract with its CPU restatement. */
#ifndef DECAFNET_HIP_ATTN_DROP_H
#define DECAFNET_HIP_ATTN_DROP_H

#include <stdint.h>

#include "decafnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCF_ATTN_DROP_EXT_VERSION 1
int dcf_attn_drop_ext_version(void);

/* The sliding-window attention core with dropout on its map.  P is the softmax map of dcf_op_local_attn: the same scores, the same
 * -1e4 at a padded key, a padded QUERY row has P = 0 and O = 0.  With Pd[t,j] = kept ? P[t,j] * scale : +0,
 *   O[t] = sum_j Pd[t,j] v[j]
 * The softmax is carried online as in the dropout-free core, so the factor multiplies the weight exp(s - m) where it enters the
 * output's accumulator and not where it enters the row sum.
 *  - With p = 0 the output has the bits of dcf_op_local_attn on the same operands: the call runs the dropout-free kernel itself, after
 *    the checks of this export (b0, p and the shape are checked at every p).
 *  - A (row, head) whose valid keys are all dropped gives O = +0 exactly.
 *  - Sequence b of a call with b0 = n has the bits of sequence b + n of a call on the larger batch with b0 = 0.
 * window odd and >= 1 (window = 0: the global form below); mask is required; the shape limits are those of dcf_op_local_attn: head dimension a power of two in
 * [4, 256], C a multiple of 4 up to 1024, B * T < 2^31 - 64. */
int dcf_op_local_attn_drop(const float* Q, const float* K, const float* V, const uint8_t* mask, float* O, int32_t B, int32_t T, int32_t C,
                           int32_t heads, int32_t window, int32_t b0, int64_t seed, int32_t site, float p, void* stream);

/* Its gradient, with the contract of dcf_op_local_attn_bwd (mask NULL = every row valid; any of dQ / dK / dV may be NULL: the work
 * that only feeds it is skipped and the others keep their bits; all three NULL is a no-op).  With k the keep factor:
 *   dPd[t,j] = dO[t] . v[j],   dP = k o dPd,   delta[t] = sum_j Pd[t,j] dPd[t,j]   (formed from the map, not from a stored O)
 *   dS = P o (dP - delta),   dV[j] = sum_t Pd[t,j] dO[t],   dQ[t] = scale_qk^2 sum_j dS[t,j] k[j],   dK[j] = scale_qk^2 sum_t dS[t,j] q[t]
 *  - With p = 0 the three outputs have the bits of dcf_op_local_attn_bwd on the same operands (the dropout-free kernels themselves).
 *  - A (row, head) whose valid keys are all dropped has delta = 0 and dS = 0: it gives dQ = 0 and adds exact zeros to dK and dV.
 *  - The b0 rule of the forward holds for every output.
 * For window <= 32 the keep bits of a (row, head) are drawn once, on the query side, and handed to the key side in the row-statistics
 * scratch; wider windows draw per element on both sides.  The bits are the same either way. */
int dcf_op_local_attn_drop_bwd(const float* Q, const float* K, const float* V, const uint8_t* mask, const float* dO, float* dQ, float* dK,
                               float* dV, int32_t B, int32_t T, int32_t C, int32_t heads, int32_t window, int32_t b0, int64_t seed,
                               int32_t site, float p, void* stream);

/* Global self attention and cross attention with dropout on the map.  P is the softmax map of the dropout-free core over the valid
 * keys of the sequence (a masked key is excluded exactly; d^-1/4 on q and on k), Pd = kept ? P * scale : +0, and the arithmetic is that
 * of dcf_op_local_attn_drop / _bwd above with every key of the sequence in the window.  The mask masks KEYS only: a padded query row is
 * an ordinary row.  At a masked key dK = dV = 0 exactly.  A sequence without a valid key gives O = 0 and zero gradients (for cross
 * attention the dropout-free export gives NaN there: a defined deviation at p > 0).  NULL outputs skip their work and leave the bits
 * of the others; all three NULL is a no-op.  The p = 0, fully-dropped-row and b0 rules are those above.
 *   dcf_op_local_attn_drop(window = 0) / dcf_op_global_attn_drop_bwd: Q, K, V, dO and the outputs [B*T][C]; the limits of
 *     dcf_op_local_attn(window = 0) / dcf_op_global_attn_bwd: head dimension 32 or 64, C <= 1024, B <= 65535; the forward needs its mask.
 *   dcf_op_xattn_drop / _bwd: Q, dO, O, dQ [B*T][C], K, V, dK, dV [B*Lk][C], kvmask [B*Lk] (required by the forward, NULL = every key
 *     valid in the backward); the limits of dcf_op_xattn_bwd: Lk from 1 to 64, head dimension 16, 32, 64 or 128, C <= 1024, B <= 65535.
 * At p > 0 these run plain vector-ALU kernels (a wave per query row, and per key row a gather over the T queries in ascending order:
 * one fixed summation order), not the tiled cores of the dropout-free exports; the keep bits of a (row, head) are drawn in blocks of
 * 32 keys, shared over the head's lanes, and handed to the key side as words in stream-ordered scratch. */
int dcf_op_global_attn_drop_bwd(const float* Q, const float* K, const float* V, const uint8_t* mask, const float* dO, float* dQ, float* dK,
                                float* dV, int32_t B, int32_t T, int32_t C, int32_t heads, int32_t b0, int64_t seed, int32_t site, float p,
                                void* stream);
int dcf_op_xattn_drop(const float* Q, const float* K, const float* V, const uint8_t* kvmask, float* O, int32_t B, int32_t T, int32_t Lk, int32_t C,
                      int32_t heads, int32_t b0, int64_t seed, int32_t site, float p, void* stream);
int dcf_op_xattn_drop_bwd(const float* Q, const float* K, const float* V, const uint8_t* kvmask, const float* dO, float* dQ, float* dK, float* dV,
                          int32_t B, int32_t T, int32_t Lk, int32_t C, int32_t heads, int32_t b0, int64_t seed, int32_t site, float p,
                          void* stream);

/* Channel dropout on rows [B*T][C] of a (B, C, T) tensor of the reference: Y[b,t,c] = kept(b,c) ? X[b,t,c] * scale : +0.  Y may alias
 * X.  It is its own backward (the same call on dY).  C a positive multiple of 4, B * T < 2^31 - 64. */
int dcf_op_channel_dropout(const float* X, float* Y, int32_t B, int32_t T, int32_t C, int32_t b0, int64_t seed, int32_t site, float p,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DECAFNET_HIP_ATTN_DROP_H */
