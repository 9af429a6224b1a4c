/* decafnet_hip_embd.h -- the embedding-stage extension of libdecafnet_hip.so.
 *
 * include/decafnet_hip.h is ABI version 12 and frozen; include/decafnet_hip_train.h, include/decafnet_hip_dist.h,
 * include/decafnet_hip_attn.h, include/decafnet_hip_front.h, include/decafnet_hip_guard.h, include/decafnet_hip_clock.h,
 * include/decafnet_hip_half.h and include/decafnet_hip_front_half.h are extensions of version 1 each and frozen too.  The level-0
 * embedding stage of the video backbone as a single operator is declared here, lives in the same shared object and carries a version
 * of its own, dcf_embd_ext_version().
 *
 * Version 1: dcf_op_embd_chain, dcf_op_embd_launches (csrc/ops_api.hip).
 *
 * Both compute, on a FINALIZED model's own parameters (E = 256, early fusion, vid_net.stride 1, two embedding convolutions, f16x3),
 *
 *   Y = relu(LN_2(conv_2(relu(LN_1(conv_1(embd_fc(x^))))))) + pe[t] * mask          (video_net.py:133-151)
 *
 * over B sequences of T rows laid back to back, X [B * T][ldx] -> Y [B * T][ldy] (fp32, 16-byte aligned, pitches multiples of 4 and
 * >= E, Y distinct from X), `mask` [B * T] the row validity.  conv_i is MaskedConv1D(k3): it multiplies its input by the mask, its
 * output is not masked; padded rows of Y hold finite values nobody should read.
 *   ln_in = 1: X is the raw fused stream and x^ = fusion.ln_out(X) (LayerNorm with the model's affine, eps 1e-5);
 *   ln_in = 0: X holds fusion.ln_out's output already, x^ = X.
 *   pe: (>= T, E) position encoding, or NULL for none.
 *
 * dcf_op_embd_chain runs the one-kernel form (csrc/head_chain.hip, k_embd_chain): embd_fc and, with ln_in, the affine of
 * fusion.ln_out are folded into the first convolution's weight image and three per-tap bias vectors when the model is finalized.  It
 * does not look at the engine's row threshold (embd_chain_min_rows) and fails with a message where the model has no images: another
 * arithmetic mode or shape, or a folded weight beyond the scaled fp16 range (|w| >= 255.9).
 *
 * dcf_op_embd_launches runs the launch sequence that kernel replaces in a forward, on the same operands: LayerNorm (ln_in), the
 * embd_fc GEMM, and per convolution a tap-3 GEMM and a LayerNorm + ReLU launch, the last one with + pe * mask.  Intermediate rows
 * live in stream-ordered scratch.
 *
 * In a forward the engine takes the one-kernel form from 16 384 level-0 rows on.  Two names of dcf_debug_set_option belong to it:
 * "embd_chain" (0: never; default 1) and "embd_chain_min_rows" (the row threshold; tests lower it to 0); a negative value restores
 * the built-in one.  It is not taken by late fusion, vid_net.stride > 1, the other arithmetic modes, the dropout forward, or while a
 * dcf_debug_copy tap is armed.  A third name came with the extension's tests: "gemm_uniform" (1: the dense GEMM picks its kernel
 * without looking at the grid size -- 64x128 tiles wherever N allows, never the k-sliced kernel, no LayerNorm or AdaLN fused
 * into an epilogue; slower; default 0), for comparing forwards of different batch sizes bit for bit.
 *
 * An operand beyond the scaled fp16 range (|x| >= 4094 on the rows the products read) raises the model's sticky numerics flag
 * (dcf_numerics_status) in both.  Equal inputs give equal bits; a row's bits do not depend on how many sequences lie beside its own.
 *
 * Everything runs on `stream` without a host wait; scratch is allocated and freed on `stream`.  0 on success, -1 with
 * dcf_last_error() otherwise. */
#ifndef DECAFNET_HIP_EMBD_H
#define DECAFNET_HIP_EMBD_H

#include <stdint.h>

#include "decafnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCF_EMBD_EXT_VERSION 1

int dcf_embd_ext_version(void);

int dcf_op_embd_chain(dcf_model* model, const float* X, int64_t ldx, const uint8_t* mask, int32_t B, int32_t T, int32_t ln_in,
                      const float* pe, float* Y, int64_t ldy, void* stream);

int dcf_op_embd_launches(dcf_model* model, const float* X, int64_t ldx, const uint8_t* mask, int32_t B, int32_t T, int32_t ln_in,
                         const float* pe, float* Y, int64_t ldy, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DECAFNET_HIP_EMBD_H */
