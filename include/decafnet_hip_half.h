/* decafnet_hip_half.h -- the half-feature extension of libdecafnet_hip.so.
 *
 * include/decafnet_hip.h is ABI version 12 and frozen; include/decafnet_hip_train.h, include/decafnet_hip_dist.h,
 * include/decafnet_hip_attn.h, include/decafnet_hip_front.h, include/decafnet_hip_guard.h and include/decafnet_hip_clock.h are
 * extensions of version 1 each and frozen too.  The eval forward on clip features stored as IEEE binary16 is declared here, lives in
 * the same shared object and carries a version of its own, dcf_half_ext_version().
 *
 * Version 1: dcf_forward_eval_h, dcf_forward_eval_videos_h (csrc/engine.hip), dcf_op_linear_cm_split_h, dcf_op_linear_cm_split_ld_h,
 * dcf_op_sidekick_h (csrc/half.hip).
 *
 * A half operand is `const uint16_t*`: the bits of binary16 values in device memory, in the layout of the fp32 operand it replaces
 * ((D, T) channel-major, T contiguous).  Every finite value, subnormals included, is read exactly as stored; what a call returns is what
 * its fp32 counterpart returns on the same values upcast to fp32 (equal as numbers; a zero may differ in sign).  Everything else --
 * text, text_cls, weights, masks, outputs -- is fp32 / bytes as in decafnet_hip.h.
 *
 * dcf_forward_eval_h, dcf_forward_eval_videos_h
 *   dcf_forward_eval / dcf_forward_eval_videos with half `vid` and `shallow_vid`; every video of a call is half.  Where the model runs the
 *   split-operand GEMMs (gemm_mode f16x3 / bf16x6), E % 128 == 0, T % 4 == 0 and the feature pointers are 8-byte aligned, the kernels that
 *   read the features read the half values themselves (the vid_map products with the sidekick scores on their side, the scoring kernels):
 *   half the bytes, and in the f16x3 mode one operand plane and two matrix products per K chunk instead of two and three.  Otherwise the
 *   features are upcast once into an engine-owned workspace and the fp32 path runs.  dcf_debug_set_option("half_native", v) chooses: 1
 *   (default) native where possible, 0 always the upcast, 2 native or the call fails with a message -- how a test asserts which path ran;
 *   with dcf_profile_enable the native launches are listed as "...,chanmajor_h>" / "sidekick_score_h", the upcast as "half_to_f32".
 *   A non-finite feature raises bit 0 of dcf_numerics_status as it does in the fp32 forward.  A captured graph is keyed by the operand
 *   type: an fp32 and a half forward never share one.
 *
 * dcf_op_linear_cm_split_h(A_cm, W, bias, C, M, N, K, nterms, unscaled, stream)
 *   dcf_op_linear_cm_split with A_cm (K, M) half.  unscaled = 0: the activation scale 2^4 of dcf_op_linear_cm_split (|a| < 4094),
 *   comparable with it bit for bit; unscaled = 1: the engine's unscaled planes (|a| <= 65504).  nterms 16 (f16x3) or 6 (bf16x6).
 *   M % 4 == 0, N % 128 == 0, K % 32 == 0 and an 8-byte aligned A_cm, or the call fails with a message before anything is launched.
 *
 * dcf_op_linear_cm_split_ld_h(A_cm, lda, W, bias, C, M, N, K, nterms, unscaled, stream)
 *   The same product with a row pitch of its own: row k of A_cm starts lda halves behind row k - 1 and its first M values are used (a
 *   window of M clips of a longer (K, lda) feature matrix).  lda >= M and lda % 4 == 0, or the call fails before a launch;
 *   dcf_op_linear_cm_split_h is this call with lda = M.
 *
 * dcf_op_sidekick_h(shallow, text_cls, correl, D, T, nq, norm, stream)
 *   dcf_op_sidekick with shallow (D, T) half; any D, T >= 1 (8-byte loads where shallow is 8-byte aligned and T % 4 == 0).
 *
 * Not here: half features in dcf_forward_train_videos, in the gated / T-sharded forwards (dcf_forward_eval_gated, dcf_hybrid_*) and
 * in the training front end; bf16 or 8-bit features; half text.
 *
 * Everything runs on `stream` without a host wait.  0 on success, -1 with dcf_last_error() otherwise. */
#ifndef DECAFNET_HIP_HALF_H
#define DECAFNET_HIP_HALF_H

#include <stdint.h>

#include "decafnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCF_HALF_EXT_VERSION 1

int dcf_half_ext_version(void);

int dcf_forward_eval_h(dcf_model* m, const uint16_t* vid, const uint16_t* shallow_vid, const uint8_t* vid_mask, int64_t T,
                       int32_t nq, const float* const* text, const uint8_t* const* text_mask, const int32_t* text_len,
                       const float* text_cls, float* logits_out, float* offsets_out, uint8_t* masks_out, void* stream);

int dcf_forward_eval_videos_h(dcf_model* m, int32_t nvid, const uint16_t* const* vid, const uint16_t* const* shallow_vid,
                              const uint8_t* const* vid_mask, int64_t T, const int32_t* nq_per_video, const float* const* text,
                              const uint8_t* const* text_mask, const int32_t* text_len, const float* const* text_cls,
                              float* logits_out, float* offsets_out, uint8_t* masks_out, void* stream);

int dcf_op_linear_cm_split_h(const uint16_t* A_cm, const float* W, const float* bias, float* C, int32_t M, int32_t N, int32_t K,
                             int32_t nterms, int32_t unscaled, void* stream);

int dcf_op_linear_cm_split_ld_h(const uint16_t* A_cm, int64_t lda, const float* W, const float* bias, float* C, int32_t M, int32_t N,
                                int32_t K, int32_t nterms, int32_t unscaled, void* stream);

int dcf_op_sidekick_h(const uint16_t* shallow, const float* text_cls, float* correl, int32_t D, int32_t T, int32_t nq,
                      int32_t norm, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DECAFNET_HIP_HALF_H */
