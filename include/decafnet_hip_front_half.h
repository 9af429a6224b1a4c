/* decafnet_hip_front_half.h -- the half-feature training-front-end extension of libdecafnet_hip.so.
 *
 * include/decafnet_hip.h is ABI version 12 and frozen; include/decafnet_hip_train.h, include/decafnet_hip_dist.h,
 * include/decafnet_hip_attn.h, include/decafnet_hip_front.h, include/decafnet_hip_guard.h, include/decafnet_hip_clock.h and
 * include/decafnet_hip_half.h are extensions of version 1 each and frozen too.  vid_map on shared products -- the first stage of the
 * training forward and its weight gradient -- on clip features stored as IEEE binary16 is declared here, lives in the same shared
 * object and carries a version of its own, dcf_front_half_ext_version().
 *
 * Version 1: dcf_op_vidmap_shared_h, dcf_op_vidmap_shared_bwd_h (csrc/front_grad.hip).
 *
 * The two operators are dcf_op_vidmap_shared / dcf_op_vidmap_shared_bwd of include/decafnet_hip_front.h with ONE difference: `vid`
 * and `shallow` are `const uint16_t*`, the bits of binary16 values in device memory, (nvid, D, T) channel-major.  Every other operand
 * keeps its type, its meaning and its constraints: D % 32 == 0, E % 32 == 0, E <= 1024, any T >= 1, shallow NULL = no msf, correl
 * NULL = no scat, db NULL, DCF_FRONT_NO_SKIP, accumulate, the sticky non-finite word of the conv-gradient operators, no host wait.
 * A half operand needs no alignment beyond that of its type.
 *
 * The contract is that of include/decafnet_hip_half.h: every finite value, subnormals included, is read exactly as stored, and a call
 * returns what its fp32 counterpart returns on the same values upcast to fp32 (equal as numbers; a zero may differ in sign), over the
 * fp32 operator's own operand range (it scales the features by 2^4: |x| < 4094).  The properties of the fp32 operators carry over:
 * equal inputs give equal bits, 2^k dY gives 2^k dW and 2^k db exactly, there are no floating-point atomics, and skipping the closed
 * gate tiles changes no bit while the features are finite.
 *
 * dcf_op_vidmap_shared_h
 *   Where the split tile path of the forward products applies -- E % 128 == 0, T % 4 == 0, 8-byte aligned feature pointers -- P1 / P2
 *   read the half values themselves (the A_CHANMAJOR_H mode of the channel-major GEMM: half the bytes, one operand plane and two
 *   matrix products per K chunk instead of two and three), grouped as in the fp32 operator: three videos per grid, the closed gate
 *   tiles of the expert half skipped.  Otherwise the features are upcast once into stream-ordered scratch and the fp32 path runs.
 *   dcf_debug_set_option("half_native", v) chooses as it does in the engine: 1 (default) native where possible, 0 always the upcast,
 *   2 native or the call fails with a message before anything is launched.
 *
 * dcf_op_vidmap_shared_bwd_h
 *   The weight-gradient kernel reads the stored values for every shape and alignment (16-byte loads of eight clips of one channel
 *   where the address allows, two-byte loads otherwise); nothing is upcast.  The stored value times 2^4 is the hi plane of the fp32
 *   form and its lo plane is exactly zero, so one feature plane is staged and two matrix products are issued per k-step instead of
 *   two and three, in the order of the fp32 form without its middle term.  The row sums of dY, their device-side scale, the T slices,
 *   the gate-tile skipping and the reduction of the partials are those of dcf_op_vidmap_shared_bwd.
 *
 * Not here: half features in dcf_forward_train_videos (the forward values of model(..., eval=False)), in the gated / T-sharded
 * forwards (dcf_forward_eval_gated, dcf_hybrid_*) and in the dense training front end; bf16 or 8-bit features; half text; a training
 * data loader.
 *
 * Everything runs on `stream` without a host wait; scratch is allocated and freed on `stream`.  0 on success, -1 with
 * dcf_last_error() otherwise. */
#ifndef DECAFNET_HIP_FRONT_HALF_H
#define DECAFNET_HIP_FRONT_HALF_H

#include <stdint.h>

#include "decafnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCF_FRONT_HALF_EXT_VERSION 1

int dcf_front_half_ext_version(void);

int dcf_op_vidmap_shared_h(const uint16_t* vid, const uint16_t* shallow, const float* W, const float* bias, const float* gate,
                           const uint8_t* mask, const float* correl, const int32_t* nq, float* Y, int32_t nvid, int32_t D, int32_t T,
                           int32_t E, int32_t flags, void* stream);

int dcf_op_vidmap_shared_bwd_h(const uint16_t* vid, const uint16_t* shallow, const float* gate, const uint8_t* mask,
                               const float* correl, const int32_t* nq, const float* dY, float* dW, float* db, int32_t nvid, int32_t D,
                               int32_t T, int32_t E, int32_t flags, int32_t accumulate, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DECAFNET_HIP_FRONT_HALF_H */
