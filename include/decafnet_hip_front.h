/* decafnet_hip_front.h -- the training-front-end extension of libdecafnet_hip.so.
 *
 * include/decafnet_hip.h is ABI version 12 and frozen; include/decafnet_hip_train.h, include/decafnet_hip_dist.h and
 * include/decafnet_hip_attn.h are extensions of version 1 each and frozen too.  vid_map on shared products -- the first stage of
 * the training forward (model.py:567-583) and its weight gradient -- is declared here, lives in the same shared object and carries a
 * version of its own, dcf_front_ext_version().
 *
 * Version 1: dcf_op_vidmap_shared, dcf_op_vidmap_shared_bwd (csrc/front_grad.hip).
 *
 * Operands (fp32 unless stated, 16-byte aligned, on the device unless stated):
 *   vid, shallow  (nvid, D, T) channel-major, as the reference's batch holds them; shallow NULL = no msf
 *   nq            HOST array of nvid int32: the queries of each video, every one >= 1; B' = sum nq; rows are in (video, query) order
 *   gate          (B', T) 0 / 1, mask (B', T) bytes, correl (B', T): the outputs of dcf_op_gate / dcf_op_sidekick; correl NULL = no scat
 *   W, dW         PyTorch's (E, Cin), Cin = D [+ D with shallow] [+ 1 with correl]: W1 = W[:, :D], W2 = W[:, D:2D], w3 = W[:, Cin-1]
 *   bias, db      (E)
 *   Y, dY         (B' T, E) token-major
 *
 * Forward (MaskedConv1D k = 1 on the gated, concatenated input, as k_vidmap_combine of the inference engine computes it):
 *   P1[b] = vid[b]^T W1^T,  P2[b] = shallow[b]^T W2^T           once per video
 *   Y[q,t,:] = bias + m[q,t] ( g[q,t] P1[b,t,:] + P2[b,t,:] + c[q,t] w3 )
 * Backward (dY is NOT assumed masked; db runs over every row, like dcf_op_conv_bwd_weight):
 *   R1[b,t,:] = sum_{q in b} m g dY[q,t,:],  R2[b,t,:] = sum_{q in b} m dY[q,t,:]
 *   dW1[e,d] = sum_b sum_t R1[b,t,e] vid[b,d,t],  dW2 likewise from R2 and shallow
 *   dw3[e] = sum_{q,t} m c dY[q,t,e],  db[e] = sum_{q,t} dY[q,t,e]
 * There is no gradient to the features, the gate or the scores: they are data.
 *
 *  - A 64-clip tile of video b in which no query of b has gate != 0 is not computed in P1 (on the split tile path of the forward
 *    product) and contributes no K step to dW1; the flags are derived from `gate` inside the call.  flags bit 0
 *    (DCF_FRONT_NO_SKIP) switches that off: the results have the same bits while vid is finite.
 *  - db may be NULL.  accumulate != 0 adds to dW / db instead of overwriting them.
 *  - Arithmetic of the weight gradient: f16x3 on the matrix cores, R scaled on the device by a power of two from its own maximum,
 *    fixed T slices whose fp32 partials are summed in a fixed order, no floating-point atomics: equal inputs give equal bits, and
 *    2^k dY gives 2^k dW, 2^k db exactly.  A non-finite sum raises the sticky word of the conv-gradient operators: the NEXT call of
 *    one of them (or of these two) returns -1 with the message.
 *  - D % 32 == 0, E % 32 == 0, E <= 1024, any T >= 1, every nq[b] >= 1, B' T < 2^31 - 64; anything else fails with a message before
 *    a launch.  Everything runs on `stream` without a host wait; scratch is allocated and freed on `stream`.  0 on success, -1 with
 *    dcf_last_error() otherwise. */
#ifndef DECAFNET_HIP_FRONT_H
#define DECAFNET_HIP_FRONT_H

#include <stdint.h>

#include "decafnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCF_FRONT_EXT_VERSION 1
#define DCF_FRONT_NO_SKIP 1
int dcf_front_ext_version(void);

int dcf_op_vidmap_shared(const float* vid, const float* shallow, const float* W, const float* bias, const float* gate,
                         const uint8_t* mask, const float* correl, const int32_t* nq, float* Y, int32_t nvid, int32_t D, int32_t T,
                         int32_t E, int32_t flags, void* stream);

int dcf_op_vidmap_shared_bwd(const float* vid, const float* shallow, const float* gate, const uint8_t* mask, const float* correl,
                             const int32_t* nq, const float* dY, float* dW, float* db, int32_t nvid, int32_t D, int32_t T, int32_t E,
                             int32_t flags, int32_t accumulate, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DECAFNET_HIP_FRONT_H */
