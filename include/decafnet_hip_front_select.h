/* decafnet_hip_front_select.h -- selected-clip training: vid_map and its weight gradient on expert rows.  An extension of
 * libdecafnet_hip.so.
 *
 * include/decafnet_hip.h is ABI version 12 and frozen, and so are the extension headers beside it.  decafnet_hip_front.h is vid_map
 * of the training step on DENSE (nvid, D, T) expert features; decafnet_hip_select_videos.h is the calling pattern the top-k gate
 * exists for -- ask which clips the gates need, run the expert encoder on those alone -- for inference.  This extension is that
 * pattern for the training step: the forward and the weight gradient of vid_map on the packed (n_rows, D) expert rows of the
 * selected clips.  Nothing of size (nvid, D, T) is read, built or kept on the expert side.
 *
 * Version 1 (csrc/front_select.hip): dcf_op_vidmap_selected, dcf_op_vidmap_selected_bwd and their _h forms.
 *
 * Operands (fp32 unless stated, on the device unless stated):
 *   rows        (>= row_first[nvid], D) clip-major and packed: video v's rows start at row_first[v], row i of them holds the expert
 *               features of the i-th selected clip of the video.  Rows at and beyond row_first[nvid] are never read (a capacity buffer).
 *               The fp32 forward needs a 16-byte aligned base (both row GEMMs load 16 bytes); the other three take any alignment.
 *   row_first   HOST (nvid + 1) int32: strictly increasing from 0 (every video has at least one row), at most T rows per video
 *   pos         (nvid, T) int32, video-local, as dcf_op_select_clips_videos writes it: the row of clip t among its video's, or -1.
 *               -1 means "no expert half at this clip" whatever the gate says: documented, not detected, as in the forwards of
 *               decafnet_hip_select_videos.h.  An entry at or beyond the video's row count is ignored by the backward.
 *   shallow     (nvid, D, T) channel-major, or NULL (no msf)
 *   nq          HOST (nvid) int32: the queries of each video, every one >= 1; B' = sum nq; rows of gate / mask / correl / Y / dY are in
 *               (video, query) order
 *   gate, mask, correl, W, bias, Y, dY, dW, db, accumulate: exactly as in decafnet_hip_front.h
 *
 * Forward:
 *   P1c = rows . W1^T                                  ONE row-major product over the packed rows of all videos: the split-operand
 *                                                      (f16x3) row GEMM where E % 128 == 0, the fp32 tile GEMM otherwise
 *   P2[v] = shallow[v]^T W2^T                          once per video, as dcf_op_vidmap_shared computes it
 *   Y[q,t,:] = bias + m ( g P1c[row_first[v] + pos[v,t], :] + P2[v,t,:] + c w3 )
 * Backward (dY is NOT assumed masked; db runs over every row):
 *   R1c[row_first[v] + pos[v,t], :] = sum_{q in v} m g dY[q,t,:]   where pos[v,t] >= 0; every other packed row is zero
 *   R2[v,t,:] = sum_{q in v} m dY[q,t,:]
 *   dW1[e,d] = sum_i R1c[i,e] rows[i,d],  dW2[e,d] = sum_v sum_t R2[v,t,e] shallow[v,d,t]
 *   dw3[e] = sum_{q,t} m c dY[q,t,e],  db[e] = sum_{q,t} dY[q,t,e]
 * With pos a bijection between the clips some query keeps and the packed rows, these are dcf_op_vidmap_shared /
 * dcf_op_vidmap_shared_bwd on the dense features with the zero rows left out.  There is no gradient to the features, the gate or the
 * scores: they are data.
 *
 *  - The _h forms take rows and shallow as IEEE binary16 (both; one of the two cannot be expressed in this interface) and return the
 *    bits of the fp32 operators on the upcast values.  The _h forward upcasts rows once into scratch (and shallow where the half
 *    channel-major product does not apply); the _h backward reads both as stored: no fp32 copy of either is made.
 *  - db may be NULL.  accumulate != 0 adds to dW / db instead of overwriting them.
 *  - Arithmetic of the weight gradient: f16x3 on the matrix cores, R1c / R2 scaled on the device by a power of two from their own
 *    maxima, a number of row slices that follows from the shapes (row_first[nvid], D, E) alone, fp32 partials summed in a fixed order,
 *    no floating-point atomics: equal inputs give equal bits, and 2^k dY gives 2^k dW, 2^k db exactly.  A non-finite sum raises the
 *    sticky word of the conv-gradient operators: the NEXT call of one of them (or of these) returns -1 with the message.
 *  - 1 <= nvid <= 16, D % 32 == 0, E % 32 == 0, E <= 1024, T >= 1, every nq[v] >= 1, B' T < 2^31 - 64, row_first as above; anything else
 *    fails with a message before a launch.  Everything runs on `stream` without a host wait; scratch is allocated and freed on
 *    `stream`; ordinary vector stores.  0 on success, -1 with dcf_last_error() otherwise.
 *
 * Not here: a gradient through a T-sharded forward, and HIP-graph capture of the step. */
#ifndef DECAFNET_HIP_FRONT_SELECT_H
#define DECAFNET_HIP_FRONT_SELECT_H

#include <stdint.h>

#include "decafnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCF_FRONT_SELECT_EXT_VERSION 1
int dcf_front_select_ext_version(void);

int dcf_op_vidmap_selected(const float* rows, const int32_t* row_first, const int32_t* pos, const float* shallow, const float* W,
                           const float* bias, const float* gate, const uint8_t* mask, const float* correl, const int32_t* nq, float* Y,
                           int32_t nvid, int32_t D, int32_t T, int32_t E, void* stream);

int dcf_op_vidmap_selected_bwd(const float* rows, const int32_t* row_first, const int32_t* pos, const float* shallow, const float* gate,
                               const uint8_t* mask, const float* correl, const int32_t* nq, const float* dY, float* dW, float* db,
                               int32_t nvid, int32_t D, int32_t T, int32_t E, int32_t accumulate, void* stream);

int dcf_op_vidmap_selected_h(const uint16_t* rows, const int32_t* row_first, const int32_t* pos, const uint16_t* shallow, const float* W,
                             const float* bias, const float* gate, const uint8_t* mask, const float* correl, const int32_t* nq, float* Y,
                             int32_t nvid, int32_t D, int32_t T, int32_t E, void* stream);

int dcf_op_vidmap_selected_bwd_h(const uint16_t* rows, const int32_t* row_first, const int32_t* pos, const uint16_t* shallow,
                                 const float* gate, const uint8_t* mask, const float* correl, const int32_t* nq, const float* dY, float* dW,
                                 float* db, int32_t nvid, int32_t D, int32_t T, int32_t E, int32_t accumulate, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DECAFNET_HIP_FRONT_SELECT_H */
