/* decafnet_hip_select_videos.h -- selected-clip inference on several videos per forward: an extension of libdecafnet_hip.so.
 *
 * include/decafnet_hip.h is ABI version 12 and frozen, and so are the extension headers beside it.  decafnet_hip_select.h is the
 * calling pattern the model was designed for -- ask which clips the top-k gates need, run the expert encoder on those alone, run the
 * forward on (count, D) rows -- for ONE video per forward.  The engine's throughput configuration is several videos per forward
 * (dcf_forward_eval_videos: one launch sequence for the queries of up to 16 videos).  This extension is the same pattern for all
 * videos of a forward:
 *
 *   1. dcf_select_videos(_h)                    scores, gates and the clip lists of every video; the caller reads `counts` (nvid
 *                                               int32: the ONE host read of the pattern) and then the lists it wants to encode
 *   2. the caller runs its expert encoder on those clips and packs the features clip-major, video after video: (row_first[nvid], D)
 *   3. dcf_forward_eval_videos_selected(_h)     one forward on the packed rows of all videos
 *
 * dcf_op_select_clips_videos is the compaction of step 1 alone, dcf_op_gather_clip_rows_videos(_h) makes the rows of step 2 from
 * dense features: the emulation path of callers and tests that hold them.  A model with opt.model.scat is served: step 1 computes
 * the sidekick scores anyway and hands them on (correl_out), step 3 takes them back (correl).
 *
 * Layout: at most DCF_MAX_VIDEOS (16) videos, all padded to the same T; their queries are one flat list in video order, exactly as
 * dcf_forward_eval_videos takes them (NQ = the sum of nq_per_video).  nq_per_video, row_first and every array of pointers are HOST
 * arrays, read before the call returns.
 *
 * Version 1 (csrc/select_videos.hip; the two forwards in csrc/engine.hip).  Conventions are those of decafnet_hip.h: everything on
 * `stream` without a host wait, no atomics and one fixed order of every sum (equal inputs give equal bits), ordinary vector stores,
 * 0 on success and -1 with dcf_last_error() otherwise; a refusal comes before any launch.
 *
 * Not here: the T-sharded and hybrid forwards (dcf_hybrid_phase1 / 2 / 3), the training forward, and the evaluation bank of the fit
 * loop: they keep the dense interface.  HIP-graph replay of the selected forwards, vid_net.stride > 1 and opt.model.sfonly. */
#ifndef DECAFNET_HIP_SELECT_VIDEOS_H
#define DECAFNET_HIP_SELECT_VIDEOS_H

#include <stdint.h>

#include "decafnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCF_SELECT_VIDEOS_EXT_VERSION 1
int dcf_select_videos_ext_version(void);

/* dcf_op_select_clips of decafnet_hip_select.h for nvid videos in ONE launch, workgroup v on the gate rows of video v's queries.
 *   gate (NQ, T) fp32 0 / 1 as dcf_op_gate writes it; vid_masks (nvid, T) bytes; nq_per_video HOST (nvid), every entry >= 1
 *   clips  (nvid, T) int32: row v holds video v's needed clips in ascending order; entries at or beyond counts[v] are not written
 *   pos    (nvid, T) int32, video-local: pos[v, clips[v, i]] = i, and -1 elsewhere
 *   counts (nvid) int32
 * Row v holds exactly what dcf_op_select_clips gives for video v alone (the same device code).  1 <= nvid <= 16, T >= 1. */
int dcf_op_select_clips_videos(const float* gate, const uint8_t* vid_masks, int32_t T, int32_t nvid, const int32_t* nq_per_video,
                               int32_t* clips, int32_t* pos, int32_t* counts, void* stream);

/* dcf_op_gather_clip_rows for nvid videos in one launch: rows[row_first[v] + i, d] = X_cm[v][d * ldx + clips[v, i]] for
 * i < row_first[v + 1] - row_first[v], d < D.  X_cm: HOST array of nvid device pointers to channel-major (D, ldx) matrices, ldx >= T;
 * clips (nvid, T) int32 as dcf_op_select_clips_videos writes it; row_first HOST (nvid + 1), non-decreasing from 0 with at most T rows
 * a video (a video may have none); rows (row_first[nvid], D) of the same element type, fp32 or (_h) IEEE binary16; the bits are
 * copied.  The 64 x 64 tiles of a video start at its own first row.  An index outside [0, ldx) is clamped into it. */
int dcf_op_gather_clip_rows_videos(const float* const* X_cm, int64_t ldx, const int32_t* clips, int32_t T, int32_t nvid,
                                   const int32_t* row_first, int32_t D, float* rows, void* stream);
int dcf_op_gather_clip_rows_videos_h(const uint16_t* const* X_cm, int64_t ldx, const int32_t* clips, int32_t T, int32_t nvid,
                                     const int32_t* row_first, int32_t D, uint16_t* rows, void* stream);

/* The first call of the pattern for a whole forward: the sidekick scores of every video's queries (the scoring kernels of
 * dcf_op_sidekick(_h), one pass over all videos), the block top-k gate (dcf_op_gate's kernel with the model's sn / sratio / msf) and
 * dcf_op_select_clips_videos.
 *   shallow_vid[v] (D, T) fp32 or (_h) binary16, vid_mask[v] (T) bytes, text_cls[v] (nq_per_video[v], D): HOST arrays of pointers
 *   gate_out (NQ, T) fp32; correl_out (NQ, T) fp32 or NULL: the raw scores, which a scat model's second call needs
 *   clips_out, pos_out (nvid, T) int32; counts_out (nvid) int32
 * Scratch comes from the model's feature workspace (it grows on first use: the one case of a host wait).  Refused before any launch:
 * a model that is not finalized, opt.model.sfonly, vid_net.stride > 1, nvid outside 1 .. 16, a query count below 1 or more than
 * 1024 queries in all. */
int dcf_select_videos(dcf_model* m, int32_t nvid, const float* const* shallow_vid, const uint8_t* const* vid_mask, int64_t T,
                      const int32_t* nq_per_video, const float* const* text_cls, float* gate_out, float* correl_out, int32_t* clips_out,
                      int32_t* pos_out, int32_t* counts_out, void* stream);
int dcf_select_videos_h(dcf_model* m, int32_t nvid, const uint16_t* const* shallow_vid, const uint8_t* const* vid_mask, int64_t T,
                        const int32_t* nq_per_video, const float* const* text_cls, float* gate_out, float* correl_out,
                        int32_t* clips_out, int32_t* pos_out, int32_t* counts_out, void* stream);

/* dcf_forward_eval_videos (the same model, text operands and outputs) as an externally gated forward on the selected clips:
 *   vid_rows (row_first[nvid], D) clip-major, 16-byte aligned, D % 4 == 0; video v's rows from row_first[v] on
 *   row_first HOST (nvid + 1): strictly increasing from 0 (every video needs at least one row), at most T rows a video
 *   pos (nvid, T) int32 and gate (NQ, T) fp32 as dcf_select_videos writes them
 *   correl (NQ, T) fp32: required if and only if the model has opt.model.scat, NULL otherwise
 * ONE row-major product P1c = vid_rows . W[:, :D]^T over the rows of all videos (split-operand where the model's gemm_mode and the
 * shapes allow, the fp32 tile GEMM otherwise); vid_map row (q, t) of a query of video v takes row row_first[v] + pos[v, t] of it
 * where gate[q, t] != 0, and w3 * correl[q, t] with scat.  With nvid = 1 and no scat the launches are those of
 * dcf_forward_eval_selected and the outputs the same bits.  The _h form takes binary16 vid_rows and shallow_vid, upcasts both once
 * into the workspace and runs the fp32 form.  Always eager: no HIP graph is captured or replayed.
 * Refused before any launch: opt.model.sfonly, vid_net.stride > 1, several videos with more than 16 queries per chunk
 * (max_batch > 16), a bad row_first, correl on a model without scat or none on one with it. */
int dcf_forward_eval_videos_selected(dcf_model* m, int32_t nvid, const float* vid_rows, const int32_t* row_first, const int32_t* pos,
                                     const float* const* shallow_vid, const uint8_t* const* vid_mask, int64_t T,
                                     const int32_t* nq_per_video, const float* const* text, const uint8_t* const* text_mask,
                                     const int32_t* text_len, const float* gate, const float* correl, float* logits_out,
                                     float* offsets_out, uint8_t* masks_out, void* stream);
int dcf_forward_eval_videos_selected_h(dcf_model* m, int32_t nvid, const uint16_t* vid_rows, const int32_t* row_first,
                                       const int32_t* pos, const uint16_t* const* shallow_vid, const uint8_t* const* vid_mask, int64_t T,
                                       const int32_t* nq_per_video, const float* const* text, const uint8_t* const* text_mask,
                                       const int32_t* text_len, const float* gate, const float* correl, float* logits_out,
                                       float* offsets_out, uint8_t* masks_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DECAFNET_HIP_SELECT_VIDEOS_H */
