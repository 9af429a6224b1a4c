/* decafnet_hip_select.h -- the selected-clip extension of libdecafnet_hip.so.
 *
 * include/decafnet_hip.h is ABI version 12 and frozen, and so are the extension headers beside it.  The top-k gate keeps
 * int(sratio * n) of a video's n blocks of clips, and the expert half of vid_map is used under an open gate only (model.py:531-543:
 * `vid * all_weight` is zero elsewhere).  Every forward of the base ABI still takes the expert features of ALL clips as a dense
 * (D, T) matrix.  This extension is the calling pattern the model was designed for:
 *
 *   1. dcf_op_sidekick(_h) + dcf_op_gate + dcf_op_select_clips   which clips does the model need?  (the caller reads `count` and the
 *                                                                first `count` entries of `clips`: the one host read of the pattern)
 *   2. the caller runs its expert encoder on those clips only and lays the features out clip-major, (count, D)
 *   3. dcf_forward_eval_selected(_h)                             the forward on the compact rows
 *
 * dcf_op_gather_clip_rows(_h) makes the rows of step 2 from dense features: the emulation path of callers and tests that hold them.
 * The operators live in the same shared object and carry a version of their own, dcf_select_ext_version().
 *
 * Version 1 (csrc/select.hip; the two forwards in csrc/engine.hip):
 *   dcf_op_select_clips            the union of the queries' gates over the valid clips as an ascending clip list and its inverse
 *   dcf_op_gather_clip_rows, _h    rows[i, :] = X[:, clips[i]]: channel-major columns to clip-major rows
 *   dcf_forward_eval_selected, _h  dcf_forward_eval_gated with the expert product on the compact rows
 *
 * Conventions are those of decafnet_hip.h: everything on `stream` without a host wait, no atomics and one fixed order of every sum
 * (equal inputs give equal bits), 0 on success and -1 with dcf_last_error() otherwise; a refusal comes before any launch.
 *
 * Not here: several videos per forward, the T-sharded and hybrid forwards (dcf_hybrid_phase1 / 2 / 3), the training forward, and the
 * evaluation bank of the fit loop: they keep the dense interface. */
#ifndef DECAFNET_HIP_SELECT_H
#define DECAFNET_HIP_SELECT_H

#include <stdint.h>

#include "decafnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCF_SELECT_EXT_VERSION 1
int dcf_select_ext_version(void);

/* gate (nq, T) fp32, 0 / 1 exactly as dcf_op_gate writes it; vid_mask (T) bytes, non-zero = valid.  Clip t is NEEDED when vid_mask[t]
 * is set and the gate of at least one query is non-zero at t.
 *   clips   int32, capacity T: the needed clips in ascending order; entries at or beyond *count are not written
 *   pos     (T) int32: pos[clips[i]] = i, and -1 at every clip that is not needed
 *   count   one int32: the number of needed clips
 * Any T >= 1 and nq >= 1.  One workgroup walks T in strips of 4096 clips and carries the running count from strip to strip: a ballot
 * per wave, the waves' counts through LDS, no atomics; all three outputs are written with ordinary vector stores. */
int dcf_op_select_clips(const float* gate, const uint8_t* vid_mask, int32_t T, int32_t nq, int32_t* clips, int32_t* pos, int32_t* count,
                        void* stream);

/* The transposing gather rows[i, d] = X_cm[d * ldx + clips[i]], i < n, d < D: from a channel-major (D, ldx) matrix (ldx >= the clip
 * count T, in elements) to clip-major (n, D) rows of the same element type, fp32 or (_h) IEEE binary16; the bits are copied.  64 x 64
 * tiles through LDS: the reads run along T (coalesced wherever the list is contiguous, which a block gate makes it for `sn` clips at a
 * time), the writes along D.  Any D >= 1, n >= 1; the operands need the alignment of their element type only.  clips holds indices in
 * [0, ldx): an index outside is a caller error and is clamped into that range, so that no read leaves the matrix. */
int dcf_op_gather_clip_rows(const float* X_cm, int64_t ldx, const int32_t* clips, int32_t n, int32_t D, float* rows, void* stream);
int dcf_op_gather_clip_rows_h(const uint16_t* X_cm, int64_t ldx, const int32_t* clips, int32_t n, int32_t D, uint16_t* rows, void* stream);

/* dcf_forward_eval_gated (the same model, text operands, gate (nq, T) and outputs; no sidekick scoring runs, the shallow half of
 * vid_map is computed densely from shallow_vid (D, T)) with the expert features of the selected clips only:
 *   vid_rows (n_rows, D) clip-major, 16-byte aligned; pos (T) int32 as dcf_op_select_clips writes it
 *   P1c (n_rows, E) = vid_rows . W[:, :D]^T   through the row-major GEMM family: split-operand where the model's gemm_mode and the
 *                                              shapes allow, the fp32 tile GEMM otherwise; every row is needed, no tile is skipped
 *   vid_map row (q, t) takes row pos[t] of P1c where gate[q, t] != 0
 * Rows of vid_rows at or beyond n_rows are never read.  pos[t] < 0 under an open gate is a caller error (the selection and the gate do
 * not belong together); it is not detected on the device: that clip then gets no expert half.  modeling.forward_selected takes gate
 * and pos from one Selection and checks their shapes on the host.
 * A non-finite value in vid_rows raises bit 0 of dcf_numerics_status as in the dense forward (f16x3 / bf16x6 modes).
 * The _h form takes binary16 vid_rows and shallow_vid (2-byte aligned), upcasts both once into the engine's workspace and runs the
 * fp32 form: the numbers fp32 operands of the same values give.
 * This forward always runs eagerly: it neither captures nor replays a HIP graph, whatever dcf_model_set_graph_mode says.
 * Refused before any launch: opt.model.scat (the scores are not handed over), opt.model.sfonly (no expert input exists),
 * vid_net.stride > 1 (the gated forward's own limit), n_rows < 1 or n_rows > T. */
int dcf_forward_eval_selected(dcf_model* m, const float* vid_rows, int32_t n_rows, const int32_t* pos, const float* shallow_vid,
                              const uint8_t* vid_mask, int64_t T, int32_t nq, const float* const* text, const uint8_t* const* text_mask,
                              const int32_t* text_len, const float* gate, float* logits_out, float* offsets_out, uint8_t* masks_out,
                              void* stream);
int dcf_forward_eval_selected_h(dcf_model* m, const uint16_t* vid_rows, int32_t n_rows, const int32_t* pos, const uint16_t* shallow_vid,
                                const uint8_t* vid_mask, int64_t T, int32_t nq, const float* const* text, const uint8_t* const* text_mask,
                                const int32_t* text_len, const float* gate, float* logits_out, float* offsets_out, uint8_t* masks_out,
                                void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DECAFNET_HIP_SELECT_H */
