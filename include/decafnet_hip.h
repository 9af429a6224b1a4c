/*
 * libdecafnet_hip.so -- C ABI of the MI355X (gfx950) DeCafNet grounding hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no torch types.  Every entry point
 * names the reference interface it replaces (paths relative to the reference repository).
 * All `const float*` / `uint8_t*` DATA pointers are DEVICE pointers (hipMalloc'ed or
 * torch-ROCm storage) unless a parameter says "host".  `stream` is a hipStream_t passed as
 * void* (NULL = the default stream).  Functions return 0 on success and -1 on failure;
 * dcf_last_error() then holds a message (thread local).
 *
 * There is NO CPU fallback: if the library, the device or a kernel is missing the call fails.
 */
#ifndef DECAFNET_HIP_H
#define DECAFNET_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

const char* dcf_last_error(void);
int dcf_abi_version(void);

/* --------------------------------------------------------------------------------------------
 * Model: replaces PtTransformerEarlyFusionIterative (libs/modeling/model.py:397-565) as built by
 * create_model (libs/worker_v2.py:182-211).  Hyper-parameters mirror opt.model.* (libs/core/opt.py:75-130).
 * ------------------------------------------------------------------------------------------ */
typedef struct dcf_model dcf_model;

typedef struct dcf_config {
  int32_t D;              /* opt.model.vid_net.in_dim: expert / sidekick feature dim               */
  int32_t E;              /* opt.model.vid_net.embd_dim                                            */
  int32_t TE;             /* opt.model.text_net.embd_dim = fusion.text_dim                         */
  int32_t vid_heads;      /* opt.model.vid_net.n_heads                                             */
  int32_t fusion_heads;   /* opt.model.fusion.n_heads                                              */
  int32_t fusion_layers;  /* opt.model.fusion.n_layers                                             */
  int32_t n_embd_convs;   /* opt.model.vid_net.arch[0]                                             */
  int32_t n_stem;         /* opt.model.vid_net.arch[1]                                             */
  int32_t n_levels;       /* opt.model.vid_net.arch[2]  (= number of FPN levels = TCN depth)       */
  int32_t win;            /* opt.model.vid_net.mha_win_size (odd; 0 = global clip attention: a correctness-first fp32
                           * O(T^2) vector-ALU kernel, csrc/attn.hip k_global_attn -- no reference default uses it)  */
  int32_t head_layers;    /* opt.model.cls_head.n_layers (= reg_head.n_layers)                     */
  int32_t sn;             /* opt.model.sn     (clips per scoring block)                            */
  float sratio;           /* opt.model.sratio (fraction of blocks that keep expert features)       */
  int32_t msf;            /* opt.model.msf                                                         */
  int32_t norm;           /* opt.model.norm                                                        */
  int32_t use_abs_pe;     /* opt.model.vid_net.use_abs_pe                                          */
  int32_t max_batch;      /* queries processed together (>= 1); 0 = library default                */
  int32_t gemm_mode;      /* dense-conv arithmetic, all fp32-accurate: 0/16 = f16x3 (two fp16 planes per operand,
                           * 3 MFMA products, default), 6 = bf16x6 (three bf16 planes, 6 products),
                           * 1 = native fp32 MFMA                                                   */
  int32_t model_kind;     /* 0 = PtTransformerEarlyFusionIterative (libs/modeling/model.py:397),
                           * 1 = PtTransformer, late fusion (model.py:30),
                           * 2 = PtTransformerEarlyFusion (model.py:163): kind 0 without the refinement stage    */
  int32_t second_fusion;  /* model_kind 0: also fuse every pyramid level before the heads (model.py:443) */
  /* text_net = TextTransformer (libs/modeling/text_net.py:92-188); text_in = 0 builds the model without it */
  int32_t text_in;        /* opt.model.text_net.in_dim (token feature dim C_t)                     */
  int32_t text_layers;    /* opt.model.text_net.n_layers                                           */
  int32_t text_heads;     /* opt.model.text_net.n_heads                                            */
  int32_t text_abs_pe;    /* opt.model.text_net.use_abs_pe                                         */
  int32_t text_bkgd;      /* opt.model.text_net.use_bkgd_token                                     */
  /* ABI version 3 */
  int32_t scat;           /* opt.model.scat: the clip's raw sidekick score is one more vid_map input channel
                           * (model.py:413-414,550-551; PtTransformer model.py:46-47,128-129)      */
  int32_t sfonly;         /* opt.model.sfonly: with msf, vid_map sees the sidekick features only (model.py:546-547);
                           * D is then the sidekick feature dim = 2 * opt.model.vid_net.in_dim; ignored by model_kind 1 */
  int32_t text_kind;      /* 0 = TextTransformer (text_net.py:92-188), 1 = TextIdentity (text_net.py:22-89: optional embd_fc,
                           * optional AttNPool1D token when text_bkgd != 0; text_layers is ignored)  */
  /* ABI version 5 */
  int32_t xattn_affine;   /* opt.model.fusion.xattn_mode: 0 = 'adaln' (the decoder modulates LayerNorm(q), blocks.py:623-624,643),
                           * 1 = 'affine' (it modulates q itself: nn.Identity, blocks.py:625-626)   */
  /* ABI version 7 */
  int32_t vid_stride;     /* opt.model.vid_net.stride (video_net.py:39,59-74): a power of two; the first log2(stride) embedding
                           * convolutions are k5 / stride 2 / padding 2 and the pyramid starts at T / stride.  0 reads as 1 */
  int32_t pool_only;      /* opt.model.vid_net.pool_only (video_net.py:98-111): a branch layer is one depthwise k3 MaskedConv1D
                           * (vid_net.branch.{i}.conv.weight, stride 1 at level 0, 2 above) instead of a TransformerEncoder */
  /* ABI version 9 */
  int32_t attn_mode;      /* arithmetic of the attention products QK^T / PV on the matrix cores (text->clip cross attention, the
                           * fusion layers' attention half, the encoder's window attention): 0 = f16x3 (two fp16 planes per operand,
                           * three products: the error of an fp32 FMA chain; default), 1 = ONE fp16 product per multiply-add
                           * (11 significant bits per operand, fp32 accumulate -- what BASELINE configs[4] calls "bf16 MFMA
                           * attention", with fp16's three extra bits; opt-in, NOT fp32-accurate: bench.py --attn-mode f16 prints
                           * its delta against the fp32 oracle).  The projections around the products stay f16x3. */
} dcf_config;

int dcf_model_create(const dcf_config* cfg, dcf_model** out);
void dcf_model_destroy(dcf_model* m);

/* Bind one tensor of the reference state_dict by its NAME (the parameter ABI):
 * "vid_map.conv.weight", "fusion.layers.0.xattn.xattn.query.weight", ...  The memory is borrowed
 * (fp32, contiguous, device) and must stay alive until the model is destroyed or re-bound.
 * text_net.* tensors feed dcf_text_encode (ignored when cfg.text_in == 0).
 * Replaces nn.Module.load_state_dict(ckpt['model_ema']) (libs/worker_v2.py:806-812). */
int dcf_model_bind(dcf_model* m, const char* name, const float* data, const int64_t* shape, int32_t ndim);

/* Numerics status of the f16x3 GEMMs (blocking: synchronises `stream`).  Returns a bit set, or -1 on error:
 *   1 = some GEMM accumulator left the finite range since the last reset (an activation beyond the fp16 operand range
 *       |a| < 4094 of the f16x3 mode, or inf/NaN in the inputs): outputs since then are not trustworthy -- re-run with
 *       gemm_mode = 6;   2 = a weight did not fit (|w| >= 255.9) and the model fell back to bf16x6 at finalize;
 *   4 = the model runs bf16x6;  8 = the model runs the native fp32 MFMA path;
 *  16 = a LayerNorm that rides between two kernels as one-pass row statistics (sum, sum of squares) met a row whose mean dwarfs its
 *       spread (mean^2 > 64 (var + eps)): the variance of such a row loses more than ~1e-5 to cancellation -- call
 *       dcf_model_set_ln_carry(m, 0) and repeat the forward (ABI version 9).   reset != 0 clears the sources of 1 and 16. */
int dcf_numerics_status(dcf_model* m, int32_t reset, void* stream);
/* The same status word without blocking: enqueues a 4-byte device -> host copy of the sticky flag (bit 0 above) into
 * `host_dst` (pinned memory) on `stream`; the caller reads it once an event recorded after the call has completed.
 * Independently of either call, a forward that ends with the flag raised overwrites its logits with NaN, so that a plain
 * `model(...)` caller (the reference's Evaluator, libs/worker_v2.py:1007) cannot mistake them for valid scores.
 * (The word copied here is the raw device word: bit 0 = status 1, bit 1 = status 16.) */
int dcf_numerics_status_async(dcf_model* m, int32_t* host_dst, void* stream);
/* on = 0: every LayerNorm of the model runs as its own two-pass launch (blocks.py:125-131: mean, then the mean of squared deviations)
 * instead of riding between kernels as one-pass row statistics; on = 1 (default): carried where the kernels allow.  Drops captured
 * graphs.  What dcf_numerics_status bit 16 asks for.  ABI version 9. */
int dcf_model_set_ln_carry(dcf_model* m, int32_t on);

/* Absolute position encoding buffer `vid_net.pe` (non-persistent in the reference,
 * libs/modeling/video_net.py:75-78): token-major (T, E) fp32 already resampled for length T
 * (video_net.py:141-151).  Borrowed.  Needed only when use_abs_pe != 0. */
int dcf_model_set_pe(dcf_model* m, const float* pe_tokens, int64_t T);

/* Position encoding buffer `text_net.pe` (non-persistent, text_net.py:120-125): token-major (L, TE) fp32,
 * L >= the longest query (already resampled if longer than max_seq_len, text_net.py:172-177).  Borrowed. */
int dcf_model_set_text_pe(dcf_model* m, const float* pe_tokens, int64_t L);

/* Text encoder of one query: replaces model.encode_text(tokens, token_masks) = TextTransformer.forward
 * (libs/modeling/model.py:434-436, text_net.py:158-188; caller libs/worker_v2.py:953).
 *   tokens     : (C_t, Lq) fp32 channel-major = tensor[0] of the reference's (1, C_t, Lq) input
 *   token_mask : (Lq) bytes, 1 = valid token; NULL = all valid
 *   text_out   : (TE, Lk) fp32 channel-major, Lk = Lq + use_bkgd_token  (the layout dcf_forward_eval takes)
 *   mask_out   : (Lk) bytes = cat(mask[:1], mask) */
int dcf_text_encode(dcf_model* m, const float* tokens, const uint8_t* token_mask, int32_t Lq, float* text_out,
                    uint8_t* mask_out, void* stream);

/* Validate that every parameter is bound and repack convolution weights for the kernels. */
int dcf_model_finalize(dcf_model* m, void* stream);

/* Number of points per query, sum_l T / 2^l. */
int64_t dcf_points_per_query(const dcf_model* m, int64_t T);

/* Eval forward: replaces model(vid, shallow_vid, vid_masks, text, text_cls, text_masks, eval=True)
 * (libs/modeling/model.py:473-565; caller libs/worker_v2.py:1007).
 *   vid, shallow_vid : (D, T) fp32 channel-major = tensor[0] of the reference's (1, D, T) inputs
 *   vid_mask         : (T) bytes (torch.bool storage), 1 = valid clip
 *   text[q]          : HOST array of nq device pointers, each (TE, text_len[q]) fp32 = encode_text()[0][0]
 *   text_mask[q]     : HOST array of nq device pointers, each (text_len[q]) bytes; entries may be NULL (= all valid)
 *   text_len         : HOST array of nq ints
 *   text_cls         : (nq, D) fp32
 * Outputs (device, caller allocated), S = dcf_points_per_query(T), levels concatenated l = 0..L-1:
 *   logits_out (nq, S) raw fp32 logits;  offsets_out (nq, S, 2) fp32 >= 0;  masks_out (nq, S) bytes. */
int dcf_forward_eval(dcf_model* m, const float* vid, const float* shallow_vid, const uint8_t* vid_mask, int64_t T,
                     int32_t nq, const float* const* text, const uint8_t* const* text_mask, const int32_t* text_len,
                     const float* text_cls, float* logits_out, float* offsets_out, uint8_t* masks_out, void* stream);

/* Same forward on a WINDOW of a longer video (T-sharding across GPUs): the 0/1 clip gate
 * (nq, T) fp32 is supplied by the caller, who selected the top-k blocks on the all-gathered sidekick scores
 * of the whole video; the position encoding set by dcf_model_set_pe must be the window's slice of the
 * whole video's encoding.  No scoring, no text_cls. */
int dcf_forward_eval_gated(dcf_model* m, const float* vid, const float* shallow_vid, const uint8_t* vid_mask, int64_t T,
                           int32_t nq, const float* const* text, const uint8_t* const* text_mask, const int32_t* text_len,
                           const float* gate, float* logits_out, float* offsets_out, uint8_t* masks_out, void* stream);

/* Training-mode forward, forward values only (PtTransformerEarlyFusionIterative._drop_forward, libs/modeling/model.py:567-632,
 * with every dropout / drop-path probability 0): a batch of videos of one padded length, video v repeated for its
 * text_size[v] = nq_per_video[v] queries (`repeat_interleave`, model.py:579-582), i.e. the rows of the batch are the
 * (video, query) pairs in video order.  Arguments as dcf_forward_eval_videos; returns, per pair, what fuse_and_predict
 * returns (model.py:442-471): logits1_out (sum(nq), S) of the first cls_head, logits2_out (sum(nq), S), offsets_out
 * (sum(nq), S, 2), masks_out (sum(nq), S).  No backward pass.  ABI version 5. */
int dcf_forward_train_videos(dcf_model* m, int32_t nvid, const float* const* vid, const float* const* shallow_vid,
                             const uint8_t* const* vid_mask, int64_t T, const int32_t* nq_per_video, const float* const* text,
                             const uint8_t* const* text_mask, const int32_t* text_len, const float* const* text_cls,
                             float* logits1_out, float* logits2_out, float* offsets_out, uint8_t* masks_out, void* stream);

/* Dropout and drop-path of the training forward (ABI version 11).  Read by dcf_forward_train_videos only: the evaluation,
 * hybrid and dcf_op_* entry points never see this state.  Rates: vid_net.proj_pdrop / path_pdrop (stem and branch encoders),
 * fusion.proj_pdrop / path_pdrop (the early-fusion decoders), the Dropout of every refinement TCN layer (tcn.py:27).  Each
 * rate must lie in [0, 1); all zero = inactive (the deterministic forward of every probability 0).  While active the forward
 * takes the unfused kernel sequence and launches eagerly (the seed is a kernel argument, never a captured graph).
 *
 * The random stream (the masks are NOT torch's draws, torch's stream is not reproducible outside torch; their distribution
 * is the reference's):
 *   Philox4x32-10, multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85;
 *   key = (seed & 0xffffffff, seed >> 32); counter = (j & 0xffffffff, j >> 32, site, 0), j = e >> 2; element e takes word e & 3;
 *   u = (word >> 8) * 2^-24; an element is kept iff u >= p (p as fp32); kept values are multiplied by 1.0f / (1.0f - p).
 *   e = index in the reference's layout: dropout on the (B', C, T_l) tensor e = (b * C + c) * T_l + t, b the (video, query)
 *       row in repeat_interleave order (model.py:579-582), T_l the padded length of the level; drop-path (per sample) e = b.
 *   site = group << 16 | layer << 4 | sub: group 1 fusion.layers[i], 2 vid_net.stem[i], 3 vid_net.branch[i], 4 refine.layers[i];
 *       sub 0 attention proj_drop (blocks.py:392; the decoder's acts on the (B', 2E, T) scale / shift tensor, c < E scale),
 *       1 FFN dropout after the GELU, 2 FFN dropout after ffn.proj (blocks.py:535-538), 3 drop_path_attn, 4 drop_path_ffn,
 *       5 the TCN layer's dropout (tcn.py:27). */
int dcf_model_set_dropout(dcf_model* m, float vid_proj_p, float vid_path_p, float fus_proj_p, float fus_path_p, float refine_p,
                          int64_t seed);
/* Test aid: the keep bits (1 = kept) of elements e0 .. e0 + n - 1 of `site` under `seed` and rate p -> out (n bytes, device).
 * ABI version 11. */
int dcf_debug_dropout_keep(int64_t seed, int32_t site, int64_t e0, int64_t n, float p, uint8_t* out, void* stream);

/* Point losses, forward values (libs/modeling/loss.py; used by Trainer.forward_backward, libs/worker_v2.py:441-461).
 *   dcf_sigmoid_focal_loss <- sigmoid_focal_loss(inputs, targets, alpha, gamma, smoothing, reduction)   (loss.py:5-57)
 *   dcf_ctr_iou_loss       <- ctr_giou_loss / ctr_diou_loss(input_offsets, target_offsets, reduction, eps) (loss.py:60-166)
 * n elements (rows of 2 offsets for the IoU losses) on the device; `select` (optional, n bytes) keeps the elements with a
 * non-zero byte -- the boolean-mask indexing `x[fpn_masks]` / `x[pos_masks]` of the caller without a compaction pass.
 * elem_out (optional, n floats): the per-element loss (reduction 'none'; unselected elements get 0); sum_out (optional,
 * 1 float) the sum over the selected elements and count_out (optional, 1 int32) their number ('sum' / 'mean'), added up
 * in a fixed order (deterministic).  kind: 0 = GIoU (reduces to IoU, loss.py:104), 1 = DIoU. */
int dcf_sigmoid_focal_loss(const float* inputs, const float* targets, const uint8_t* select, int64_t n, float alpha, float gamma,
                           int32_t smoothing, float* elem_out, float* sum_out, int32_t* count_out, void* stream);
int dcf_ctr_iou_loss(const float* input_offsets, const float* target_offsets, const uint8_t* select, int64_t n, int32_t kind,
                     float eps, float* elem_out, float* sum_out, int32_t* count_out, void* stream);

/* Point annotation and the Trainer's objective on the packed (B', S) outputs of dcf_forward_train_videos (ABI version 12).  No
 * backward pass.  The candidate points are not an argument: point i of a row follows from (T, L) and the parameters of
 * PtGenerator (libs/modeling/model.py:668-743) -- level l holds T >> l points of stride 2^l at (i - first_l) * 2^l
 * (+ 2^l - 0.5 with use_offset: the reference adds 0.5 * 2^l in place on a strided view of one tic array, model.py:710-712, so
 * level l carries the shifts of the levels below it too), with the regression range of model.py:686-696 built from regression_range, sigma and
 * max_seq_len as PtGenerator.__init__ builds it.  1 <= L <= 16, T a multiple of 2^(L-1), T <= max_seq_len, T < 2^23.
 * targets (nrows, 2): the segments, already divided by vid_stride.  center_sampling: 1 = 'radius' (within `radius` strides of
 * the segment centre), 0 = anything else (inside the segment).
 *   dcf_annotate_points <- annotate_points_per_video per target (libs/worker_v2.py:93-133) = Trainer._annotate_points
 *     (:575-637): labels_out (nrows, S) bytes, offsets_out (nrows, S, 2), optionally the two predicates the function returns
 *     third (in_window_out, in_range_out: (nrows, S) bytes).  Bit-equal to the reference.
 *   dcf_point_objective <- Trainer._microbatch_forward_backward after the model call (:441-476), without the backward:
 *     pos = labels & masks, norm = pos.sum(), calc_focal_loss (:85-87, label l * (1 - smoothing) + smoothing / 2, gamma 2) of
 *     both heads over masks, calc_iou_loss (:89-91; iou_kind 0 GIoU, 1 DIoU) over pos, each / loss_norm * world_size,
 *     cls = (cls1 + cls2) / 2, total = cls + loss_weight * reg.  Labels and ground-truth offsets are formed in registers and
 *     never written.  logits1 may be NULL (one classification head: cls = cls2, Evaluator._calc_loss :1029-1061).
 *     loss_norm_dev: one float on the device (the Trainer's running loss_norm), read by the kernel so that the host never waits.
 *     rows_out (optional, (nrows, 4)): per row (focal1_sum, focal2_sum, iou_sum, n_pos), focal over masks, iou over
 *     labels & masks.  out4 (optional, 4 floats): cls, reg, total, norm.  Sums are taken in a fixed order that depends on
 *     (nrows, S) alone (deterministic); the only allocation is stream-ordered scratch sized from (nrows, S). */
int dcf_annotate_points(const float* targets, int32_t nrows, int64_t T, int32_t L, double regression_range, double sigma, int32_t use_offset,
                        int64_t max_seq_len, int32_t center_sampling, double radius, uint8_t* labels_out, float* offsets_out,
                        uint8_t* in_window_out, uint8_t* in_range_out, void* stream);
int dcf_point_objective(const float* logits1, const float* logits2, const float* offsets, const uint8_t* masks, const float* targets,
                        int32_t nrows, int64_t T, int32_t L, double regression_range, double sigma, int32_t use_offset, int64_t max_seq_len,
                        int32_t center_sampling, double radius, float alpha, double smoothing, int32_t iou_kind, float eps,
                        const float* loss_norm_dev, float world_size, float loss_weight, float* rows_out, float* out4, void* stream);

/* Gradients of the point losses and of the Trainer's objective: `total_loss.backward()` (libs/worker_v2.py:467-468) cut at the
 * three tensors the training forward returns.  Nothing below those outputs is differentiated here.  Additions to ABI version 12.
 *
 * Sub-gradient convention.  The reference wraps its losses in torch.jit.script, and its scripted gradient is not a stable
 * function at the non-smooth points (ctr_diou_loss, reduction 'sum', gradient with respect to pred):
 *
 *   pred, gt                                  scripted reference                        same body, eager autograd
 *   [2,3], [2,3] (both min / max tie)         [0.2, 0.2]                                [0, 0]
 *   [0,1], [0,2] (left tie)                   [0.375, -0.625]                           [-0.03125, -0.625]
 *   [0,0], [0,0] (union under eps)            first call [-5e7, -5e7], later [0, 0]     [-5e7, -5e7]
 *   [0,0], [1,2]; any tie-free pair           equal                                     equal
 *
 * These kernels follow eager PyTorch autograd (derivatives.yaml): minimum / maximum give each argument half the gradient at
 * a == b; clamp(min=eps) passes the gradient where x >= eps and blocks it below; `targets >= 0.5` and the label rule carry no
 * gradient.  Away from ties and clamp edges this is what the scripted reference computes as well.
 *
 *   dcf_sigmoid_focal_loss_grad <- d sigmoid_focal_loss / d inputs (loss.py:5-57; every alpha, gamma, smoothing)
 *   dcf_ctr_iou_loss_grad       <- d ctr_giou_loss / d input_offsets (loss.py:60-109, kind 0), d ctr_diou_loss (:111-166, kind 1)
 *     grad_out (n floats / n x 2 floats) is overwritten; unselected elements get 0.  The upstream gradient is grad_elem
 *     (n floats, reduction 'none') or *grad_scalar (one device float, 'sum' / 'mean'; NULL = 1), not both.  count_dev
 *     (optional, one device int32, the count_out of the forward call): reduction 'mean' -- the gradient is divided by it on the
 *     device, and a count of 0 gives zeros (`0.0 * loss.sum()`, loss.py:105,164).
 *   dcf_point_objective_grad <- the backward of what dcf_point_objective computes, arguments as there:
 *       g_logits_h = focal'(x_h, t) * world_size / loss_norm / n_heads * (grad_total + grad_cls)            on masks, 0 elsewhere
 *       g_offsets  = iou'(pred, gt) * world_size / loss_norm * (loss_weight * grad_total + grad_reg)        on labels & masks, 0 elsewhere
 *     grad_total_dev: one device float, the upstream gradient of `total` (NULL = 1).  grad_parts_dev: two device floats, the
 *     upstream gradients of `cls` and `reg` taken on their own (NULL = 0, 0).  g_logits1 is NULL exactly when logits1 is.
 *     accumulate != 0 adds into the g_* buffers instead of overwriting them (micro-batches, worker_v2.py:366-376).  rows_out /
 *     out4 (both optional): when either is given the same pass also produces the values of dcf_point_objective, bit-equal to
 *     that call.  One elementwise launch for the gradient: no atomics, no scratch, no host wait, deterministic. */
int dcf_sigmoid_focal_loss_grad(const float* inputs, const float* targets, const uint8_t* select, int64_t n, float alpha, float gamma,
                                int32_t smoothing, const float* grad_elem, const float* grad_scalar, const int32_t* count_dev,
                                float* grad_out, void* stream);
int dcf_ctr_iou_loss_grad(const float* input_offsets, const float* target_offsets, const uint8_t* select, int64_t n, int32_t kind,
                          float eps, const float* grad_elem, const float* grad_scalar, const int32_t* count_dev, float* grad_out,
                          void* stream);
int dcf_point_objective_grad(const float* logits1, const float* logits2, const float* offsets, const uint8_t* masks, const float* targets,
                             int32_t nrows, int64_t T, int32_t L, double regression_range, double sigma, int32_t use_offset, int64_t max_seq_len,
                             int32_t center_sampling, double radius, float alpha, double smoothing, int32_t iou_kind, float eps,
                             const float* loss_norm_dev, float world_size, float loss_weight, const float* grad_total_dev,
                             const float* grad_parts_dev, float* g_logits1, float* g_logits2, float* g_offsets, int32_t accumulate,
                             float* rows_out, float* out4, void* stream);

/* Throughput extension: several videos of the SAME padded length T in one forward (the reference evaluates one video per
 * call, model.py:496; videos no longer than opt.model.max_vid_len are all padded to that length, worker_v2.py:969-976).
 * Video v has nq_per_video[v] queries; text / text_mask / text_len and the outputs list the queries of all videos in
 * video order (sum(nq) entries, outputs (sum(nq), S) ...); text_cls[v] is (nq_per_video[v], D).  After vid_map every
 * kernel works on rows [query][t], so the result of each query is the one dcf_forward_eval gives for its video alone.
 * 1 <= nvid <= 16; with nvid > 1 max_batch must be <= 16.  ABI version 3. */
int dcf_forward_eval_videos(dcf_model* m, int32_t nvid, const float* const* vid, const float* const* shallow_vid,
                            const uint8_t* const* vid_mask, int64_t T, const int32_t* nq_per_video, const float* const* text,
                            const uint8_t* const* text_mask, const int32_t* text_len, const float* const* text_cls,
                            float* logits_out, float* offsets_out, uint8_t* masks_out, void* stream);

/* Debug taps for parity tests.  what 0 / 1 / 4 copy an intermediate of the LAST forward chunk into `dst` (device) now:
 *   0 = sidekick scores (nq, T); 1 = gate (B, T); 4 = pyramid features (B*S rows [level][b][t], E+32).
 * what 2 / 3 ARM a one-shot tap: the NEXT forward (run eagerly, no graph) copies 2 = the vid_map output / 3 = the fusion
 * output (B*T, E) token-major of its last query chunk into `dst` and disarms the tap; `dst` must stay alive until then and
 * hold max_floats >= B*T*E floats (checked by that forward). */
int dcf_debug_copy(dcf_model* m, int32_t what, float* dst, int64_t max_floats, void* stream);

/* One long video with few queries, T-sharded over ranks WITHOUT recomputing the top of the pyramid (extension; the reference's eval is
 * single-GPU, libs/worker_v2.py:922-924).  The pyramid is cut at level k: a rank runs levels 0..k on a NARROW window of Tn clips and levels
 * k+1..L-1 on a COARSE window of Tc level-k rows taken from the all-gathered level-k feature map; the refinement TCN (model.py:449-458)
 * couples the levels, hence a second exchange (the refined level-k map).  cvpr2025-decafnet_amd/dist.py `hybrid_plan` / `hybrid_forward`
 * derive the windows and run the collectives; windows are treated as sequences, their halos absorb the ends.  ABI version 8.
 *   phase 1: vid_map, early fusion, embedding, levels 0..k on the narrow window with the caller's gate (as dcf_forward_eval_gated; set the
 *            window's position-encoding slice with dcf_model_set_pe first) -> featk_out (nq, Tn >> k, E)
 *   phase 2: featk_c (nq, Tc, E) / maskk_c (Tc): the gathered level-k features and level-k validity on the coarse window; off_k = first
 *            level-k row of the narrow window inside the coarse one -> refk_out (nq, Tn >> k, 32): the refined map at level k
 *   phase 3: refk_c (nq, Tc, 32): the gathered refined map on the coarse window -> outputs of levels 0..k on the narrow window
 *            (logits_n (nq, Sn), offsets_n (nq, Sn, 2), masks_n (nq, Sn), Sn = sum_{l<=k} Tn >> l) and of levels k+1.. on the coarse one
 *            (.._c, Sc = sum_{j>=1} Tc >> j), levels concatenated as in dcf_forward_eval.
 * Any other forward on the model between the phases invalidates them (they share its workspace). */
int dcf_hybrid_phase1(dcf_model* m, int32_t k, const float* vid_w, const float* shallow_w, const uint8_t* mask_w, int64_t Tn, int64_t Tc,
                      int32_t nq, const float* const* text, const uint8_t* const* text_mask, const int32_t* text_len, const float* gate_w,
                      float* featk_out, void* stream);
int dcf_hybrid_phase2(dcf_model* m, const float* featk_c, const uint8_t* maskk_c, int64_t off_k, float* refk_out, void* stream);
int dcf_hybrid_phase3(dcf_model* m, const float* refk_c, float* logits_n, float* offsets_n, uint8_t* masks_n, float* logits_c,
                      float* offsets_c, uint8_t* masks_c, void* stream);

/* How the last dcf_forward_eval* call on this model was issued: 0 = eager kernel launches, 1 = replay of the captured HIP
 * graph, 2 = the call that captured the graph (and launched it).  A forward called on the NULL (legacy default) stream,
 * which cannot be captured, runs on an engine-owned stream ordered after / before the caller's by events.  ABI version 4. */
int dcf_graph_active(const dcf_model* m);
/* HIP-graph policy of the repeated forward: 0 = auto (replay for forwards of >= 65536 level-0 rows, i.e. batched queries /
 * videos; eager launches for the one-video-per-call pattern, which measures 5 % faster that way), 1 = always capture and
 * replay, 2 = never.  The environment variable DCF_NO_GRAPH=1 disables graphs whatever the mode.  ABI version 5. */
int dcf_model_set_graph_mode(dcf_model* m, int32_t mode);
/* Test / developer switch (process wide): override a built-in dispatch threshold so that the operator tests can send small
 * reference fixtures through the kernels the engine only picks for large grids.  Names: "dec_chain_min_rows" (level-0 rows from
 * which the attention half of a fusion layer runs as one kernel, csrc/dec_chain.hip), "enc_chain_min_rows" / "enc_attn_min_rows" (the same for
 * the two halves of the encoder layers' attention, csrc/enc_chain.hip), "fuse_scores" (0: the sidekick scores by their own kernels instead
 * of on the shallow vid_map GEMM), "tcn_frag" (0: every workgroup of a TCN layer builds its weight fragments itself instead of reading the
 * per-model image).  value < 0 restores the built-in value.  Not a reference interface; results do not depend on it beyond
 * rounding.  ABI version 6 (the last two names: 8). */
int dcf_debug_set_option(const char* name, int32_t value);
/* Measurement aid (not a reference interface): the matrix rate THIS device sustains.  Runs bare fp16 MFMA loops (shape 0:
 * v_mfma_f32_32x32x16_f16, shape 1: v_mfma_f32_16x16x32_f16; operands in registers, one wave per SIMD, one workgroup per CU,
 * mfmas_per_wave MFMAs per wave, a few launches back to back on the NULL stream, synchronous) and returns the CU count and the
 * nanoseconds one MFMA occupies a SIMD for.  Nominal: 32 (16) cycles at 2.4 GHz = 13.3 (6.7) ns; under load the part holds
 * 1.5 - 1.75 GHz, which bounds every kernel of the dense family below ~0.7 of the nominal peak the roofline prices against.
 * bench.py reports it as roofline.checks.mfma_sustained.  ABI version 10. */
int dcf_calib_mfma_rate(int32_t shape, int32_t mfmas_per_wave, int32_t* n_cus, float* ns_per_mfma);

/* --------------------------------------------------------------------------------------------
 * Proposal decoding: replaces Evaluator._collect_segments (libs/worker_v2.py:1131-1187).
 *   logits (nq, S), offsets (nq, S, 2), masks (nq, S) as produced by dcf_forward_eval.
 *   segs_out (nq, pre_nms_topk, 2), scores_out (nq, pre_nms_topk), counts_out (nq) int32 (device).
 * ------------------------------------------------------------------------------------------ */
int dcf_collect_segments(const float* logits, const float* offsets, const uint8_t* masks, int32_t nq, int64_t T,
                         int32_t n_levels, float pre_nms_thresh, int32_t pre_nms_topk, float seg_len_thresh,
                         float* segs_out, float* scores_out, int32_t* counts_out, void* stream);

/* The same with the optional external per-clip scores of _collect_segments (worker_v2.py:1137,1150-1156):
 * ext_scores (nq, T) fp32 device or NULL; they multiply sigmoid(logits) level by level after a k3/s2/p1 max-pool
 * per level.  ABI version 3. */
int dcf_collect_segments_ext(const float* logits, const float* offsets, const uint8_t* masks, const float* ext_scores,
                             int32_t nq, int64_t T, int32_t n_levels, float pre_nms_thresh, int32_t pre_nms_topk,
                             float seg_len_thresh, float* segs_out, float* scores_out, int32_t* counts_out, void* stream);

/* --------------------------------------------------------------------------------------------
 * NMS: replaces the extension module nms_1d_cpu_vg (libs/nms/src/nms_cpu.cpp:184-194).
 * Batched over nq independent problems laid out with a fixed `stride` (entries) per problem;
 * counts (device int32, may be NULL => every problem has n_max entries).  n_max <= 4096.
 *   dcf_nms_1d      <- nms_1d(segs, scores, iou_thresh)                       (nms_cpu.cpp:20-70)
 *   dcf_softnms_1d  <- softnms_1d(segs, scores, dets, iou_thresh, sigma, min_score, method) (:72-181)
 *   max_iters = 0 reproduces the reference (all picks); k > 0 stops after k picks (the only
 *   ones SoftNMSop keeps when max_num_segs = k, libs/nms/nms.py:54-59).
 * ------------------------------------------------------------------------------------------ */
int dcf_nms_1d(const float* segs, const float* scores, const int32_t* counts, int32_t nq, int32_t n_max,
               int32_t stride, float iou_thresh, int64_t* keep_out, int32_t* keep_counts_out, void* stream);
int dcf_softnms_1d(const float* segs, const float* scores, const int32_t* counts, int32_t nq, int32_t n_max,
                   int32_t stride, float iou_thresh, float sigma, float min_score, int32_t method,
                   int32_t max_iters, float* dets_out, int64_t* inds_out, int32_t* out_counts, void* stream);
/* segment_voting (libs/nms/nms.py:64-103). nms_segs rows have `nms_ld` floats (2, or 3 for dets). */
int dcf_segment_voting(const float* nms_segs, int32_t nms_ld, const int32_t* n1_counts, int32_t n1_max,
                       int32_t n1_stride, const float* all_segs, const float* all_scores,
                       const int32_t* n2_counts, int32_t n2_max, int32_t n2_stride, float iou_thresh,
                       int32_t nq, float* out, void* stream);

/* --------------------------------------------------------------------------------------------
 * Measurement aid: when enabled, every kernel launch of the library is bracketed by HIP events on
 * its own stream.  dcf_profile_report writes a JSON object {kernel: {count, ms, flops, bytes}} (flops
 * and bytes are the ALGORITHMIC work of the launches) into buf and returns the required size.
 * ------------------------------------------------------------------------------------------ */
int dcf_profile_enable(int32_t on);
int64_t dcf_profile_report(char* buf, int64_t cap);

/* --------------------------------------------------------------------------------------------
 * Single-operator entry points (used by the parity tests and micro-benchmarks).
 * ------------------------------------------------------------------------------------------ */
/* C[M][N] = act(A[M][K] * W[N][K]^T + bias): nn.Conv1d(k=1) on token-major activations.
 * act: 0 none, 1 exact GELU, 2 ReLU. */
int dcf_op_linear(const float* A, const float* W, const float* bias, float* C, int32_t M, int32_t N, int32_t K,
                  int32_t act, void* stream);
/* same through the split-operand MFMA GEMM (gemm_bf16s.hip); nterms = 16 (f16x3, the forward's default) or 6 (bf16x6).
 * Operand envelope of f16x3 (planes scaled by 2^4 / 2^8): 22-bit operands for 2^-7 <= |a| < 4094 and 2^-11 <= |w| < 255.9; below that
 * an absolute representation floor of 2^-29 (a) / 2^-33 (w), fp16 subnormals kept; beyond it non-finite results and the sticky
 * numerics word where the caller has one.  bf16x6 has fp32's exponent range and commutes with a power of two on A bit for bit.
 * Pinned by tests/test_operand_range_cpu.py (the numbers) and tests/test_gpu_operand_range.py (the kernels). */
int dcf_op_linear_split(const float* A, const float* W, const float* bias, float* C, int32_t M, int32_t N, int32_t K,
                        int32_t act, int32_t nterms, void* stream);
/* same with A given channel-major (K, M) -- the reference's (C, T) layout */
int dcf_op_linear_cm(const float* A_cm, const float* W, const float* bias, float* C, int32_t M, int32_t N, int32_t K,
                     void* stream);
/* Y = LayerNorm_channels(A W^T + bias) * ln_w + ln_b [ReLU], the normalisation fused into the GEMM epilogue (how the
 * head trunks run: MaskedConv1D -> LayerNorm -> ReLU, libs/modeling/head.py:53-64); C (optional, may be NULL) receives
 * the raw product.  Only shapes the engine fuses: N = 256, M >= 28672, K % 32 == 0. */
int dcf_op_linear_ln(const float* A, const float* W, const float* bias, const float* ln_w, const float* ln_b, float* C, float* Y,
                     int32_t M, int32_t N, int32_t K, int32_t relu, int32_t nterms, void* stream);

/* Two chained 1x1 convolutions with a channel LayerNorm between them, the LayerNorm carried as row statistics instead of a
 * pass over the rows (how attn.proj -> ln_ffn -> ffn.fc runs, libs/modeling/blocks.py:586-590):
 *   X = A W1^T + b1 (+ R)            written with (sum, sum of squares) of every row on the side
 *   Y = act(LayerNorm(X) W2^T + b2)  computed from the RAW X with ln_w folded into W2 and (mean, rstd) applied in the epilogue
 * act = erf GELU if gelu != 0.  Shapes the engine carries: N1 % 64 == 0, tile-kernel grids (M * N / 4096 > 256). */
int dcf_op_linear_ln_carry(const float* A, const float* W1, const float* b1, const float* R, const float* ln_w, const float* ln_b,
                           const float* W2, const float* b2, float* X, float* Y, int32_t M, int32_t N1, int32_t K1, int32_t N2,
                           int32_t gelu, int32_t nterms, void* stream);

/* The FFN half of a transformer block (libs/modeling/blocks.py:535-538 with the residual of :589-590):
 *   C = X + ls * ((GELU(LN(X) W1^T + b1) W2^T + b2) * mask),   W1 (4E, E), W2 (E, 4E), hidden width 4E
 * ln_w / ln_b NULL = no LayerNorm in front; ls NULL = 1; mask NULL = all rows valid; stats_out (optional, (M, E / 64, 2)):
 * (sum, sum of squares) of every row written to C.  f16x3 operand split.  chain = 0: two GEMMs with the hidden activations in
 * memory; chain = 1 (E = 256 only): one kernel, the hidden activations stay in registers (csrc/ffn_chain.hip: the default kernel;
 * chain = 2: its four-wave form, chain = 3: its eight-wave producer / consumer form -- bit-identical results).  C must not alias X.  With a LayerNorm
 * in front the one-kernel form carries it as one-pass row statistics; if a row turns out ill-conditioned for that (dcf_numerics_status
 * bit 16) the call repeats itself with the LayerNorm as its own two-pass launch, as the engine does after dcf_model_set_ln_carry(m, 0). */
int dcf_op_ffn(const float* X, const float* ln_w, const float* ln_b, const float* W1, const float* b1, const float* W2, const float* b2,
               const float* ls, const uint8_t* mask, float* C, float* stats_out, int32_t M, int32_t E, int32_t chain, void* stream);

/* same product on the split-operand matrix-core path (how vid_map runs); needs M % 4 == 0, N % 128 == 0, K % 32 == 0.  The operand
 * envelope of dcf_op_linear_split (activation scale 2^4).  Inside the forward this product runs on UNSCALED planes of the raw
 * features: |feature| < 65504, 22 bits from 2^-3 on, an absolute floor of 2^-25 below (the input envelope). */
int dcf_op_linear_cm_split(const float* A_cm, const float* W, const float* bias, float* C, int32_t M, int32_t N, int32_t K,
                           int32_t nterms, void* stream);
/* A prediction head (libs/modeling/head.py:53-64 ClsHead, :95-103 RegHead) on B sequences of T token-major rows (B*T, C):
 *   x = relu(LayerNorm(MaskedConv1D_k3(x, mask)))  twice (W1 / ln1, W2 / ln2: PyTorch (C, C, 3) weights, no bias), then
 *   out (B*T, NO) = MaskedConv1D_k3(x, mask) with Wout (NO, C, 3) and bout; scale != 0: relu(scale * out) (RegHead's Scale + ReLU).
 * f16x3 operand split.  chain = 0: GEMM, LayerNorm and output-convolution launches with the trunk activations in memory;
 * chain = 1 (C = 256 / 288): one kernel, the trunk activations stay in registers (csrc/head_chain.hip). */
int dcf_op_head(const float* X, const uint8_t* mask, const float* W1, const float* ln1_w, const float* ln1_b, const float* W2,
                const float* ln2_w, const float* ln2_b, const float* Wout, const float* bout, float* out, int32_t B, int32_t T,
                int32_t C, int32_t NO, float scale, int32_t chain, void* stream);

/* MaskedConv1D(k=3, pad=1, no bias) on token-major (B*T, Cin) rows; W is the PyTorch (N, Cin, 3) weight. */
int dcf_op_conv3(const float* X, const uint8_t* mask, const float* W_ock, float* Y, int32_t B, int32_t T, int32_t Cin,
                 int32_t N, void* stream);
/* the same convolution on the split-operand matrix-core path the forward uses (nterms 16 = f16x3, 6 = bf16x6); Cin % 32 == 0.
 * The operand envelope of dcf_op_linear_split.  ABI version 4. */
int dcf_op_conv3_split(const float* X, const uint8_t* mask, const float* W_ock, float* Y, int32_t B, int32_t T, int32_t Cin,
                       int32_t N, int32_t nterms, void* stream);
/* channel LayerNorm (libs/modeling/blocks.py:125-131) per row; w/b may be NULL. */
int dcf_op_layernorm(const float* X, const float* w, const float* b, float* Y, int32_t rows, int32_t C, int32_t relu,
                     void* stream);
/* Backward of the two operators above (additions to ABI version 12): MaskedConv1D, dense, k = 1 / 3, padding (k - 1) / 2, and the
 * channel LayerNorm, on token-major rows.  They differentiate
 *   Y[b,t,n] = bias[n] + sum_j sum_c W[n,c,j] m[b,t+j-p] X[b,t+j-p,c]      (libs/modeling/blocks.py:87-106: `self.conv(x * mask_float)`;
 *                                                                           taps stay inside sequence b, Y is not masked)
 *   out = [relu] (LayerNorm(X) * w + b)                                     (blocks.py:125-131, two-pass, eps = 1e-5; the ReLU of
 *                                                                           head.py:58 / :100 passes the gradient where out > 0)
 *   dcf_op_conv_bwd_data   : dX[b,t,c] = m[b,t] sum_j sum_n dY[b,t-j+p,n] W[n,c,j]          (what autograd leaves in x.grad)
 *   dcf_op_conv_bwd_weight : dW[n,c,j] = sum_{b,t} dY[b,t,n] m X[b,t+j-p,c],  db[n] = sum_{b,t} dY[b,t,n]   (conv.weight.grad, conv.bias.grad)
 *   dcf_op_layernorm_bwd   : dX, dw[c] = sum_rows dy xhat, db[c] = sum_rows dy, dy = dOut where the ReLU passes
 * W_ock / dW_ock: PyTorch's (N, Cin, k) layout.  mask (B*T bytes) NULL = every row valid.  Cin % 32 == 0; N % 32 == 0 (f16x3 on the
 * matrix cores, the arithmetic of the forward) or N = 1, 2 (vector ALU: the heads' output convolutions); C % 32 == 0, C <= 1024;
 * anything else fails with a message.  accumulate != 0 adds into dW / db / dw (`.grad +=`), otherwise they are overwritten; db, dw
 * may be NULL.  dY is not assumed to be masked: a non-zero dY at a padded row is used.
 * The fp16 planes take dY times a power of two chosen on the device from max |dY| (no host wait); sums run over fixed row slices
 * in a fixed order without floating-point atomics, so results are bit-identical from run to run and scaling dY by a power of two
 * scales them by exactly that.  If a sum comes out non-finite (inf / NaN operands, |X| >= 4094, |W| >= 255.9) the outputs hold the
 * non-finite values and the NEXT call of one of these three functions returns -1 once, with a message; nothing falls back to
 * another arithmetic. */
int dcf_op_conv_bwd_data(const float* dY, const uint8_t* mask, const float* W_ock, float* dX, int32_t B, int32_t T, int32_t Cin,
                         int32_t N, int32_t k, void* stream);
int dcf_op_conv_bwd_weight(const float* X, const uint8_t* mask, const float* dY, float* dW_ock, float* db, int32_t B, int32_t T,
                           int32_t Cin, int32_t N, int32_t k, int32_t accumulate, void* stream);
int dcf_op_layernorm_bwd(const float* X, const float* w, const float* b, const float* dOut, float* dX, float* dw, float* db,
                         int32_t rows, int32_t C, int32_t relu, int32_t accumulate, void* stream);
/* The k = 5 / stride 2 / padding 2 MaskedConv1D of vid_net.stride > 1 (video_net.py:62-70; dense, no bias) as a single operator and
 * its two gradients (additions to ABI version 12), on token-major fp32 rows, T even, To = T / 2:
 *   dcf_op_conv5s2_split      : Y[b,u,n]  = sum_{j<5} sum_c W[n,c,j] m[b,2u+j-2] X[b,2u+j-2,c]   (taps stay inside sequence b; Y (B*To, N)
 *                               is not masked; the mask that goes on is m[b,2u], blocks.py:101-105) -- the forward's own path: the five
 *                               taps gathered into rows, then the split-operand GEMM (nterms 16 = f16x3, 6 = bf16x6)
 *   dcf_op_conv5s2_bwd_weight : dW[n,c,j] = sum_{b,u} dY[b,u,n] m[b,2u+j-2] X[b,2u+j-2,c]
 *   dcf_op_conv5s2_bwd_data   : dX[b,t,c] = m[b,t] sum_{j = t (mod 2), 0 <= (t+2-j)/2 < To} sum_n dY[b,(t+2-j)/2,n] W[n,c,j]
 * W_ock / dW_ock: PyTorch's (N, Cin, 5) layout.  mask (B*T bytes, the INPUT rows) NULL = every row valid.  Cin % 32 == 0, N % 32 == 0,
 * T even; anything else fails with a message.  The gradients are f16x3 on the matrix cores with the device-side power-of-two scale of
 * dY, fixed-order sums without floating-point atomics (bit-identical from run to run; a power of two on dY scales them by exactly
 * that) and the sticky numerics word of dcf_op_conv_bwd_data / _weight: after a non-finite sum the NEXT call of any of these
 * functions returns -1 once. */
int dcf_op_conv5s2_split(const float* X, const uint8_t* mask, const float* W_ock, float* Y, int32_t B, int32_t T, int32_t Cin,
                         int32_t N, int32_t nterms, void* stream);
int dcf_op_conv5s2_bwd_data(const float* dY, const uint8_t* mask, const float* W_ock, float* dX, int32_t B, int32_t T, int32_t Cin,
                            int32_t N, void* stream);
int dcf_op_conv5s2_bwd_weight(const float* X, const uint8_t* mask, const float* dY, float* dW_ock, int32_t B, int32_t T, int32_t Cin,
                              int32_t N, int32_t accumulate, void* stream);
/* cross-attention core (libs/modeling/blocks.py:374-389): Q (B*T, C), K/V (B*Lk, C), kvmask (B*Lk) -> O (B*T, C).  Two fp16 planes
 * per operand: |x| <= 65504.  q d^-1/4, k d^-1/4 and the probabilities are unscaled (22 bits from 2^-3 on, an absolute floor of
 * 2^-25 below): they feed or leave a softmax.  The floor of v would reach the output, so where max |v| over the MFMA keys of a
 * (batch, head) is below 2^-2 its planes carry the power of two that lifts that maximum into [8, 16) (floor: 2^-28 max |v|);
 * a larger v runs on unscaled planes. */
int dcf_op_xattn(const float* Q, const float* K, const float* V, const uint8_t* kvmask, float* O, int32_t B, int32_t T,
                 int32_t Lk, int32_t C, int32_t heads, void* stream);
/* sliding-window attention core (blocks.py:204-325,357-373): Q/K/V (B*T, C), mask (B*T) -> O; window = 0: global attention over
 * every valid key of the sequence (blocks.py:339-356, :374-393; head dimension 32 or 64) */
int dcf_op_local_attn(const float* Q, const float* K, const float* V, const uint8_t* mask, float* O, int32_t B, int32_t T,
                      int32_t C, int32_t heads, int32_t window, void* stream);
/* Backward of the sliding-window core above for window > 0 (addition to ABI version 12).  It differentiates, per sequence b, head h
 * (head dimension d, channels h*d .. h*d + d - 1 of a row) and query row t, with half = window / 2 and scale = d^-1/4:
 *   s[t,j] = (scale q[t]) . (scale k[j]) + pen[j]     for |j - t| <= half, 0 <= j < T      (keys outside the sequence do not exist)
 *   pen[j] = -1e4 if key j is padded, else 0                                               (blocks.py:279: finite)
 *   p[t,.] = softmax_j s[t,j],  O[t] = sum_j p[t,j] v[j];   O[t] = 0 and p[t,.] = 0 if QUERY t is padded   (blocks.py:293)
 * and returns, given dO,
 *   dP[t,j] = dO[t] . v[j],   delta[t] = sum_j p[t,j] dP[t,j],   dS[t,j] = p[t,j] (dP[t,j] - delta[t])
 *   dV[j] = sum_t p[t,j] dO[t],   dQ[t] = scale^2 sum_j dS[t,j] k[j],   dK[j] = scale^2 sum_t dS[t,j] q[t]
 * with the sums over t running over the live queries whose window holds j.  Q / K / V / dO / dQ / dK / dV: (B*T, C) token-major fp32,
 * mask (B*T bytes) NULL = every row valid.  Any of dQ / dK / dV may be NULL: the work that only feeds it is skipped and the others
 * keep their bits.  Shapes: those of the forward (power-of-two head dimension in [4, 256], C % 4 == 0, C <= 1024), window odd;
 * window = 0 (global attention) and anything else unsupported fail with a message.  dO is not assumed to be masked, but a padded
 * query row passes nothing on: dQ is exactly 0 there, and dK = dV = 0 exactly at a padded key row (exp(-1e4 - m) is 0).
 * fp32 on the vector ALU; dK / dV are gathered per key row in ascending t, without floating-point atomics: results are bit-identical
 * from run to run and scaling dO by a power of two scales them by exactly that.  The per-row softmax statistics live in scratch
 * that is allocated and freed on `stream`; no host wait. */
int dcf_op_local_attn_bwd(const float* Q, const float* K, const float* V, const uint8_t* mask, const float* dO, float* dQ, float* dK,
                          float* dV, int32_t B, int32_t T, int32_t C, int32_t heads, int32_t window, void* stream);
/* Forward / backward pairs of what a TransformerEncoder block (libs/modeling/blocks.py:541-591) needs besides the operators above
 * (additions to ABI version 12; csrc/enc_grad.hip).  Conventions of all eight: token-major fp32 rows (B*T, C), C % 4 == 0, C <= 1024,
 * 16-byte aligned pointers; a mask is B*T bytes, NULL = every row valid; everything runs on `stream` without a host wait, scratch is
 * allocated and freed on it; no floating-point atomics -- the two column reductions (dW, dls) run over fixed row slices and a balanced
 * tree in a fixed order, so results are bit-identical from run to run and scaling the upstream gradient by a power of two scales them
 * by exactly that; an output pointer that is NULL skips the work that only feeds it; accumulate != 0 adds into the parameter gradient
 * (`.grad +=`); unsupported shapes fail with a message.  The upstream gradient is not assumed to be masked.
 *
 * Depthwise MaskedConv1D (blocks.py:87-106 with groups = C; k = 3, padding 1, no bias, stride s = 1 or 2 dividing T), n = 1 .. 3
 * convolutions sharing one input (n = 3: q / k / v_conv of ConvAttNLayer, blocks.py:437-445, :464-466; n = 1: a pool_only branch
 * layer, the decoder's q_conv).  W (n, C, 3): PyTorch's (C, 1, 3) weights stacked; Y / dY (n, B*T/s, C); X is read once for all n.
 *   Y_i[b,o,c] = sum_j W_i[c,j] m[b,s o+j-1] X[b,s o+j-1,c]        (taps stay inside sequence b; Y is not masked; the mask of Y is m[b, s o])
 *   dX[b,t,c]  = m[b,t] sum_i sum_j dY_i[b,o,c] W_i[c,j]           over the (o, j) with s o + j - 1 = t, i then j ascending
 *   dW_i[c,j]  = sum_{b,o} dY_i[b,o,c] m[b,s o+j-1] X[b,s o+j-1,c] */
int dcf_op_dwconv3(const float* X, const uint8_t* mask, const float* W, float* Y, int32_t B, int32_t T, int32_t C, int32_t n,
                   int32_t stride, void* stream);
int dcf_op_dwconv3_bwd(const float* X, const uint8_t* mask, const float* W, const float* dY, float* dX, float* dW, int32_t B, int32_t T,
                       int32_t C, int32_t n, int32_t stride, int32_t accumulate, void* stream);
/* masked_max_pool1d (blocks.py:31-47) with kernel 3, stride 2, padding 1; T even; Y / dY (B*T/2, C), mask_out (B*T/2 bytes, may be NULL).
 *   f[b,t,c]  = m[b,t] ? X[b,t,c] : min_t' X[b,t',c]              (the minimum over all T rows of the channel; detached, blocks.py:38)
 *   mo[b,o]   = m[b,2o-1] | m[b,2o] | m[b,2o+1]                   (positions inside the sequence)
 *   Y[b,o,c]  = mo[b,o] max_{t in {2o-1, 2o, 2o+1}, 0 <= t < T} f[b,t,c]
 *   dX[b,t,c] = m[b,t] sum of dY[b,o,c] mo[b,o] over the at most two windows o whose maximum sits at t
 * The backward recomputes the selection from (X, mask): among equal values the lowest position holds the maximum (torch's CPU pooling
 * takes the first `val > max`), and the choice is made on the filled values f -- a padded slot that wins swallows the gradient. */
int dcf_op_masked_maxpool(const float* X, const uint8_t* mask, float* Y, uint8_t* mask_out, int32_t B, int32_t T, int32_t C, void* stream);
int dcf_op_masked_maxpool_bwd(const float* X, const uint8_t* mask, const float* dY, float* dX, int32_t B, int32_t T, int32_t C,
                              void* stream);
/* exact (erf) GELU of FFN.actv (blocks.py:531, :536) on n elements: Y = X Phi(X), dX = dY (Phi(X) + X phi(X)), Phi / phi the standard
 * normal distribution function / density; Phi from erfc of |x| / sqrt 2 (the lower tail keeps its relative accuracy), phi from exp with
 * the rounding residual of x^2 carried. */
int dcf_op_gelu(const float* X, float* Y, int64_t n, void* stream);
int dcf_op_gelu_bwd(const float* X, const float* dY, float* dX, int64_t n, void* stream);
/* LayerScale residual (blocks.py:670-682 inside :586 and :589-590): Y = R m_R + ls (H m_H), ls (C) broadcast over the rows, either
 * mask NULL (`skip * mask + ls * h` of :586 is m_H NULL, `x + ls * (h * mask)` of :589-590 is m_R NULL).  H NULL: Y = R m_R.
 *   dR = dY m_R,   dH = ls dY m_H,   dls[c] = sum_rows dY H m_H */
int dcf_op_layerscale_residual(const float* R, const uint8_t* mR, const float* H, const uint8_t* mH, const float* ls, float* Y, int32_t rows,
                               int32_t C, void* stream);
int dcf_op_layerscale_residual_bwd(const float* dY, const float* H, const uint8_t* mR, const uint8_t* mH, const float* ls, float* dR, float* dH,
                                   float* dls, int32_t rows, int32_t C, int32_t accumulate, void* stream);
/* Backward of the cross-attention core dcf_op_xattn and the AdaLN modulation of a fusion decoder layer with its backward (additions to
 * ABI version 12; csrc/xattn_grad.hip).  Token-major fp32, 16-byte aligned pointers, everything on `stream` without a host wait, scratch
 * allocated and freed on it, no floating-point atomics; an output pointer that is NULL skips the work that only feeds it and leaves the
 * bits of the others unchanged; unsupported shapes fail with a message, nothing falls back to another arithmetic.
 *
 * dcf_op_xattn_bwd differentiates, per sequence b, head h (head dimension d = C / heads), query row t < T and key j < Lk, scale = d^-1/4:
 *   s[t,j] = (scale q[t]) . (scale k[j])     over the keys with kvmask[b,j] != 0; a masked key contributes exactly 0 (blocks.py:381-384)
 *   p[t,.] = softmax_j s[t,j],   O[t] = sum_j p[t,j] v[j]
 * and returns, given dO,
 *   dP[t,j] = dO[t] . v[j],   delta[t] = sum_j p[t,j] dP[t,j],   dS[t,j] = p[t,j] (dP[t,j] - delta[t])
 *   dQ[t] = scale^2 sum_j dS[t,j] k[j],   dK[j] = scale^2 sum_t dS[t,j] q[t],   dV[j] = sum_t p[t,j] dO[t]
 * Q / dO / dQ: (B*T, C); K / V / dK / dV: (B*Lk, C); kvmask (B*Lk bytes), NULL = every key valid.  There is no query mask (the
 * reference's global branch has none): dO at every row is used.  dK = dV = 0 exactly at a masked key.  A sequence without a valid key is
 * NaN in the forward and undefined here.  delta is formed from p and dP, so a one-key sequence gives dQ = dK = 0 exactly.
 * Shapes: 1 <= Lk <= 64, head dimension 16, 32, 64 or 128, C % 4 == 0, C <= 1024, any T >= 1, B <= 65535; Lk = 0, Lk > 64 and any other
 * head dimension fail with a message (there is no slower variant).  fp32 on the vector ALU, the exponential with its rounding residual
 * carried.  dK / dV are summed per workgroup over slices of 512 query rows of a sequence (a constant: the order depends on the shapes
 * alone, never on the device), the slices then in a fixed blocked order: results are bit-identical from run to run and scaling dO by
 * a power of two scales them by exactly that.
 *
 * dcf_op_adaln, per row: Y = N(X m) * H[:, :C] + H[:, C:]  (blocks.py:643-645), X / Y (rows, C), H (rows, 2C) the cross-attention output
 * (scale | shift), m (rows bytes) the row mask, NULL = every row valid; N = the affine-free channel LayerNorm (blocks.py:125-131, two-pass,
 * eps 1e-5) for norm != 0, the identity for norm = 0 (xattn_mode 'affine', blocks.py:622-626).  A masked row has N(0) = 0: Y = shift.
 * dcf_op_adaln_bwd: dH[:, :C] = dY * N(X m),  dH[:, C:] = dY,  dX = m LN'(dY * H[:, :C])  (norm = 0: m dY * H[:, :C]); dX = 0 exactly at
 * a masked row.  dX or dH may be NULL.  C % 4 == 0, C <= 1024. */
int dcf_op_xattn_bwd(const float* Q, const float* K, const float* V, const uint8_t* kvmask, const float* dO, float* dQ, float* dK,
                     float* dV, int32_t B, int32_t T, int32_t Lk, int32_t C, int32_t heads, void* stream);
int dcf_op_adaln(const float* X, const uint8_t* mask, const float* H, float* Y, int32_t rows, int32_t C, int32_t norm, void* stream);
int dcf_op_adaln_bwd(const float* X, const uint8_t* mask, const float* H, const float* dY, float* dX, float* dH, int32_t rows, int32_t C,
                     int32_t norm, void* stream);
/* Forward / backward pairs of the refinement stage of PtTransformerEarlyFusionIterative (model.py:449-455, tcn.py:21-38; additions to
 * ABI version 12; csrc/refine_grad.hip).  Conventions of all four: token-major fp32 rows (B*T0, 32), 16-byte aligned pointers; a mask is
 * B*T0 bytes, NULL = every row valid; everything runs on `stream` without a host wait, scratch is allocated and freed on it; no
 * floating-point atomics -- parameter gradients are summed over fixed slices of 128 rows (RG_SLICE_ROWS) and then in a fixed blocked
 * tree, so results are bit-identical from run to run and scaling the upstream gradient by a power of two scales them by exactly that;
 * an output pointer that is NULL skips the work that only feeds it and leaves the bits of the others unchanged; accumulate != 0 adds
 * into the parameter gradients (`.grad +=`); unsupported shapes fail with a message.  Weights are in PyTorch's layouts.  fp32 on the
 * vector ALU, every contraction an fma chain in ascending index; there is no other arithmetic to fall back to.
 *
 * dcf_op_refine_in: the stacking of the nearest-upsampled first-pass logits (model.py:449-455) fused with refine.conv_1x1.
 * logits1 (B, S) in the pyramid order of the forward's outputs: level l at offset sum_{j<l} T_j, T_l = T0 >> l, S = sum_l T_l;
 * W_in (32, L), b_in (32); 1 <= L <= 16, T0 % 2^(L-1) == 0.
 *   u[b,t,0] = logits1[b,0,t]   (level 0 is not masked, to the letter),   u[b,t,l] = m0[b,t] logits1[b,l,t >> l]   for l > 0
 *   H[b,t,c] = b_in[c] + sum_l W_in[c,l] u[b,t,l]
 *   dlogits1[b,l,s] = sum over the 2^l rows t >> l == s, t ascending, of (l == 0 ? 1 : m0[b,t]) sum_c W_in[c,l] dH[b,t,c]
 *   dW_in[c,l] = sum_{b,t} dH[b,t,c] u[b,t,l],   db_in[c] = sum_{b,t} dH[b,t,c]
 *
 * dcf_op_tcn_layer: one DilatedResidualLayer (tcn.py:21-38) on 32 channels: Wd (32, 32, 3), Wp (32, 32), dilation >= 1.
 *   h = relu(bd + sum_{j,ci} Wd[.,ci,j] X[b, t + (j-1) dilation, ci])   (taps stay inside sequence b; the input is NOT masked: the
 *                                                                        reference's convolution is a plain nn.Conv1d)
 *   o = drop(bp + Wp h),   z = (X + o) m,   Y = LN(z) ln_w + ln_b       (two-pass, eps 1e-5)
 * drop: element (b, c, t) is kept iff drop_keep(seed, drop_site(DROP_G_REFINE, layer, DROP_TCN), ((b0 + b) * 32 + c) * T0 + t, p)
 * (csrc/dropout.h: the bits of the training forward, dcf_model_set_dropout) and then multiplied by 1 / (1 - p); p = 0 is the identity
 * and runs the kernel compiled without dropout.
 * dcf_op_tcn_layer_bwd saves nothing but X: it recomputes h, o, the keep bits and the LayerNorm statistics, and returns dX, dWd, dbd,
 * dWp, dbp, dln_w, dln_b (any may be NULL).  ReLU passes nothing at h == 0.  At a padded row dz = 0, but dln_b still takes dY there (the
 * LayerNorm runs on every row); dX is NOT zero at padded rows: valid neighbours read them through the unmasked side taps. */
int dcf_op_refine_in(const float* logits1, const uint8_t* mask0, const float* W_in, const float* b_in, float* H, int32_t B, int32_t T0,
                     int32_t L, void* stream);
int dcf_op_refine_in_bwd(const float* logits1, const uint8_t* mask0, const float* W_in, const float* dH, float* dlogits1, float* dW_in,
                         float* db_in, int32_t B, int32_t T0, int32_t L, int32_t accumulate, void* stream);
int dcf_op_tcn_layer(const float* X, const uint8_t* mask, const float* Wd, const float* bd, const float* Wp, const float* bp,
                     const float* ln_w, const float* ln_b, float* Y, int32_t B, int32_t T0, int32_t dilation, int64_t seed, float p,
                     int32_t layer, int32_t b0, void* stream);
int dcf_op_tcn_layer_bwd(const float* X, const uint8_t* mask, const float* Wd, const float* bd, const float* Wp, const float* bp,
                         const float* ln_w, const float* ln_b, const float* dY, float* dX, float* dWd, float* dbd, float* dWp, float* dbp,
                         float* dln_w, float* dln_b, int32_t B, int32_t T0, int32_t dilation, int64_t seed, float p, int32_t layer,
                         int32_t b0, int32_t accumulate, void* stream);
/* sidekick scoring (model.py:500-505): shallow (D, T) channel-major, text_cls (nq, D) -> correl (nq, T) */
int dcf_op_sidekick(const float* shallow, const float* text_cls, float* correl, int32_t D, int32_t T, int32_t nq,
                    int32_t norm, void* stream);
/* block top-k gate (model.py:531-541) for nq queries: correl (nq, T), vid_mask (T) -> gate (nq, T) fp32 0/1 */
int dcf_op_gate(const float* correl, const uint8_t* vid_mask, float* gate, uint8_t* mask_out, int32_t T, int32_t nq,
                int32_t sn, double sratio, int32_t msf, void* stream);

/* --------------------------------------------------------------------------------------------
 * Composite blocks on a SCRATCH model (ABI version 4): dcf_model_create(cfg) + dcf_model_bind of the block's parameters
 * under `prefix` (reference state_dict names below it), never finalized.  They exist so that the reference's operator
 * fixtures (tests/golden/ops.npz) run through the very kernels and launch sequences of the forward.  Token-major rows.
 *   dcf_op_encoder : TransformerEncoder.forward (libs/modeling/blocks.py:578-591, ConvAttNLayer :462-473), stride 1 or 2;
 *                    X (B*T, E), mask (B*T) -> Y (B*T/stride, E), mask_out (B*T/stride).  Uses cfg E, vid_heads, win, gemm_mode.
 *   dcf_op_enc_pre : its front half alone -- ln_attn, the three depthwise k3 convolutions (blocks.py:63-106, groups = E),
 *                    their LayerNorms and, for stride 2, masked_max_pool1d (blocks.py:31-47) -> Qc, Kc, Vc, Skip (B*T/stride, E).
 *   dcf_op_decoder : TransformerDecoder.forward (blocks.py:632-650, ConvXAttNLayer :513-520, adaln) in place on X (B*T, E);
 *                    text[b] (TE, len_b) channel-major, text_mask[b] (len_b) or NULL.  Uses cfg E, TE, fusion_heads, gemm_mode.
 *   dcf_op_tcn     : TCN.forward (libs/modeling/tcn.py:66-84) on x (B*T, n_in) -> Y (B*T, 32).
 * ------------------------------------------------------------------------------------------ */
int dcf_op_encoder(dcf_model* m, const char* prefix, const float* X, const uint8_t* mask, int32_t B, int32_t T, int32_t stride,
                   float* Y, uint8_t* mask_out, void* stream);
int dcf_op_enc_pre(dcf_model* m, const char* prefix, const float* X, const uint8_t* mask, int32_t B, int32_t T, int32_t stride,
                   float* Qc, float* Kc, float* Vc, float* Skip, void* stream);
int dcf_op_decoder(dcf_model* m, const char* prefix, float* X, const uint8_t* mask, int32_t B, int32_t T,
                   const float* const* text, const uint8_t* const* text_mask, const int32_t* text_len, void* stream);
int dcf_op_tcn(dcf_model* m, const char* prefix, const float* x, const uint8_t* mask, int32_t B, int32_t T, int32_t n_in,
               int32_t n_layers, float* Y, void* stream);

/* --------------------------------------------------------------------------------------------
 * The training update (libs/worker_v2.py:320-325): clip_grad_norm_, Adam / AdamW .step() and the EMA copy as multi-tensor kernels
 * over a DEVICE TABLE that the host builds (additions to ABI version 12).  fp32, no atomics, nothing waits on the host.
 *
 * The table: n_tensors rows of dcf_optim_row (64 bytes each, no padding), one per parameter tensor, in device memory.
 *   p, g, exp_avg, exp_avg_sq, ema : device addresses of n contiguous fp32 each; ema may be NULL (no EMA copy of this tensor); g,
 *                                    exp_avg and exp_avg_sq are not read when the row has DCF_OPTIM_NO_GRAD.  An address need only be
 *                                    4-byte aligned: arrays on a 16-byte boundary move through 16-byte accesses, the others and the last
 *                                    n % 4 elements one element at a time, with the same arithmetic.
 *   n      : elements (>= 0)
 *   group  : index into the groups of dcf_optim_adam_step
 *   flags  : DCF_OPTIM_NO_GRAD = no gradient this step (torch's `grad is None`)
 *   chunk0 : the PREFIX: the number of chunks of the rows before this one, chunk0[i+1] = chunk0[i] + ceil(n[i] / DCF_OPTIM_CHUNK)
 * The chunk map: n_chunks int32 in device memory, chunk_map[c] = the row that owns chunk c (rows in ascending order, a row with
 * n == 0 owns none).  One workgroup runs chunk c: it covers the elements [(c - chunk0) * DCF_OPTIM_CHUNK, + DCF_OPTIM_CHUNK) of its
 * row, the last chunk of a row being short.  A chunk is DCF_OPTIM_CHUNK = 4096 elements.
 *
 * dcf_optim_grad_norm: the L2 norm of every gradient that is present, and torch's clip coefficient.
 *   Each lane sums the squares of its own 16 elements in fp32; lanes, waves and chunks are added in fp64 in a fixed order (chunk
 *   partials, then one workgroup over the partials), so the result has the same bits on every run.
 *   *norm_out = (float) sqrt(sum);  *coef_out = min(1, max_norm / (norm + 1e-6)) in fp32, 1 for max_norm <= 0.  A NaN norm gives a NaN
 *   coefficient (and an infinite one gives 0), as torch.nn.utils.clip_grad_norm_ does by default.  Either output may be NULL.
 * dcf_optim_scale: g *= *scale for every gradient that is present (scale: one device float).
 * dcf_optim_adam_step: one pass.  Per element of a row whose gradient is present, with the row's group h and c = coef ? *coef : 1:
 *     g' = g c;   DCF_OPTIM_ADAMW: p *= 1 - lr wd;   DCF_OPTIM_ADAM: g' += wd p
 *     m = b1 m + (1 - b1) g';   v = b2 v + (1 - b2) g'^2;   p -= (lr / bc1) (m / (sqrt(v) / sqrt_bc2 + eps))
 *   every product, sum, quotient and root rounded once to fp32; 1 - b1 and 1 - b2 are the group's one_minus_b1 / one_minus_b2, taken in
 *   double on the host (in fp32, 1 - 0.999f is off by 1.3e-5 of its value, and with it the whole second moment).  A row with DCF_OPTIM_NO_GRAD keeps p, exp_avg and exp_avg_sq bit for
 *   bit.  Then, with_ema != 0 and ema != NULL, gradient or not:  ema = lerp(p_new, ema, beta) by torch's two-branch rule
 *     beta < 0.5: p + beta (ema - p);   else: ema - (ema - p)(1 - beta)          (beta = 0: p's bits; beta = 1: ema untouched)
 *   The stored gradients are not written.  `groups` is a HOST array of n_groups <= DCF_OPTIM_MAX_GROUPS records that travels by
 *   value with the launch (a new learning rate needs no upload); bc1 = 1 - b1^t and sqrt_bc2 = sqrt(1 - b2^t) come from the host, in double.
 * A null table, a negative count, more than DCF_OPTIM_MAX_GROUPS groups and an unknown mode fail with a message.
 * ------------------------------------------------------------------------------------------ */
#define DCF_OPTIM_CHUNK 4096
#define DCF_OPTIM_MAX_GROUPS 8
#define DCF_OPTIM_NO_GRAD 1
#define DCF_OPTIM_ADAMW 0
#define DCF_OPTIM_ADAM 1
typedef struct dcf_optim_row {
  void* p;
  void* g;
  void* exp_avg;
  void* exp_avg_sq;
  void* ema;
  int64_t n;
  int32_t group;
  int32_t flags;
  int64_t chunk0;
} dcf_optim_row;
typedef struct dcf_optim_group {
  float lr;
  float weight_decay;
  float b1;
  float b2;
  float one_minus_b1;
  float one_minus_b2;
  float eps;
  float bc1;
  float sqrt_bc2;
  int32_t mode;
} dcf_optim_group;
int dcf_optim_grad_norm(const dcf_optim_row* table, const int32_t* chunk_map, int32_t n_tensors, int64_t n_chunks, float max_norm,
                        float* norm_out, float* coef_out, void* stream);
int dcf_optim_scale(const dcf_optim_row* table, const int32_t* chunk_map, int32_t n_tensors, int64_t n_chunks, const float* scale,
                    void* stream);
int dcf_optim_adam_step(const dcf_optim_row* table, const int32_t* chunk_map, int32_t n_tensors, int64_t n_chunks,
                        const dcf_optim_group* groups, int32_t n_groups, const float* coef, int32_t with_ema, float ema_beta, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DECAFNET_HIP_H */
