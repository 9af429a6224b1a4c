// Runtime of the grounding forward: owns the parameter table (bound by reference state_dict
// name), repacked convolution weights, the HBM workspace arena and the launch sequence of
// PtTransformerEarlyFusionIterative._drop_forward_eval (libs/modeling/model.py:480-565).
//
// HBM layout of one batched forward (B queries of one video, T0 padded clips, S = sum_l T0/2^l):
//   P1, P2      [T0][E]          query-independent halves of vid_map (W[:, :D].vid, W[:, D:].shallow)
//   X, R0..R6   [B*T0][E]        token-major activations (level l uses the first B*T_l rows)
//   H2          [B*T0][2E]       xattn projection (AdaLN scale | shift)
//   HID         [B*T0][4E]       FFN hidden
//   F           [B*S][E+32]      feature pyramid, rows ordered [level][query][t]; the last 32
//                                columns receive the refined logits (model.py:462-467)
//   HA, HB      [B*S][E+32]      head trunk ping-pong
//   mask_all, nbr_all [B*S]      per-row validity / k3-neighbour flags for every level
// Nothing here synchronises the host: vid_len, the gate and every mask stay on the device.
#include <algorithm>

#include "engine.h"
#include "../../include/decafnet_hip_half.h"
#include "../../include/decafnet_hip_select.h"
#include "../../include/decafnet_hip_select_videos.h"

namespace dcf {

// masks_out[b][off_l + t] = mask_all[start_l + b*T_l + t].  Last kernel of a forward: when the sticky numerics word of the
// f16x3 GEMMs is raised -- bit 0: an operand left the fp16 range somewhere upstream, and a ReLU / max may have swallowed the
// NaN since; bit 1: a LayerNorm carried as one-pass row statistics met a row whose mean dwarfs its spread (common.h
// LN_ILL_RATIO), its rstd is off by an unbounded amount -- the logits of the forward are overwritten with NaN, so that a
// caller who never asks dcf_numerics_status -- the reference's Evaluator -- sees invalid scores instead of plausible wrong ones.
__global__ void k_masks_out(const uint8_t* __restrict__ mask_all, uint8_t* __restrict__ out, const LevelTable* lt,
                            const unsigned* __restrict__ status, float* __restrict__ logits) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  const int total = lt->start[lt->n_levels];
  if (r >= total) return;
  int l = 0;
  while (l + 1 < lt->n_levels && r >= lt->start[l + 1]) ++l;
  const int rel = r - lt->start[l];
  const int b = rel / lt->T[l], t = rel - b * lt->T[l];
  const int64_t o = (int64_t)b * lt->S + lt->off[l] + t;
  out[o] = mask_all[r];
  if (status && (status[0] & 3u)) logits[o] = __uint_as_float(0x7fc00000u);
}
void launch_masks_out(const uint8_t* mask_all, uint8_t* out, const LevelTable* lt, const unsigned* status, float* logits, int rows,
                      hipStream_t st) {
  hipLaunchKernelGGL(k_masks_out, dim3((rows + 255) / 256), dim3(256), 0, st, mask_all, out, lt, status, logits);
}

// out[b][off_l + t] = rows[start_l + b*T_l + t]: a per-point value of the pyramid from level-major to query-major order
__global__ void k_points_out(const float* __restrict__ rows, float* __restrict__ out, const LevelTable* lt) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  const int total = lt->start[lt->n_levels];
  if (r >= total) return;
  int l = 0;
  while (l + 1 < lt->n_levels && r >= lt->start[l + 1]) ++l;
  const int rel = r - lt->start[l];
  const int b = rel / lt->T[l], t = rel - b * lt->T[l];
  out[(int64_t)b * lt->S + lt->off[l] + t] = rows[r];
}

// gate[b][t] = override[q0 + b][t]; mask = vid_mask (msf) or vid_mask & gate (model.py:544-545).  vid_mask (nvid, T): batch element b
// reads the row of its own video, nibble b of vmap (0 for one video)
__global__ void k_apply_gate(const float* __restrict__ gate_in, const uint8_t* __restrict__ vid_mask, float* __restrict__ gate,
                             uint8_t* __restrict__ mask_out, int T, int rows, int msf, unsigned long long vmap) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const int t = r % T + (int)((vmap >> (4 * ((r / T) & 15))) & 15ull) * T;
  const float g = gate_in[r];
  const bool m = vid_mask[t] != 0;
  gate[r] = g;
  mask_out[r] = msf ? m : (m && g != 0.f);
}

struct MaskPtrs { const uint8_t* p[DCF_MAX_VIDEOS]; };
__global__ void k_gather_masks(MaskPtrs mp, uint8_t* __restrict__ dst, int T0) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < T0) dst[(size_t)blockIdx.y * T0 + t] = mp.p[blockIdx.y][t];
}
// the videos' masks side by side, dst (nvid, T0): one launch (it was one copy node per video)
int launch_gather_masks(const uint8_t* const* masks, int nvid, uint8_t* dst, int T0, hipStream_t st) {
  MaskPtrs mp{};
  for (int v = 0; v < nvid; ++v) mp.p[v] = masks[v];
  hipLaunchKernelGGL(k_gather_masks, dim3((unsigned)((T0 + 255) / 256), (unsigned)nvid), dim3(256), 0, st, mp, dst, T0);
  DCF_HIP(hipGetLastError());
  return 0;
}

int grow_half_ws(dcf_model* m, size_t need, hipStream_t st) {
  if (need <= m->half_ws_bytes) return 0;
  DCF_CHECK(!m->capturing, "internal: workspace growth during graph capture");
  drop_graph(m, true);                          // (a captured graph bakes the copies' addresses in)
  DCF_HIP(hipStreamSynchronize(st));
  if (m->half_ws) DCF_HIP(hipFree(m->half_ws));
  m->half_ws = nullptr; m->half_ws_bytes = 0;
  DCF_HIP(hipMalloc(&m->half_ws, need));
  m->half_ws_bytes = need;
  return 0;
}

// Half features (VideoSet::half): read as they are where the kernels in front can -- the split-operand vid_map GEMMs (with the scores on
// their side or the scoring kernels beside them) --, otherwise upcast once into m->half_ws and handed on as an fp32 video set.
// *use = the set the forward goes on with.  dcf_debug_set_option("half_native", 0 / 1 / 2): never / where possible / or fail.
static int half_features(dcf_model* m, const VideoSet& in, int T0, const ForwardCall& fc, hipStream_t st, VideoSet& f32, const VideoSet** use) {
  const dcf_config& c = m->cfg;
  DCF_CHECK(!fc.gate && !in.logits1_out && m->hyb_levels == 0, "half features: the eval forwards dcf_forward_eval_h / dcf_forward_eval_videos_h only");
  const int want = debug_option("half_native", 1);
  auto image_ok = [&](const float* w) { return !w || (m->wsplit.count(w) && m->wsplit_ldw[w] == m->vid_ldw); };
  bool native = want != 0 && m->gemm_terms != 0 && c.E % 128 == 0 && T0 % 4 == 0 && image_ok(m->vid_w1) && image_ok(m->vid_w2) && (m->vid_w1 || m->vid_w2);
  if (m->vid_w1 && m->vid_w2) native = native && m->wsplit_terms[m->vid_w1] == m->wsplit_terms[m->vid_w2];
  for (int v = 0; v < in.nvid; ++v)
    native = native && ((reinterpret_cast<uintptr_t>(in.vid[v]) | reinterpret_cast<uintptr_t>(in.shallow[v])) & 7) == 0;
  DCF_CHECK(native || want != 2, "half features: this forward cannot read them natively (gemm_mode fp32, E %% 128 != 0, T %% 4 != 0 or a feature "
                                 "pointer that is not 8-byte aligned) and the option half_native = 2 forbids the upcast");
  if (native) { *use = &in; return 0; }
  const size_t per = ((size_t)c.D * T0 * sizeof(float) + 255) & ~(size_t)255;
  TRY(grow_half_ws(m, per * 2 * in.nvid, st));
  f32 = in;
  f32.half = false;
  for (int v = 0; v < in.nvid; ++v) {
    float* dv = reinterpret_cast<float*>(m->half_ws + per * (2 * v));
    float* ds = reinterpret_cast<float*>(m->half_ws + per * (2 * v + 1));
    TRY(launch_half_to_f32(reinterpret_cast<const uint16_t*>(in.vid[v]), dv, (int64_t)c.D * T0, st));
    TRY(launch_half_to_f32(reinterpret_cast<const uint16_t*>(in.shallow[v]), ds, (int64_t)c.D * T0, st));
    f32.vid[v] = dv; f32.shallow[v] = ds;
  }
  *use = &f32;
  return 0;
}

int forward(dcf_model* m, const VideoSet& vs_in, int T0, int nq, const ForwardCall& fc, hipStream_t st) {
  const dcf_config& c = m->cfg;
  VideoSet vs_f32;                                // half features this forward reads as fp32 copies (below)
  const VideoSet* vsp = &vs_in;
  DCF_CHECK(m->finalized, "dcf_forward_eval: model not finalized");
  DCF_CHECK(T0 > 0 && nq > 0 && vs_in.nvid >= 1 && vs_in.nvid <= DCF_MAX_VIDEOS, "dcf_forward_eval: empty input");
  if (vs_in.half) TRY(half_features(m, vs_in, T0, fc, st, vs_f32, &vsp));
  const VideoSet& vs = *vsp;
  const bool half_native = vs.half;               // the kernels that read the features read binary16
  const int E = c.E, D = c.D;
  const int L = m->hyb_levels > 0 ? m->hyb_levels : c.n_levels;      // dcf_hybrid_phase1: the pyramid up to the split level only
  const int nvid = vs.nvid;
  if (m->hyb) m->hyb->valid = false;              // the phases of a level-cut forward live in this workspace
  const bool sel = fc.sel_rows != nullptr;        // dcf_forward_eval_selected: the expert product on the rows of the selected clips
  DCF_CHECK(!(fc.gate && nvid != 1) || (sel && fc.sel_first), "the externally gated forward takes one video");
  int video_of[DCF_MAX_VIDEOS * 64];           // flat query -> video
  {
    int tot = 0;
    for (int v = 0; v < nvid; ++v) {
      DCF_CHECK(vs.nq[v] >= 1 && tot + vs.nq[v] <= DCF_MAX_VIDEOS * 64, "dcf_forward_eval: bad query count of video %d", v);
      for (int i = 0; i < vs.nq[v]; ++i) video_of[tot++] = v;
    }
    DCF_CHECK(tot == nq, "dcf_forward_eval: query counts do not add up");
  }
  const uint8_t* vid_mask = vs.mask[0];
  // vid_net.stride = sv > 1 (video_net.py:59-74, worker_v2.py:285-286): vid_map and the early fusion run on the T0 input clips, the first
  // log2(sv) embedding convolutions halve the sequence, the pyramid starts at Tp = T0 / sv
  const int sv = vid_stride_of(c);
  int npre = 0;
  while ((1 << npre) < sv) ++npre;
  DCF_CHECK(T0 % (sv << (L - 1)) == 0, "T=%d must be a multiple of vid_net.stride * 2^(levels-1)=%d", T0, sv << (L - 1));
  const int Tp = T0 / sv;
  const int half = c.win / 2;
  DCF_CHECK(half == 0 || c.pool_only || (Tp >> (L - 1)) % half == 0, "T=%d: coarsest level must be a multiple of win//2=%d (blocks.py:216)", T0, half);
  if (c.use_abs_pe) DCF_CHECK(m->pe && m->pe_T == Tp, "position encoding for T=%d not set (dcf_model_set_pe)", Tp);
  DCF_CHECK(!(fc.gate && sv > 1), "the externally gated (T-sharded) forward takes vid_net.stride = 1");
  const int Bmax = std::min(nq, c.max_batch > 0 ? c.max_batch : 8);
  DCF_CHECK(Bmax <= DCF_MAX_BATCH, "max_batch %d > %d", Bmax, DCF_MAX_BATCH);
  DCF_CHECK(nvid == 1 || Bmax <= 16, "several videos per forward need max_batch <= 16 (got %d)", Bmax);
  int Lk = 1;
  for (int q = 0; q < nq; ++q) {
    DCF_CHECK(fc.text_len[q] >= 1 && fc.text[q], "text %d is empty", q);
    Lk = std::max(Lk, (int)fc.text_len[q]);
  }
  int S = 0;
  for (int l = 0; l < L; ++l) S += Tp >> l;

  // ---- workspace
  Buffers b{};
  const size_t need = carve_at(nullptr, c, T0, Bmax, nq, S, Lk, nvid, b, m->hyb_extra, &m->hyb_extra_ptr);
  if (need > m->arena_bytes) {
    DCF_CHECK(!m->capturing, "internal: workspace growth during graph capture");
    drop_graph(m, true);                       // the eager call that grows the workspace still counts as the first sighting
    DCF_HIP(hipStreamSynchronize(st));
    if (m->arena) DCF_HIP(hipFree(m->arena));
    m->arena = nullptr; m->arena_bytes = 0;
    DCF_HIP(hipMalloc(&m->arena, need));
    m->arena_bytes = need;
  }
  carve_at(m->arena, c, T0, Bmax, nq, S, Lk, nvid, b, m->hyb_extra, &m->hyb_extra_ptr);
  // ---- per video: sidekick scores and the query-independent halves of vid_map
  DCF_CHECK(!(fc.gate && c.scat) || fc.sel_correl, "opt.model.scat needs the sidekick scores: the externally gated (T-sharded) forward does not take them");
  SelFirst sel_first{};                           // first row of every video among the selected rows
  if (sel) {
    DCF_CHECK(fc.gate && fc.sel_pos && (nvid == 1 || fc.sel_first), "internal: the selected-clip forward is an externally gated forward");
    DCF_CHECK(!fc.sel_correl || (fc.sel_first && c.scat), "internal: the scores go with dcf_forward_eval_videos_selected on a scat model");
    for (int v = 0; v <= nvid; ++v) sel_first.r[v] = fc.sel_first ? fc.sel_first[v] : (v == 0 ? 0 : fc.sel_n);
    DCF_CHECK(m->vid_w1, "dcf_forward_eval_selected: opt.model.sfonly reads no expert features: there is nothing to select");
    DCF_CHECK(fc.sel_n >= 1 && fc.sel_n <= (int64_t)nvid * T0, "dcf_forward_eval_selected: n_rows=%d must lie in [1, T=%d] a video", fc.sel_n, T0);
    DCF_CHECK(D % 4 == 0 && aligned16(fc.sel_rows), "dcf_forward_eval_selected: vid_rows needs D %% 4 == 0 and a 16-byte aligned base");
  }
  // The sidekick scores ride on the shallow half of vid_map where they can: that GEMM streams exactly the (D, T) matrix the scores
  // are a reduction of, so the scoring pass's read of it (4 KB per clip) disappears; otherwise three launches of their own.
  // (dcf_debug_set_option("fuse_scores", 0) = the scoring kernels)
  static const Setting no_fuse_scores(nullptr, "DCF_NO_FUSE_SCORES", 0, Setting::PRESENT);
  bool scores_on_gemm = !fc.gate && !no_fuse_scores.get() && debug_option("fuse_scores", 1) != 0 && m->vid_w2 && m->gemm_terms != 0 && m->wsplit.count(m->vid_w2) &&
                        m->wsplit_ldw[m->vid_w2] == m->vid_ldw && E % 128 == 0 && T0 % 4 == 0;
  for (int v = 0; v < nvid; ++v) scores_on_gemm = scores_on_gemm && vs.nq[v] <= GEMM_SCORE_MAXQ;
  {
    // ... and the text vectors of a video's queries have to fit beside the GEMM's tile in the default 64 KiB of LDS (the tile and its
    // statistics block take ~22 KiB): 4 queries x D = 2048 do, D = 4096 does not -- the scoring kernels serve those
    int maxq = 0;
    for (int v = 0; v < nvid; ++v) maxq = std::max(maxq, vs.nq[v]);
    scores_on_gemm = scores_on_gemm && (size_t)maxq * D * sizeof(float) <= 40960;
  }
  int q_of[DCF_MAX_VIDEOS];                          // first query row of video v in tn / correl
  for (int v = 0, q_off = 0; v < nvid; q_off += vs.nq[v], ++v) q_of[v] = q_off;
  if (!fc.gate) {                              // the scores of every video's queries
    DCF_CHECK(nvid <= SCORE_MAXVID, "%d videos per forward > %d", nvid, SCORE_MAXVID);
    ScoreArgs sa{};
    for (int v = 0; v < nvid; ++v) {
      sa.shallow[v] = vs.shallow[v]; sa.text_cls[v] = vs.text_cls[v]; sa.nq[v] = vs.nq[v]; sa.qoff[v] = q_of[v];
    }
    sa.nvid = nvid; sa.tn = b.tn; sa.partial = b.partial; sa.correl = b.correl; sa.D = D; sa.T = T0; sa.NQ = nq; sa.norm = c.norm;
    if (scores_on_gemm) TRY(launch_text_cls_norm(sa, st));
    else TRY(launch_sidekick(sa, st, half_native));
  }
  // Gate first, expert product second (model.py:531-543): `vid * all_weight` is zero outside the top-k blocks, so the rows of
  // W1 . vid under a closed gate are never used -- with every query of a video in THIS chunk (nq <= max_batch) the gate of all of them
  // is known before the expert GEMMs start, and a row tile that none of the video's queries keeps is skipped (GemmArgs::tile_skip).
  // One query per video: the gate keeps int(0.3 n) of n blocks of `sn` clips, ~half of the 64-row tiles touch none of them;
  // q queries: ~0.5^q of the tiles (independent gates).  Several chunks of queries / the externally gated forward: every tile.
  const int nflags = (T0 + 63) / 64;
  static const Setting no_gate_skip(nullptr, "DCF_NO_GATE_SKIP", 0, Setting::PRESENT);        // developer switch: every row tile of the expert product
  const bool gate_first = !fc.gate && nq <= Bmax && m->vid_w1 && m->gemm_terms != 0 && !no_gate_skip.get() && debug_option("gate_skip", 1) != 0;
  unsigned long long vmap0 = 0;
  for (int i = 0; i < nq && i < 16; ++i) vmap0 |= (unsigned long long)video_of[i] << (4 * i);
  {
    // the deep and shallow halves of vid_map of every video have the same shape: three of them share a grid (blockIdx.z
    // selects the operand set), so five videos are four full launches instead of five two-thirds-full ones
    GemmArgs g[3];
    int ng = 0;
    auto flush = [&]() -> int {
      if (ng == 0) return 0;
      for (int i = 0; i < ng; ++i) { g[i].ldw = m->vid_ldw; g[i].a_scale = 1.f; }
      const int rc = run_gemm(m, g, ng, half_native ? A_CHANMAJOR_H : A_CHANMAJOR, st);
      ng = 0;
      return rc;
    };
    auto shallow_half = [&](int v) -> int {
      g[ng] = gemm(vs.shallow[v], T0, m->vid_w2, nullptr, b.P2 + (size_t)v * T0 * E, E, T0, E, D);
      if (scores_on_gemm) {
        g[ng].score_tn = b.tn + (size_t)q_of[v] * D; g[ng].score_out = b.correl + (size_t)q_of[v] * T0;
        g[ng].score_nq = vs.nq[v]; g[ng].score_norm = c.norm;
      }
      if (++ng == 3) return flush();
      return 0;
    };
    auto expert_half = [&](int v, bool skip) -> int {
      g[ng] = gemm(vs.vid[v], T0, m->vid_w1, nullptr, b.P1 + (size_t)v * T0 * E, E, T0, E, D);
      if (skip) { g[ng].tile_skip = b.tile_flags + (size_t)q_of[v] * nflags; g[ng].skip_nq = vs.nq[v]; g[ng].skip_stride = nflags; }
      if (++ng == 3) return flush();
      return 0;
    };
    auto gather_masks = [&]() -> int {
      if (nvid > 1) TRY(launch_gather_masks(vs.mask, nvid, b.maskv, T0, st));
      return 0;
    };
    if (gate_first) {
      if (m->vid_w2) for (int v = 0; v < nvid; ++v) TRY(shallow_half(v));
      TRY(flush());
      TRY(gather_masks());
      GateArgs ga{b.correl, nvid > 1 ? b.maskv : vid_mask, b.gate, sv > 1 ? b.mask_pre : b.mask_all, T0, nq, 0, c.sn, c.msf, (double)c.sratio, vmap0,
                  b.tile_flags, nflags};
      TRY(launch_gate(ga, st));
      // the expert halves of ALL videos in one grid where the operands allow it: the ~half of the row tiles that survive the gates
      // then fill the chip once (three launches of three videos each took as long as without the gate: a 64 x 256 tile is bound
      // by the latency of its 32 K steps, not by how many tiles run beside it)
      auto wit = m->wsplit.find(m->vid_w1);
      const bool one_grid = nvid > 1 && nvid <= GEMM_ZMAX && E % 256 == 0 && T0 % 4 == 0 && wit != m->wsplit.end() && m->wsplit_ldw[m->vid_w1] == m->vid_ldw;
      if (one_grid) {
        GemmArgs base = gemm(vs.vid[0], T0, m->vid_w1, nullptr, b.P1, E, T0, E, D);
        base.ldw = m->vid_ldw; base.a_scale = 1.f; base.Ws = wit->second; base.status = m->status; base.skip_stride = nflags;
        const float* zA[GEMM_ZMAX]; float* zC[GEMM_ZMAX]; const uint8_t* zs[GEMM_ZMAX]; int zq[GEMM_ZMAX];
        for (int v = 0; v < nvid; ++v) { zA[v] = vs.vid[v]; zC[v] = b.P1 + (size_t)v * T0 * E; zs[v] = b.tile_flags + (size_t)q_of[v] * nflags; zq[v] = vs.nq[v]; }
        // the profile prices this launch at the clips the gate keeps at least -- int(sratio n) of n blocks -- not at the full product:
        // the tiles it skips are work the reference does (on zeros) and this kernel does not
        TRY(launch_gemm_split_z(base, nvid, zA, zC, zs, zq, m->wsplit_terms[m->vid_w1], st, std::min(1.0, std::max(0.0, (double)c.sratio)),
                                half_native ? A_CHANMAJOR_H : A_CHANMAJOR));
      } else {
        for (int v = 0; v < nvid; ++v) TRY(expert_half(v, true));
        TRY(flush());
      }
    } else {
      for (int v = 0; v < nvid; ++v) {
        if (m->vid_w1 && !sel) TRY(expert_half(v, false));
        if (m->vid_w2) TRY(shallow_half(v));
      }
      TRY(flush());
      TRY(gather_masks());
      if (sel) {
        // P1c (n_rows, E) = vid_rows . W1^T into the first n_rows rows of P1: a row-major GEMM on the same weight image; every row is
        // needed by construction, so no tile is skipped
        GemmArgs ge = gemm(fc.sel_rows, D, m->vid_w1, nullptr, b.P1, E, fc.sel_n, E, D);
        ge.ldw = m->vid_ldw; ge.a_scale = 1.f;
        TRY(run_gemm(m, &ge, 1, A_ROWS, st));        // (several videos: ONE product over the packed rows of all of them)
      }
    }
  }
  if (nvid > 1) vid_mask = b.maskv;

  for (int q0 = 0; q0 < nq; q0 += Bmax) {
    const int B = std::min(Bmax, nq - q0);
    Plan* pl;
    TRY(get_plan(m, Tp, B, L, st, &pl));
    const LevelTable& lt = pl->lt;
    const int rows0 = B * T0, rowsP = B * Tp, rowsAll = B * S;
    uint8_t* mask_in = sv > 1 ? b.mask_pre : b.mask_all;      // validity of the T0 input clips (gate stage)
    if (m->drop) m->drop->b0 = q0;
    unsigned long long vmap = 0;           // video of batch element i in nibble i (B <= 16 with several videos, <= 16 videos)
    for (int i = 0; i < B && i < 16; ++i) vmap |= (unsigned long long)video_of[q0 + i] << (4 * i);

    // ---- gate + masks for every level
    if (fc.gate) {
      // T-sharded videos: the gate was selected globally (all-gathered scores) by the caller
      hipLaunchKernelGGL(k_apply_gate, dim3((rows0 + 255) / 256), dim3(256), 0, st, fc.gate + (int64_t)q0 * T0, vid_mask,
                         b.gate, mask_in, T0, rows0, c.msf, vmap);
      DCF_HIP(hipGetLastError());
    } else if (!gate_first) {                      // (gate_first: selected in front of the expert products, above)
      GateArgs ga{b.correl, vid_mask, b.gate, mask_in, T0, B, q0, c.sn, c.msf, (double)c.sratio, vmap, nullptr, 0};
      TRY(launch_gate(ga, st));
    }
    int pre_off = 0;                              // first row of the last input-resolution level (= pyramid level 0) in mask_pre
    if (sv > 1) {
      int rows_pre = 0;
      for (int j = 0; j <= npre; ++j) { if (j == npre) pre_off = rows_pre; rows_pre += B * (T0 >> j); }
      TRY(launch_pyramid_masks(b.mask_pre, b.nbr_pre, B, T0, npre + 1, rows_pre, st));       // mask_j[i] = mask_0[i << j] (blocks.py:101-105)
      DCF_HIP(hipMemcpyAsync(b.mask_all, b.mask_pre + pre_off, (size_t)rowsP, hipMemcpyDeviceToDevice, st));
    }
    TRY(launch_pyramid_masks(b.mask_all, b.nbr_all, B, Tp, L, rowsAll, st));
    const uint8_t* mask0 = mask_in;               // input clips: vid_map, early fusion, embd_fc
    const uint8_t* maskP = b.mask_all;            // pyramid level 0

    // ---- vid_map (model.py:543-555)
    if (sel) TRY(launch_vidmap_combine_sel(b.P1, fc.sel_pos, sel_first, m->vid_w2 ? b.P2 : nullptr, m->vid_map_b, b.gate, mask0, m->vid_w3,
                                           m->vid_w3 ? fc.sel_correl + (int64_t)q0 * T0 : nullptr, b.X, T0, rows0, E, vmap, st));
    else
    TRY(launch_vidmap_combine(m->vid_w1 ? b.P1 : nullptr, m->vid_w2 ? b.P2 : nullptr, m->vid_map_b, b.gate, mask0,
                              m->vid_w3, m->vid_w3 ? b.correl + (int64_t)q0 * T0 : nullptr, b.X, T0, rows0, E, vmap, st));
    if (m->keep_debug) DCF_CHECK((int64_t)rows0 * E <= m->dbg_cap, "dcf_debug_copy: armed destination holds %lld floats, the tap needs %lld", (long long)m->dbg_cap, (long long)rows0 * E);
    if (m->keep_debug && m->dbg_vidmap) DCF_HIP(hipMemcpyAsync(m->dbg_vidmap, b.X, (size_t)rows0 * E * 4, hipMemcpyDeviceToDevice, st));

    // ---- text side: pointers of this chunk
    // the kernels take the pointers by value (kernel argument): a captured graph bakes them in, which is what its key
    // (every text pointer and length) promises
    TextMeta tm{};
    for (int i = 0; i < B; ++i) {
      tm.text[i] = fc.text[q0 + i];
      tm.text_mask[i] = fc.text_mask ? fc.text_mask[q0 + i] : nullptr;
      tm.len[i] = fc.text_len[q0 + i];
    }
    const TextMeta* dm = &tm;

    // ---- early fusion: XAttNFusion on the level-0 sequence (fusion.py:56-66)
    bool fused_as_stats = false;                  // fusion.ln_out carried into vid_net.embd_fc as row statistics
    if (c.model_kind != 1) {
      const bool tap = m->keep_debug && m->dbg_fused;    // the `fused` debug tap wants the normalised rows themselves
      if (m->drop) TRY(run_fusion_drop(m, b, b.X, E, B, T0, mask0, dm, Lk, b.R[0], E, st));
      else TRY(run_fusion(m, b, b.X, E, B, T0, nullptr, mask0, nullptr, dm, Lk, b.R[0], E, st, tap ? nullptr : &fused_as_stats));
      if (tap) DCF_HIP(hipMemcpyAsync(m->dbg_fused, b.R[0], (size_t)rows0 * E * 4, hipMemcpyDeviceToDevice, st));
    }

    // ---- vid_net: VideoTransformer.forward (video_net.py:123-164)
    {
      const bool chain_embd = can_chain_embd(m, rows0);
      if (chain_embd) {
        // embd_fc, both embedding convolutions, their LayerNorms and + pe * mask in one kernel: from the raw stream in b.X where
        // fusion.ln_out came as row statistics (the kernel normalises its rows itself), from the normalised rows in R[0] otherwise.
        // Not in place: neighbouring windows read each other's halo rows.
        TRY(run_embd_chain(m, fused_as_stats ? b.X : b.R[0], E, b.nbr_all, rows0, T0, fused_as_stats, c.use_abs_pe ? m->pe : nullptr, b.R[3], E, st));
        std::swap(b.X, b.R[3]);
      } else
      if (c.model_kind != 1 && fused_as_stats) {
        // embd_fc(ln_out(x) * mask) from the raw x in b.X: padded rows come out as finite garbage instead of the bias, and every
        // consumer masks its input rows (blocks.py:98-99).  Not in place: column tiles of other workgroups still read b.X.
        GemmArgs ge = gemm(b.X, E, m->embd_fc_wf, m->embd_fc_c, b.R[3], E, rows0, E, E);
        ge.flags = G_AMASK; ge.rowmask = mask0;
        ge.stats_in = b.stats; ge.ln_s = m->embd_fc_s; ge.stats_slots = E / STATS_W; ge.stats_w = STATS_W;
        TRY(run_gemm(m, &ge, 1, A_ROWS, st));
        std::swap(b.X, b.R[3]);
      } else if (c.model_kind != 1) {
        GemmArgs ge = gemm(b.R[0], E, m->embd_fc_w, m->embd_fc_b, b.X, E, rows0, E, E);
        ge.flags = G_AMASK; ge.rowmask = mask0;
        TRY(run_gemm(m, &ge, 1, A_ROWS, st));
      }   // late fusion (PtTransformer): b.X already IS embd_fc([gate*vid ; shallow] * mask), model.py:132-140
      if (sv > 1) {
        // vid_net.stride > 1 (video_net.py:62-73): while the sequence is longer than the pyramid's, a convolution is k5 / stride 2 /
        // padding 2 on the masked input -- its five taps gathered into rows [B T/2][5E] and one plain GEMM --, then k3 as usual; every
        // one followed by LayerNorm + ReLU, the last one by + pe * mask (video_net.py:136-152)
        int Tc = T0, off = 0;
        for (int i = 0; i < c.n_embd_convs; ++i) {
          const bool with_pe = c.use_abs_pe && i == c.n_embd_convs - 1;
          if (Tc > Tp) {
            TRY(launch_im2col5s2(b.X, E, b.mask_pre + off, b.col5, B, Tc, E, st));
            GemmArgs g = gemm(b.col5, 5 * E, m->embd_conv[i], nullptr, b.R[0], E, B * (Tc / 2), E, 5 * E);
            TRY(run_gemm(m, &g, 1, A_ROWS, st));
            off += B * Tc;
            Tc /= 2;
          } else {
            GemmArgs g = gemm(b.X, E, m->embd_conv[i], nullptr, b.R[0], E, B * Tc, E, 3 * E);
            g.cin = E; g.nbr = b.nbr_pre + off;
            TRY(run_gemm(m, &g, 1, A_ROWS_TAP3, st));
          }
          LnArgs ln{}; ln.X = b.R[0]; ln.ldx = E; ln.Y = b.X; ln.ldy = E; ln.w = m->embd_ln_w[i]; ln.b = m->embd_ln_b[i];
          ln.rows = B * Tc; ln.C = E; ln.relu = 1;
          if (with_pe) { ln.pe = m->pe; ln.mask = b.mask_pre + off; ln.T = Tc; }
          TRY(launch_ln(ln, st));
        }
        DCF_CHECK(Tc == Tp, "vid_net.arch[0]=%d embedding convolutions cannot divide the sequence by vid_net.stride=%d (video_net.py:53)", c.n_embd_convs, sv);
      }
      int epend = -1, epend_w = 0;                  // embedding layer whose LayerNorm + ReLU the next convolution applies on load
      for (int i = 0; i < c.n_embd_convs && sv == 1 && !chain_embd; ++i) {
        GemmArgs g = gemm(b.X, E, m->embd_conv[i], nullptr, b.R[0], E, rows0, E, 3 * E);
        g.cin = E; g.nbr = b.nbr_all;
        const bool with_pe = c.use_abs_pe && i == c.n_embd_convs - 1;
        int sw = 0;
        if (epend >= 0) {
          // A = the RAW output of the previous convolution (in R[0]); this one writes to R[3] (a level-0 sized scratch that no
          // fusion pass uses) and the LayerNorm reads it from there.  The buffers are NOT swapped: R[0..2] hold rowsF rows (the
          // whole pyramid with late / second fusion), R[3..6] only the level-0 rows.
          g.A = b.R[0]; g.C = b.R[3];
          norm_a(g, b.hstats[0], E, epend_w, m->embd_ln_w[epend], m->embd_ln_b[epend]);
          epend = -1;
          TRY(run_gemm(m, &g, 1, A_ROWS_TAP3, st));
          LnArgs ln{}; ln.X = b.R[3]; ln.ldx = E; ln.Y = b.X; ln.ldy = E; ln.w = m->embd_ln_w[i]; ln.b = m->embd_ln_b[i];
          ln.rows = rows0; ln.C = E; ln.relu = 1;
          if (with_pe) { ln.pe = m->pe; ln.mask = mask0; ln.T = T0; }
          TRY(launch_ln(ln, st));
        } else if (i + 1 < c.n_embd_convs && i + 2 == c.n_embd_convs && can_norm_a(m, m->embd_conv[i], m->embd_conv[i + 1], rows0, E, &sw)) {
          g.stats_out = b.hstats[0]; g.stats_w = sw;                 // raw output (R[0]) + row statistics; no LayerNorm launch
          TRY(run_gemm(m, &g, 1, A_ROWS_TAP3, st));
          epend = i; epend_w = sw;
        } else
        if (can_fuse_ln(m, m->embd_conv[i], rows0, E, 3 * E, A_ROWS_TAP3)) {
          // conv -> LN -> ReLU (+ pe * mask) in one kernel; the result goes to R[3] (same size as X) because the k3
          // taps of other workgroups still read X, then X and R[3] swap roles
          g.C = nullptr; g.ln_w = m->embd_ln_w[i]; g.ln_b = m->embd_ln_b[i]; g.Y = b.R[3]; g.ldy = E; g.ln_relu = 1;
          if (with_pe) { g.ln_pe = m->pe; g.ln_mask = mask0; g.ln_T = T0; }
          TRY(run_gemm(m, &g, 1, A_ROWS_TAP3, st));
          std::swap(b.X, b.R[3]);
        } else {
          TRY(run_gemm(m, &g, 1, A_ROWS_TAP3, st));
          LnArgs ln{}; ln.X = b.R[0]; ln.ldx = E; ln.Y = b.X; ln.ldy = E; ln.w = m->embd_ln_w[i]; ln.b = m->embd_ln_b[i];
          ln.rows = rows0; ln.C = E; ln.relu = 1;
          if (with_pe) { ln.pe = m->pe; ln.mask = mask0; ln.T = T0; }
          TRY(launch_ln(ln, st));
        }
      }
      if (c.use_abs_pe && c.n_embd_convs == 0) {
        LnArgs ln{}; ln.X = b.X; ln.ldx = E; ln.Y = b.X; ln.ldy = E; ln.rows = rows0; ln.C = E; ln.skip_ln = 1;
        ln.pe = m->pe; ln.mask = mask0; ln.T = T0;
        TRY(launch_ln(ln, st));
      }
      for (size_t i = 0; i < m->stem.size(); ++i) {
        // stem layers work in place at level 0: out -> R[3] is free for stride 1, then copy back via swap of roles
        if (m->drop) TRY(run_encoder_drop(m, m->stem[i], b, b.X, E, maskP, maskP, B, Tp, 1, b.R[3], E, drop_site(DROP_G_STEM, (uint32_t)i, 0), st));
        else TRY(run_encoder(m, m->stem[i], b, b.X, E, maskP, maskP, B, Tp, 1, b.R[3], E, st));
        DCF_HIP(hipMemcpyAsync(b.X, b.R[3], (size_t)rowsP * E * 4, hipMemcpyDeviceToDevice, st));
      }
      const int ldf = E + TCN_HID;
      const float* xin = b.X;
      int64_t ldx = E;
      for (int l = 0; l < L; ++l) {
        const int stride = l > 0 ? 2 : 1;
        const uint8_t* mi = b.mask_all + lt.start[l > 0 ? l - 1 : 0];
        const uint8_t* mo = b.mask_all + lt.start[l];
        float* xo = b.F + (int64_t)lt.start[l] * ldf;
        if (c.pool_only) TRY(launch_dwconv3(xin, ldx, mi, m->pool_w[l], xo, ldf, B, l > 0 ? lt.T[l - 1] : Tp, stride, E, st));   // video_net.py:107-109
        else if (m->drop) TRY(run_encoder_drop(m, m->branch[l], b, xin, ldx, mi, mo, B, l > 0 ? lt.T[l - 1] : Tp, stride, xo, ldf,
                                               drop_site(DROP_G_BRANCH, (uint32_t)l, 0), st));
        else TRY(run_encoder(m, m->branch[l], b, xin, ldx, mi, mo, B, l > 0 ? lt.T[l - 1] : Tp, stride, xo, ldf, st));
        xin = xo; ldx = ldf;
      }
    }

    if (m->hyb_levels > 0) {                      // dcf_hybrid_phase1: the pyramid stands up to level k; hand it over and stop
      TRY(hybrid_take(m, b, *pl, B, Lk, st));
      continue;
    }

    // ---- second / late fusion over the whole pyramid (model.py:443-444, :66-67; fusion.py:68-78), in place on F
    if (c.model_kind == 1 || c.second_fusion)
      TRY(run_fusion(m, b, b.F, E + TCN_HID, B, Tp, &lt, b.mask_all, b.nbr_all, dm, Lk, b.F, E + TCN_HID, st));

    if (c.model_kind != 0) {
      // ---- PtTransformer / PtTransformerEarlyFusion.fuse_and_predict (model.py:65-69, :204-209): cls_head / reg_head on the pyramid
      TRY(run_head_pair(m, m->cls1, m->reg, b, *pl, E, 1, 0, fc.logits + (int64_t)q0 * S, 2, 1, fc.offsets + (int64_t)q0 * S * 2, st));
    } else {
    // ---- heads: fuse_and_predict (model.py:442-471)
    TRY(run_head(m, m->cls1, b, *pl, E, 1, 0, 0, b.logits1, st));
    if (vs.logits1_out) {
      hipLaunchKernelGGL(k_points_out, dim3((rowsAll + 255) / 256), dim3(256), 0, st, (const float*)b.logits1,
                         vs.logits1_out + (int64_t)q0 * S, (const LevelTable*)pl->d_lt);
      DCF_HIP(hipGetLastError());
    }
    {
      RefineArgs ra = refine_args(m);
      ra.logits1 = b.logits1; ra.lt = pl->d_lt; ra.mask_all = b.mask_all;
      ra.bufA = b.tcnA; ra.bufB = b.tcnB; ra.F = b.F; ra.ldf = E + TCN_HID; ra.E = E;
      ra.B = B; ra.T0 = Tp; ra.n_levels = L; ra.n_layers = L;
      if (m->drop) {
        ra.drop_seed = m->drop->seed; ra.drop_p = m->drop->p[DROP_R_REFINE]; ra.drop_scale = m->drop->scale[DROP_R_REFINE]; ra.drop_b0 = q0;
      }
      TRY(launch_refine(ra, lt, st));
    }
    TRY(run_head_pair(m, m->cls2, m->reg, b, *pl, E + TCN_HID, 1, 0, fc.logits + (int64_t)q0 * S, 2, 1,
                      fc.offsets + (int64_t)q0 * S * 2, st));
    }
    launch_masks_out(b.mask_all, fc.masks + (int64_t)q0 * S, pl->d_lt, m->status, fc.logits + (int64_t)q0 * S, rowsAll, st);
    DCF_HIP(hipGetLastError());

    m->dbg.correl = b.correl; m->dbg.gate = b.gate; m->dbg.F = b.F;
    m->dbg.nq = nq; m->dbg.T0 = T0; m->dbg.B = B; m->dbg.S = S;
  }
  m->keep_debug = false;                      // the taps of dcf_debug_copy(2 / 3) fill once
  m->dbg_vidmap = m->dbg_fused = nullptr;
  return 0;
}

// TextTransformer.forward (text_net.py:158-188) for one query: embd_fc 1x1 on x * mask, + pe * mask, background
// token, n x TransformerEncoder(stride 0) (blocks.py:578-591 with global MaskedMHA, blocks.py:374-393).
// tokens (C_t, Lq) channel-major -> text_out (TE, Lk) channel-major (the layout dcf_forward_eval takes), Lk = Lq + bkgd.
static int text_encode(dcf_model* m, const float* tokens, const uint8_t* token_mask, int Lq, float* text_out, uint8_t* mask_out,
                       hipStream_t st) {
  const dcf_config& c = m->cfg;
  DCF_CHECK(m->finalized, "dcf_text_encode: model not finalized");
  DCF_CHECK(m->text_embd_w || c.text_kind == 1, "dcf_text_encode: the model was created without a text encoder (text_in / text_layers = 0)");
  DCF_CHECK(Lq >= 1 && tokens && text_out && mask_out, "dcf_text_encode: bad arguments");
  const int TE = c.TE, Lk = Lq + (c.text_bkgd ? 1 : 0);
  if (c.text_abs_pe) DCF_CHECK(m->text_pe && m->text_pe_L >= Lq, "text position encoding for %d tokens not set (dcf_model_set_text_pe)", Lq);
  // workspace: X, X2, R0, Q, K, V [Lk][TE]; HID [Lk][4 TE]
  const size_t rowB = ((size_t)Lk * TE * sizeof(float) + 255) & ~(size_t)255;
  const size_t need = 10 * rowB;
  if (need > m->text_ws_bytes) {
    DCF_HIP(hipStreamSynchronize(st));
    if (m->text_ws) DCF_HIP(hipFree(m->text_ws));
    m->text_ws = nullptr; m->text_ws_bytes = 0;
    DCF_HIP(hipMalloc(&m->text_ws, need));
    m->text_ws_bytes = need;
  }
  auto buf = [&](int i) { return reinterpret_cast<float*>(m->text_ws + (size_t)i * rowB); };
  float *X = buf(0), *X2 = buf(1), *R0 = buf(2), *Q = buf(3), *K = buf(4), *V = buf(5), *HID = buf(6);   // HID spans 4 slots

  TextEmbedArgs te{tokens, token_mask, m->text_embd_w, m->text_embd_b, c.text_abs_pe ? m->text_pe : nullptr, m->text_bkgd, X, mask_out,
                   c.text_in, Lq, TE, (c.text_kind == 1 && c.text_bkgd) ? 1 : 0};
  TRY(launch_text_embed(te, st));
  if (c.text_kind == 1) {
    if (c.text_bkgd) {
      // AttNPool1D (blocks.py:396-411): h = [masked mean ; x], pooled token = MaskedMHA(h, kv_mask)[..., :1], out = [pool ; x]
      const TextEncW& w = m->text_pool;
      GemmArgs g3[3] = {gemm(X, TE, w.wq, w.bq, Q, TE, Lk, TE, TE), gemm(X, TE, w.wk, w.bk, K, TE, Lk, TE, TE),
                        gemm(X, TE, w.wv, w.bv, V, TE, Lk, TE, TE)};
      TRY(run_gemm(m, g3, 3, A_ROWS, st));
      XAttnArgs xa{Q, K, V, mask_out, R0, 1, Lk, Lk, TE, c.text_heads, m->status};
      TRY(launch_xattn(xa, st));
      GemmArgs gp = gemm(R0, TE, w.wp, w.bp, X, TE, 1, TE, TE);                       // only the pooled row is kept
      TRY(run_gemm(m, &gp, 1, A_ROWS, st));
    }
    TRY(launch_rows_to_chanmajor(X, text_out, Lk, TE, st));
    return 0;
  }
  for (const TextEncW& w : m->text_enc) {
    TRY(launch_mask_rows(X, mask_out, Lk, TE, st));                                   // x = x * mask   (blocks.py:581)
    LnArgs ln{}; ln.X = X; ln.ldx = TE; ln.Y = R0; ln.ldy = TE; ln.w = w.ln_attn_w; ln.b = w.ln_attn_b; ln.rows = Lk; ln.C = TE;
    TRY(launch_ln(ln, st));
    GemmArgs g3[3] = {gemm(R0, TE, w.wq, w.bq, Q, TE, Lk, TE, TE), gemm(R0, TE, w.wk, w.bk, K, TE, Lk, TE, TE),
                      gemm(R0, TE, w.wv, w.bv, V, TE, Lk, TE, TE)};
    TRY(run_gemm(m, g3, 3, A_ROWS, st));
    XAttnArgs xa{Q, K, V, mask_out, R0, 1, Lk, Lk, TE, c.text_heads, m->status};                   // softmax over the valid tokens
    TRY(launch_xattn(xa, st));
    GemmArgs gp = gemm(R0, TE, w.wp, w.bp, X2, TE, Lk, TE, TE);                        // x = skip * mask + ls * proj(ctx)
    gp.flags = G_RES; gp.R = X; gp.ldr = TE; gp.ls = w.ls_attn;
    TRY(run_gemm(m, &gp, 1, A_ROWS, st));
    LnArgs l2{}; l2.X = X2; l2.ldx = TE; l2.Y = R0; l2.ldy = TE; l2.w = w.ln_ffn_w; l2.b = w.ln_ffn_b; l2.rows = Lk; l2.C = TE;
    TRY(launch_ln(l2, st));
    GemmArgs gf = gemm(R0, TE, w.fc_w, w.fc_b, HID, 4 * TE, Lk, 4 * TE, TE);
    gf.flags = G_GELU;
    TRY(run_gemm(m, &gf, 1, A_ROWS, st));
    GemmArgs go = gemm(HID, 4 * TE, w.pj_w, w.pj_b, X, TE, Lk, TE, 4 * TE);             // x += ls * (ffn * mask)
    go.flags = G_RES | G_OUT_MASK; go.rowmask = mask_out; go.R = X2; go.ldr = TE; go.ls = w.ls_ffn;
    TRY(run_gemm(m, &go, 1, A_ROWS, st));
  }
  TRY(launch_rows_to_chanmajor(X, text_out, Lk, TE, st));
  return 0;
}

}  // namespace dcf

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" {

const char* dcf_last_error(void) { return dcf::last_error(); }
int dcf_abi_version(void) { return 12; }

namespace dcf {
// eager on the first call with a given argument set, capture + replay from the second identical call on
static int forward_graph_on(dcf_model* m, const VideoSet& vs, int T0, int nq, const ForwardCall& fc, hipStream_t st) {
  std::vector<uint64_t> key = {(uint64_t)vs.nvid, (uint64_t)T0, (uint64_t)nq, (uint64_t)vs.logits1_out,
                               (uint64_t)fc.gate, (uint64_t)fc.logits, (uint64_t)fc.offsets, (uint64_t)fc.masks, (uint64_t)st, (uint64_t)m->pe, (uint64_t)m->pe_T,
                               (uint64_t)(vs.half ? 1 : 0)};      // (the operand type of vid / shallow: an fp32 and a half forward never share a graph;
                                                                  //  the half_native option needs no slot: every dcf_debug_set_option bumps option_epoch,
                                                                  //  and forward_maybe_graph drops the captured graph before it gets here)
  for (int v = 0; v < vs.nvid; ++v) {
    key.push_back((uint64_t)vs.vid[v]); key.push_back((uint64_t)vs.shallow[v]); key.push_back((uint64_t)vs.mask[v]);
    key.push_back((uint64_t)vs.text_cls[v]); key.push_back((uint64_t)vs.nq[v]);
  }
  for (int q = 0; q < nq; ++q) {
    key.push_back((uint64_t)fc.text[q]);
    key.push_back(fc.text_mask ? (uint64_t)fc.text_mask[q] : 0);
    key.push_back((uint64_t)fc.text_len[q]);
  }
  m->last_launch = 0;
  if (m->graph_exec && key == m->graph_key) {
    DCF_HIP(hipGraphLaunch(m->graph_exec, st));
    m->last_launch = 1;
    return 0;
  }
  if (key != m->last_key || key == m->nocapture_key) {   // first sighting (allocates workspace / plans), or known not to capture
    m->last_key = key;
    return forward(m, vs, T0, nq, fc, st);
  }
  // second identical call: capture
  drop_graph(m);
  m->last_key = key;
  if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) != hipSuccess) {
    (void)hipGetLastError();
    m->nocapture_key = key;
    return forward(m, vs, T0, nq, fc, st);
  }
  m->capturing = true;
  const int rc = forward(m, vs, T0, nq, fc, st);
  m->capturing = false;
  hipGraph_t g = nullptr;
  const hipError_t ec = hipStreamEndCapture(st, &g);
  if (rc != 0 || ec != hipSuccess || !g) {           // capture failed: nothing ran; fall back to an eager forward
    (void)hipGetLastError();
    if (g) (void)hipGraphDestroy(g);
    m->nocapture_key = key;
    const std::string err = last_error();
    const int rc2 = forward(m, vs, T0, nq, fc, st);
    if (rc2 != 0 && !err.empty()) set_error("%s", err.c_str());
    return rc2;
  }
  hipGraphExec_t ge = nullptr;
  if (hipGraphInstantiate(&ge, g, nullptr, nullptr, 0) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipGraphDestroy(g);
    m->nocapture_key = key;
    return forward(m, vs, T0, nq, fc, st);
  }
  m->graph = g;
  m->graph_exec = ge;
  m->graph_key = key;
  DCF_HIP(hipGraphLaunch(ge, st));
  m->last_launch = 2;
  return 0;
}

static int forward_maybe_graph(dcf_model* m, const VideoSet& vs, int T0, int nq, const ForwardCall& fc, hipStream_t st) {
  static const Setting no_graph(nullptr, "DCF_NO_GRAPH", 0, Setting::PRESENT);
  if (m->hyb) m->hyb->valid = false;              // whatever way this forward is issued (a graph replay does not pass through forward())
  if (m->option_epoch != option_epoch()) { drop_graph(m); m->option_epoch = option_epoch(); }
  // Auto: replay a graph only for forwards of >= 64 K level-0 rows.  Measured on MI355X (profiles/r03_notes.md): the batched
  // forward runs at the same speed either way (25.36 vs 25.35 ms per 24-video step) and the graph shields it from host
  // jitter; ONE video per call (~100 launches of 5 - 40 us) is 5 % faster launched eagerly (1.75 vs 1.84 ms: a graph node
  // costs ~0.9 us more than an in-order launch, and the host needs ~0.5 ms to issue the forward the GPU takes 1.75 ms for).
  const bool want = m->graph_mode == 1 || (m->graph_mode == 0 && (long long)nq * T0 >= 65536);
  // (dropout: eager, the seed is a kernel argument that a captured graph would bake in)
  // (the selected-clip forward: eager, its row count and row pointers are no part of a graph's key)
  const bool eligible = want && !no_graph.get() && !profiling_on() && !m->keep_debug && nq > 0 && !m->drop && !fc.sel_rows;
  if (!eligible) {
    m->last_launch = 0;
    return forward(m, vs, T0, nq, fc, st);
  }
  if (st != nullptr) return forward_graph_on(m, vs, T0, nq, fc, st);
  // legacy default stream: hop to the engine's own stream (see dcf_model::own)
  if (!m->own) {
    DCF_HIP(hipStreamCreateWithFlags(&m->own, hipStreamNonBlocking));
    DCF_HIP(hipEventCreateWithFlags(&m->ev_in, hipEventDisableTiming));
    DCF_HIP(hipEventCreateWithFlags(&m->ev_out, hipEventDisableTiming));
  }
  DCF_HIP(hipEventRecord(m->ev_in, st));
  DCF_HIP(hipStreamWaitEvent(m->own, m->ev_in, 0));
  const int rc = forward_graph_on(m, vs, T0, nq, fc, m->own);
  DCF_HIP(hipEventRecord(m->ev_out, m->own));
  DCF_HIP(hipStreamWaitEvent(st, m->ev_out, 0));
  return rc;
}

// the videos of a multi-video entry point `what` into vs; *nq_out = the queries of all of them
static int fill_videos(VideoSet& vs, const char* what, int nvid, const float* const* vid, const float* const* shallow_vid,
                       const uint8_t* const* vid_mask, const float* const* text_cls, const int32_t* nq_per_video, int* nq_out) {
  vs.nvid = nvid;
  int nq = 0;
  for (int v = 0; v < nvid; ++v) {
    DCF_CHECK(vid[v] && shallow_vid[v] && vid_mask[v] && text_cls[v] && nq_per_video[v] >= 1, "%s: video %d is incomplete", what, v);
    vs.vid[v] = vid[v]; vs.shallow[v] = shallow_vid[v]; vs.mask[v] = vid_mask[v]; vs.text_cls[v] = text_cls[v]; vs.nq[v] = nq_per_video[v];
    nq += nq_per_video[v];
  }
  *nq_out = nq;
  return 0;
}
}  // namespace dcf

int dcf_text_encode(dcf_model* m, const float* tokens, const uint8_t* token_mask, int32_t Lq, float* text_out, uint8_t* mask_out,
                    void* stream) {
  DCF_CHECK(m, "dcf_text_encode: null model");
  return dcf::text_encode(m, tokens, token_mask, Lq, text_out, mask_out, (hipStream_t)stream);
}

int64_t dcf_points_per_query(const dcf_model* m, int64_t T) {
  int64_t s = 0;
  const int64_t Tp = T / dcf::vid_stride_of(m->cfg);     // the pyramid starts behind the strided embedding convolutions
  for (int l = 0; l < m->cfg.n_levels; ++l) s += Tp >> l;
  return s;
}

int dcf_forward_eval(dcf_model* m, const float* vid, const float* shallow_vid, const uint8_t* vid_mask, int64_t T,
                     int32_t nq, const float* const* text, const uint8_t* const* text_mask, const int32_t* text_len,
                     const float* text_cls, float* logits_out, float* offsets_out, uint8_t* masks_out, void* stream) {
  DCF_CHECK(m && vid && shallow_vid && vid_mask && text && text_len && text_cls && logits_out && offsets_out && masks_out,
            "dcf_forward_eval: null argument");
  DCF_CHECK(T < (1ll << 24), "T too large");
  dcf::VideoSet vs;
  vs.nvid = 1; vs.vid[0] = vid; vs.shallow[0] = shallow_vid; vs.mask[0] = vid_mask; vs.text_cls[0] = text_cls; vs.nq[0] = nq;
  return dcf::forward_maybe_graph(m, vs, (int)T, nq, {text, text_mask, text_len, nullptr, logits_out, offsets_out, masks_out},
                                  (hipStream_t)stream);
}

int dcf_forward_eval_videos(dcf_model* m, int32_t nvid, const float* const* vid, const float* const* shallow_vid,
                            const uint8_t* const* vid_mask, int64_t T, const int32_t* nq_per_video, const float* const* text,
                            const uint8_t* const* text_mask, const int32_t* text_len, const float* const* text_cls,
                            float* logits_out, float* offsets_out, uint8_t* masks_out, void* stream) {
  DCF_CHECK(m && vid && shallow_vid && vid_mask && nq_per_video && text && text_len && text_cls && logits_out && offsets_out && masks_out,
            "dcf_forward_eval_videos: null argument");
  DCF_CHECK(nvid >= 1 && nvid <= dcf::DCF_MAX_VIDEOS, "dcf_forward_eval_videos: 1 .. %d videos per call", dcf::DCF_MAX_VIDEOS);
  DCF_CHECK(T < (1ll << 24), "T too large");
  dcf::VideoSet vs;
  int nq = 0;
  if (dcf::fill_videos(vs, "dcf_forward_eval_videos", nvid, vid, shallow_vid, vid_mask, text_cls, nq_per_video, &nq)) return -1;
  return dcf::forward_maybe_graph(m, vs, (int)T, nq, {text, text_mask, text_len, nullptr, logits_out, offsets_out, masks_out},
                                  (hipStream_t)stream);
}

int dcf_forward_eval_h(dcf_model* m, const uint16_t* vid, const uint16_t* shallow_vid, const uint8_t* vid_mask, int64_t T,
                       int32_t nq, const float* const* text, const uint8_t* const* text_mask, const int32_t* text_len,
                       const float* text_cls, float* logits_out, float* offsets_out, uint8_t* masks_out, void* stream) {
  DCF_CHECK(m && vid && shallow_vid && vid_mask && text && text_len && text_cls && logits_out && offsets_out && masks_out,
            "dcf_forward_eval_h: null argument");
  DCF_CHECK(T < (1ll << 24), "T too large");
  dcf::VideoSet vs;
  vs.nvid = 1; vs.vid[0] = reinterpret_cast<const float*>(vid); vs.shallow[0] = reinterpret_cast<const float*>(shallow_vid);
  vs.mask[0] = vid_mask; vs.text_cls[0] = text_cls; vs.nq[0] = nq; vs.half = true;
  return dcf::forward_maybe_graph(m, vs, (int)T, nq, {text, text_mask, text_len, nullptr, logits_out, offsets_out, masks_out},
                                  (hipStream_t)stream);
}

int dcf_forward_eval_videos_h(dcf_model* m, int32_t nvid, const uint16_t* const* vid, const uint16_t* const* shallow_vid,
                              const uint8_t* const* vid_mask, int64_t T, const int32_t* nq_per_video, const float* const* text,
                              const uint8_t* const* text_mask, const int32_t* text_len, const float* const* text_cls,
                              float* logits_out, float* offsets_out, uint8_t* masks_out, void* stream) {
  DCF_CHECK(m && vid && shallow_vid && vid_mask && nq_per_video && text && text_len && text_cls && logits_out && offsets_out && masks_out,
            "dcf_forward_eval_videos_h: null argument");
  DCF_CHECK(nvid >= 1 && nvid <= dcf::DCF_MAX_VIDEOS, "dcf_forward_eval_videos_h: 1 .. %d videos per call", dcf::DCF_MAX_VIDEOS);
  DCF_CHECK(T < (1ll << 24), "T too large");
  dcf::VideoSet vs;
  int nq = 0;
  if (dcf::fill_videos(vs, "dcf_forward_eval_videos_h", nvid, reinterpret_cast<const float* const*>(vid),
                       reinterpret_cast<const float* const*>(shallow_vid), vid_mask, text_cls, nq_per_video, &nq)) return -1;
  vs.half = true;
  return dcf::forward_maybe_graph(m, vs, (int)T, nq, {text, text_mask, text_len, nullptr, logits_out, offsets_out, masks_out},
                                  (hipStream_t)stream);
}

int dcf_forward_train_videos(dcf_model* m, int32_t nvid, const float* const* vid, const float* const* shallow_vid,
                             const uint8_t* const* vid_mask, int64_t T, const int32_t* nq_per_video, const float* const* text,
                             const uint8_t* const* text_mask, const int32_t* text_len, const float* const* text_cls,
                             float* logits1_out, float* logits2_out, float* offsets_out, uint8_t* masks_out, void* stream) {
  DCF_CHECK(m && vid && shallow_vid && vid_mask && nq_per_video && text && text_len && text_cls && logits1_out && logits2_out && offsets_out && masks_out,
            "dcf_forward_train_videos: null argument");
  DCF_CHECK(m->cfg.model_kind == 0, "dcf_forward_train_videos: the iterative early-fusion model only (model.py:567-632)");
  DCF_CHECK(nvid >= 1 && nvid <= dcf::DCF_MAX_VIDEOS, "dcf_forward_train_videos: 1 .. %d videos per call", dcf::DCF_MAX_VIDEOS);
  DCF_CHECK(T < (1ll << 24), "T too large");
  dcf::VideoSet vs;
  vs.logits1_out = logits1_out;
  int nq = 0;
  if (dcf::fill_videos(vs, "dcf_forward_train_videos", nvid, vid, shallow_vid, vid_mask, text_cls, nq_per_video, &nq)) return -1;
  if (m->drop_state.active) {
    DCF_CHECK(!m->cfg.second_fusion, "dcf_forward_train_videos: dropout with the second fusion is not implemented");
    m->drop = &m->drop_state;
  }
  const int rc = dcf::forward_maybe_graph(m, vs, (int)T, nq, {text, text_mask, text_len, nullptr, logits2_out, offsets_out, masks_out},
                                          (hipStream_t)stream);
  m->drop = nullptr;
  return rc;
}

int dcf_forward_eval_gated(dcf_model* m, const float* vid, const float* shallow_vid, const uint8_t* vid_mask, int64_t T,
                           int32_t nq, const float* const* text, const uint8_t* const* text_mask, const int32_t* text_len,
                           const float* gate, float* logits_out, float* offsets_out, uint8_t* masks_out, void* stream) {
  DCF_CHECK(m && vid && shallow_vid && vid_mask && text && text_len && gate && logits_out && offsets_out && masks_out,
            "dcf_forward_eval_gated: null argument");
  DCF_CHECK(T < (1ll << 24), "T too large");
  dcf::VideoSet vs;
  vs.nvid = 1; vs.vid[0] = vid; vs.shallow[0] = shallow_vid; vs.mask[0] = vid_mask; vs.text_cls[0] = nullptr; vs.nq[0] = nq;
  return dcf::forward_maybe_graph(m, vs, (int)T, nq, {text, text_mask, text_len, gate, logits_out, offsets_out, masks_out},
                                  (hipStream_t)stream);
}

namespace dcf {
// The selected-clip forward of `nvid` videos.  row_first = nullptr is the one-video form (nvid = 1, the rows are [0, n_rows)): forward()
// takes that path on `nvid == 1 || fc.sel_first`, so the one-video entry points never hand a row_first over.
static int forward_selected(dcf_model* m, int nvid, const float* rows, const int32_t* row_first, int32_t n_rows, const int32_t* pos,
                            const float* const* shallow, const uint8_t* const* vid_mask, int64_t T, const int32_t* nq_per_video, int nq,
                            const float* const* text, const uint8_t* const* text_mask, const int32_t* text_len, const float* gate,
                            const float* correl, float* logits_out, float* offsets_out, uint8_t* masks_out, hipStream_t st) {
  VideoSet vs;
  vs.nvid = nvid;
  for (int v = 0; v < nvid; ++v) {
    vs.vid[v] = nullptr; vs.shallow[v] = shallow[v]; vs.mask[v] = vid_mask[v]; vs.text_cls[v] = nullptr; vs.nq[v] = nq_per_video[v];
  }
  ForwardCall fc{text, text_mask, text_len, gate, logits_out, offsets_out, masks_out};
  fc.sel_rows = rows; fc.sel_pos = pos; fc.sel_n = n_rows; fc.sel_first = row_first; fc.sel_correl = correl;
  return forward_maybe_graph(m, vs, (int)T, nq, fc, st);
}
// The refusals of the selected-clip forwards that need no workspace: before any launch, and before the half forms' upcast.  row_first =
// nullptr is the one-video form, which refuses scat and bounds n_rows; the several-video form wants correl exactly with scat and bounds
// every video's rows.  *nq_out = the queries of all videos.
static int selected_checks(const dcf_model* m, const char* who, int nvid, const int32_t* row_first, int32_t n_rows, int64_t T,
                           const int32_t* nq_per_video, const float* correl, int* nq_out) {
  DCF_CHECK(T >= 1 && T < (1ll << 24), "%s: T out of range", who);
  DCF_CHECK(m->finalized, "%s: model not finalized", who);
  if (row_first) DCF_CHECK(nvid >= 1 && nvid <= DCF_MAX_VIDEOS, "%s: 1 .. %d videos per call (got %d)", who, DCF_MAX_VIDEOS, nvid);
  else DCF_CHECK(!m->cfg.scat, "%s: opt.model.scat needs the sidekick scores, which this forward is not handed (as dcf_forward_eval_gated)", who);
  DCF_CHECK(m->vid_w1, "%s: opt.model.sfonly reads no expert features: there is nothing to select", who);
  DCF_CHECK(vid_stride_of(m->cfg) == 1, "%s: vid_net.stride = %d: the externally gated forward takes vid_net.stride = 1", who, vid_stride_of(m->cfg));
  int nq = 0;
  if (!row_first) {
    DCF_CHECK(n_rows >= 1 && n_rows <= T, "%s: n_rows=%d must lie in [1, T=%lld]", who, (int)n_rows, (long long)T);
    nq = nq_per_video[0];
  } else {
    DCF_CHECK(!m->cfg.scat == !correl, "%s: correl (the sidekick scores of dcf_select_videos) is required with opt.model.scat and must be "
                                       "null without it", who);
    for (int v = 0; v < nvid; ++v) {
      DCF_CHECK(nq_per_video[v] >= 1 && nq + nq_per_video[v] <= DCF_MAX_VIDEOS * 64, "%s: bad query count of video %d", who, v);
      nq += nq_per_video[v];
    }
    const int Bmax = std::min(nq, m->cfg.max_batch > 0 ? m->cfg.max_batch : 8);
    DCF_CHECK(nvid == 1 || Bmax <= 16, "%s: several videos per forward need max_batch <= 16 (got %d)", who, Bmax);
    DCF_CHECK(row_first[0] == 0, "%s: row_first[0] = %d, not 0", who, (int)row_first[0]);
    for (int v = 0; v < nvid; ++v) {
      const int64_t n = (int64_t)row_first[v + 1] - row_first[v];
      DCF_CHECK(n >= 1 && n <= T, "%s: video %d has %lld rows: every video needs 1 .. T = %lld", who, v, (long long)n, (long long)T);
    }
  }
  *nq_out = nq;
  return 0;
}
// The half forms: the packed rows and every video's shallow features upcast once into the engine's half workspace (exact: every binary16
// value is an fp32 value), then the fp32 form: the same numbers as fp32 operands of the same values give.  Layout: the rows, then the
// videos' shallow features, each piece rounded up to 256 bytes.
static int upcast_selected_h(dcf_model* m, int nvid, const uint16_t* vid_rows, int64_t n_rows, const uint16_t* const* shallow_vid, int64_t T,
                             hipStream_t st, const float** rows32, const float** sh32) {
  const int D = m->cfg.D;
  const size_t rows_b = ((size_t)n_rows * D * sizeof(float) + 255) & ~(size_t)255;
  const size_t sh_b = ((size_t)D * T * sizeof(float) + 255) & ~(size_t)255;
  if (grow_half_ws(m, rows_b + sh_b * nvid, st)) return -1;
  if (launch_half_to_f32(vid_rows, reinterpret_cast<float*>(m->half_ws), n_rows * D, st)) return -1;
  *rows32 = reinterpret_cast<const float*>(m->half_ws);
  for (int v = 0; v < nvid; ++v) {
    float* d = reinterpret_cast<float*>(m->half_ws + rows_b + sh_b * v);
    if (launch_half_to_f32(shallow_vid[v], d, (int64_t)D * T, st)) return -1;
    sh32[v] = d;
  }
  return 0;
}
}  // namespace dcf

int dcf_select_ext_version(void) { return DCF_SELECT_EXT_VERSION; }

int dcf_forward_eval_selected(dcf_model* m, const float* vid_rows, int32_t n_rows, const int32_t* pos, const float* shallow_vid,
                              const uint8_t* vid_mask, int64_t T, int32_t nq, const float* const* text, const uint8_t* const* text_mask,
                              const int32_t* text_len, const float* gate, float* logits_out, float* offsets_out, uint8_t* masks_out,
                              void* stream) {
  const char* who = "dcf_forward_eval_selected";
  DCF_CHECK(m && vid_rows && pos && shallow_vid && vid_mask && text && text_len && gate && logits_out && offsets_out && masks_out,
            "%s: null argument", who);
  int nq_all = 0;
  if (dcf::selected_checks(m, who, 1, nullptr, n_rows, T, &nq, nullptr, &nq_all)) return -1;
  return dcf::forward_selected(m, 1, vid_rows, nullptr, n_rows, pos, &shallow_vid, &vid_mask, T, &nq, nq, text, text_mask, text_len, gate,
                               nullptr, logits_out, offsets_out, masks_out, (hipStream_t)stream);
}

int dcf_forward_eval_selected_h(dcf_model* m, const uint16_t* vid_rows, int32_t n_rows, const int32_t* pos, const uint16_t* shallow_vid,
                                const uint8_t* vid_mask, int64_t T, int32_t nq, const float* const* text, const uint8_t* const* text_mask,
                                const int32_t* text_len, const float* gate, float* logits_out, float* offsets_out, uint8_t* masks_out,
                                void* stream) {
  const char* who = "dcf_forward_eval_selected_h";
  DCF_CHECK(m && vid_rows && pos && shallow_vid && vid_mask && text && text_len && gate && logits_out && offsets_out && masks_out,
            "%s: null argument", who);
  int nq_all = 0;
  if (dcf::selected_checks(m, who, 1, nullptr, n_rows, T, &nq, nullptr, &nq_all)) return -1;
  const float *rows32, *sh32;
  if (dcf::upcast_selected_h(m, 1, vid_rows, n_rows, &shallow_vid, T, (hipStream_t)stream, &rows32, &sh32)) return -1;
  return dcf::forward_selected(m, 1, rows32, nullptr, n_rows, pos, &sh32, &vid_mask, T, &nq, nq, text, text_mask, text_len, gate, nullptr,
                               logits_out, offsets_out, masks_out, (hipStream_t)stream);
}

int dcf_forward_eval_videos_selected(dcf_model* m, int32_t nvid, const float* vid_rows, const int32_t* row_first, const int32_t* pos,
                                     const float* const* shallow_vid, const uint8_t* const* vid_mask, int64_t T,
                                     const int32_t* nq_per_video, const float* const* text, const uint8_t* const* text_mask,
                                     const int32_t* text_len, const float* gate, const float* correl, float* logits_out,
                                     float* offsets_out, uint8_t* masks_out, void* stream) {
  const char* who = "dcf_forward_eval_videos_selected";
  DCF_CHECK(m && vid_rows && row_first && pos && shallow_vid && vid_mask && nq_per_video && text && text_len && gate && logits_out &&
                offsets_out && masks_out, "%s: null argument", who);
  int nq = 0;
  if (dcf::selected_checks(m, who, nvid, row_first, 0, T, nq_per_video, correl, &nq)) return -1;
  for (int v = 0; v < nvid; ++v) DCF_CHECK(shallow_vid[v] && vid_mask[v], "%s: video %d is incomplete", who, v);
  return dcf::forward_selected(m, nvid, vid_rows, row_first, row_first[nvid], pos, shallow_vid, vid_mask, T, nq_per_video, nq, text,
                               text_mask, text_len, gate, correl, logits_out, offsets_out, masks_out, (hipStream_t)stream);
}

int dcf_forward_eval_videos_selected_h(dcf_model* m, int32_t nvid, const uint16_t* vid_rows, const int32_t* row_first,
                                       const int32_t* pos, const uint16_t* const* shallow_vid, const uint8_t* const* vid_mask, int64_t T,
                                       const int32_t* nq_per_video, const float* const* text, const uint8_t* const* text_mask,
                                       const int32_t* text_len, const float* gate, const float* correl, float* logits_out,
                                       float* offsets_out, uint8_t* masks_out, void* stream) {
  const char* who = "dcf_forward_eval_videos_selected_h";
  DCF_CHECK(m && vid_rows && row_first && pos && shallow_vid && vid_mask && nq_per_video && text && text_len && gate && logits_out &&
                offsets_out && masks_out, "%s: null argument", who);
  int nq = 0;
  if (dcf::selected_checks(m, who, nvid, row_first, 0, T, nq_per_video, correl, &nq)) return -1;
  for (int v = 0; v < nvid; ++v) DCF_CHECK(shallow_vid[v] && vid_mask[v], "%s: video %d is incomplete", who, v);
  const float *rows32, *sh32[dcf::DCF_MAX_VIDEOS];
  if (dcf::upcast_selected_h(m, nvid, vid_rows, row_first[nvid], shallow_vid, T, (hipStream_t)stream, &rows32, sh32)) return -1;
  return dcf::forward_selected(m, nvid, rows32, row_first, row_first[nvid], pos, sh32, vid_mask, T, nq_per_video, nq, text, text_mask,
                               text_len, gate, correl, logits_out, offsets_out, masks_out, (hipStream_t)stream);
}

int dcf_graph_active(const dcf_model* m) { return m ? m->last_launch : 0; }

}  // extern "C"
