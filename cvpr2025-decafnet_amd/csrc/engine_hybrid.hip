#include "engine.h"

namespace dcf {

// =============================================================================================
// One long video cut at pyramid level k (dist.py hybrid_forward, SURVEY 8e: the NQ = 1 corner of T-sharding).
// A rank holds TWO ordinary power-of-two pyramids: the NARROW one, levels 0 .. k on a window of Tn clips (everything a forward
// does in front of level k + 1), and the COARSE one, levels k .. L - 1 on a window of Tc level-k rows whose level 0 is the
// all-gathered level-k feature map.  Three phases with one exchange between each two:
//   phase 1  narrow window: vid_map, early fusion, embedding, levels 0 .. k           -> level-k features (narrow window)
//   phase 2  coarse window: levels k + 1 .. L - 1; cls_head on both pyramids; the refinement TCN on the narrow window's clips over the
//            stacked logits of ALL levels (model.py:449-458); pooled down to level k    -> refined level-k map (narrow window)
//   phase 3  refined map pooled down the coarse pyramid; cls_head2 / reg_head on both    -> outputs of levels <= k (narrow) and > k (coarse)
// Windows are treated as sequences (zero padding at their ends); the halos of dist.hybrid_plan absorb that.
// =============================================================================================
void free_hybrid(dcf_model* m) {
  if (!m->hyb) return;
  for (Plan* p : {&m->hyb->pn, &m->hyb->pc, &m->hyb->pch}) if (p->d_lt) (void)hipFree(p->d_lt);
  delete m->hyb;
  m->hyb = nullptr;
}

// size of the coarse pyramid's own buffers behind the forward's workspace (phase 1 reserves them: no reallocation between phases)
static size_t hybrid_extra_bytes(const dcf_config& c, int B, int Tc, int LC, int Tn, int L) {
  size_t rows = 0;
  for (int j = 0; j < LC; ++j) rows += (size_t)B * (Tc >> j);
  const size_t EH = c.E + TCN_HID;
  return rows * EH * 4 + 2 * (rows + 256) + rows * 4 + (size_t)B * Tn * L * 4 + 8 * 256;
}

int hybrid_take(dcf_model* m, const Buffers& b, const Plan& pl, int B, int Lk, hipStream_t st) {
  HybridState& h = *m->hyb;
  const dcf_config& c = m->cfg;
  const int E = c.E, ldf = E + TCN_HID, k = h.k;
  h.bn = b; h.B = B; h.Lk = Lk;
  h.pn.lt = pl.lt; h.pn.T0 = pl.T0; h.pn.B = pl.B; h.pn.L = pl.L;
  if (!h.pn.d_lt) DCF_HIP(hipMalloc(&h.pn.d_lt, sizeof(LevelTable)));
  DCF_HIP(hipMemcpyAsync(h.pn.d_lt, pl.d_lt, sizeof(LevelTable), hipMemcpyDeviceToDevice, st));
  // the coarse pyramid's buffers
  const int LC = c.n_levels - k;
  Arena a{m->hyb_extra_ptr, 0, m->hyb_extra, false};
  size_t rows = 0;
  for (int j = 0; j < LC; ++j) rows += (size_t)B * (h.Tc >> j);
  h.Fc = a.take<float>(rows * ldf);
  h.maskc = a.take<uint8_t>(rows);
  h.nbrc = a.take<uint8_t>(rows);
  h.logits1c = a.take<float>(rows);
  h.stacked = a.take<float>((size_t)B * h.Tn * c.n_levels);
  DCF_CHECK(a.off <= m->hyb_extra, "internal: hybrid workspace");
  // level-k features of the narrow window -> caller (B, Tn >> k, E)
  DCF_HIP(hipMemcpy2DAsync(m->hyb_feat_out, (size_t)E * 4, b.F + (int64_t)pl.lt.start[k] * ldf, (size_t)ldf * 4, (size_t)E * 4,
                           (size_t)B * pl.lt.T[k], hipMemcpyDeviceToDevice, st));
  h.valid = true;
  return 0;
}

// u[b][t][l] = logits1 of level l at the narrow window's clip t (nearest: index t >> l), times the clip's mask for l > 0 (model.py:449-455);
// levels > k come from the coarse pyramid: its level j = l - k at index (((t >> k) + off_k) >> j)
__global__ void k_hybrid_stack(const float* __restrict__ l1n, const LevelTable* __restrict__ ltn, const float* __restrict__ l1c,
                               const LevelTable* __restrict__ ltc, const uint8_t* __restrict__ mask0, float* __restrict__ out,
                               int B, int Tn, int k, int L, int off_k) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= B * Tn) return;
  const int b = r / Tn, t = r - b * Tn;
  const float m0 = mask0[r] ? 1.f : 0.f;
  for (int l = 0; l < L; ++l) {
    float u;
    if (l <= k) u = l1n[ltn->start[l] + b * ltn->T[l] + (t >> l)];
    else {
      const int j = l - k - 1;                                    // level of the heads' coarse table (levels k + 1 ..)
      int i = ((t >> k) + off_k) >> (j + 1);
      i = i < 0 ? 0 : (i < ltc->T[j] ? i : ltc->T[j] - 1);
      u = l1c[ltc->start[j] + b * ltc->T[j] + i];
    }
    out[(int64_t)r * L + l] = l > 0 ? u * m0 : u;
  }
}

// Buffers of the coarse pyramid's HEAD levels (k + 1 ..): the narrow pyramid's scratch with F / masks / logits re-based
static Buffers hybrid_coarse_heads(const HybridState& h, int ldf) {
  Buffers bc = h.bn;
  const int s1 = h.pc.lt.start[1];
  bc.F = h.Fc + (int64_t)s1 * ldf; bc.mask_all = h.maskc + s1; bc.nbr_all = h.nbrc + s1; bc.logits1 = h.logits1c;
  return bc;
}

static int hybrid_phase2(dcf_model* m, const float* featk_c, const uint8_t* maskk_c, int off_k, float* refk_out, hipStream_t st) {
  HybridState& h = *m->hyb;
  const dcf_config& c = m->cfg;
  const int E = c.E, ldf = E + TCN_HID, k = h.k, L = c.n_levels, LC = L - k, B = h.B;
  // ---- the coarse pyramid: level 0 = the gathered level-k features, its masks from the level-k validity of the window
  DCF_HIP(hipMemcpy2DAsync(h.Fc, (size_t)ldf * 4, featk_c, (size_t)E * 4, (size_t)E * 4, (size_t)B * h.Tc, hipMemcpyDeviceToDevice, st));
  for (int b = 0; b < B; ++b) DCF_HIP(hipMemcpyAsync(h.maskc + (size_t)b * h.Tc, maskk_c, (size_t)h.Tc, hipMemcpyDeviceToDevice, st));
  TRY(launch_pyramid_masks(h.maskc, h.nbrc, B, h.Tc, LC, h.pc.lt.start[LC], st));
  const LevelTable& lc = h.pc.lt;
  for (int j = 1; j < LC; ++j) {
    const float* xin = h.Fc + (int64_t)lc.start[j - 1] * ldf;
    float* xo = h.Fc + (int64_t)lc.start[j] * ldf;
    if (c.pool_only) TRY(launch_dwconv3(xin, ldf, h.maskc + lc.start[j - 1], m->pool_w[k + j], xo, ldf, B, lc.T[j - 1], 2, E, st));
    else TRY(run_encoder(m, m->branch[k + j], h.bn, xin, ldf, h.maskc + lc.start[j - 1], h.maskc + lc.start[j], B, lc.T[j - 1], 2, xo, ldf, st));
  }
  // ---- cls_head on both pyramids (level-major rows)
  TRY(run_head(m, m->cls1, h.bn, h.pn, E, 1, 0, 0, h.bn.logits1, st));
  Buffers bc = hybrid_coarse_heads(h, ldf);
  if (LC > 1) TRY(run_head(m, m->cls1, bc, h.pch, E, 1, 0, 0, h.logits1c, st));
  // ---- the refinement TCN on the narrow window's clips over the stacked logits of all levels
  const int rows0 = B * h.Tn;
  hipLaunchKernelGGL(k_hybrid_stack, dim3((rows0 + 255) / 256), dim3(256), 0, st, (const float*)h.bn.logits1, (const LevelTable*)h.pn.d_lt,
                     (const float*)h.logits1c, (const LevelTable*)h.pch.d_lt, (const uint8_t*)h.bn.mask_all, h.stacked, B, h.Tn, k, L, off_k);
  DCF_HIP(hipGetLastError());
  RefineArgs ra = refine_args(m);
  ra.stacked = h.stacked; ra.mask_all = h.bn.mask_all;
  ra.bufA = h.bn.tcnA; ra.bufB = h.bn.tcnB; ra.F = h.bn.F; ra.ldf = ldf; ra.E = E;
  ra.B = B; ra.T0 = h.Tn; ra.n_levels = L; ra.n_layers = L;
  TRY(launch_refine(ra, h.pn.lt, st));
  const LevelTable& ln = h.pn.lt;
  for (int l = 1; l <= k; ++l)
    TRY(launch_refine_pool(h.bn.F, ldf, E, h.bn.mask_all + ln.start[l - 1], ln.start[l - 1], ln.start[l], B, ln.T[l - 1], st));
  DCF_HIP(hipMemcpy2DAsync(refk_out, (size_t)TCN_HID * 4, h.bn.F + (int64_t)ln.start[k] * ldf + E, (size_t)ldf * 4, (size_t)TCN_HID * 4,
                           (size_t)B * ln.T[k], hipMemcpyDeviceToDevice, st));
  return 0;
}

static int hybrid_phase3(dcf_model* m, const float* refk_c, float* logits_n, float* offsets_n, uint8_t* masks_n, float* logits_c,
                         float* offsets_c, uint8_t* masks_c, hipStream_t st) {
  HybridState& h = *m->hyb;
  const dcf_config& c = m->cfg;
  const int E = c.E, ldf = E + TCN_HID, LC = c.n_levels - h.k, B = h.B;
  const LevelTable& lc = h.pc.lt;
  DCF_HIP(hipMemcpy2DAsync(h.Fc + E, (size_t)ldf * 4, refk_c, (size_t)TCN_HID * 4, (size_t)TCN_HID * 4, (size_t)B * h.Tc, hipMemcpyDeviceToDevice, st));
  for (int j = 1; j < LC; ++j)
    TRY(launch_refine_pool(h.Fc, ldf, E, h.maskc + lc.start[j - 1], lc.start[j - 1], lc.start[j], B, lc.T[j - 1], st));
  TRY(run_head_pair(m, m->cls2, m->reg, h.bn, h.pn, E + TCN_HID, 1, 0, logits_n, 2, 1, offsets_n, st));
  const int rows_n = h.pn.lt.start[h.pn.lt.n_levels];
  launch_masks_out(h.bn.mask_all, masks_n, h.pn.d_lt, m->status, logits_n, rows_n, st);
  DCF_HIP(hipGetLastError());
  if (LC > 1) {
    Buffers bc = hybrid_coarse_heads(h, ldf);
    TRY(run_head_pair(m, m->cls2, m->reg, bc, h.pch, E + TCN_HID, 1, 0, logits_c, 2, 1, offsets_c, st));
    const int rows_c = h.pch.lt.start[h.pch.lt.n_levels];
    launch_masks_out(bc.mask_all, masks_c, h.pch.d_lt, m->status, logits_c, rows_c, st);
    DCF_HIP(hipGetLastError());
  }
  return 0;
}

}  // namespace dcf

extern "C" {

// ---- one long video cut at pyramid level k (see HybridState): three phases, an exchange between each two (dist.py hybrid_forward)
int dcf_hybrid_phase1(dcf_model* m, int32_t k, const float* vid_w, const float* shallow_w, const uint8_t* mask_w, int64_t Tn, int64_t Tc,
                      int32_t nq, const float* const* text, const uint8_t* const* text_mask, const int32_t* text_len, const float* gate_w,
                      float* featk_out, void* stream) {
  DCF_CHECK(m && vid_w && shallow_w && mask_w && text && text_len && gate_w && featk_out, "dcf_hybrid_phase1: null argument");
  const dcf_config& c = m->cfg;
  DCF_CHECK(m->finalized, "dcf_hybrid_phase1: model not finalized");
  DCF_CHECK(c.model_kind == 0 && !c.second_fusion && c.msf && !c.scat && dcf::vid_stride_of(c) == 1,
            "dcf_hybrid_phase1: the iterative early-fusion model with msf, without second_fusion / scat / vid_net.stride > 1");
  const int L = c.n_levels, LC = L - k, half = c.win / 2 > 0 ? c.win / 2 : 1;
  DCF_CHECK(k >= 0 && k < L, "dcf_hybrid_phase1: split level %d outside 0 .. %d", k, L - 1);
  DCF_CHECK(Tn > 0 && Tn < (1ll << 24) && Tn % ((int64_t)half << k) == 0, "dcf_hybrid_phase1: the narrow window (%lld clips) must be a multiple of %d", (long long)Tn, half << k);
  DCF_CHECK(Tc > 0 && Tc < (1ll << 24) && Tc % ((int64_t)half << (LC - 1)) == 0, "dcf_hybrid_phase1: the coarse window (%lld level-%d rows) must be a multiple of %d", (long long)Tc, k, half << (LC - 1));
  const int Bmax = c.max_batch > 0 ? c.max_batch : 8;
  DCF_CHECK(nq >= 1 && nq <= Bmax, "dcf_hybrid_phase1: 1 .. max_batch = %d queries per call", Bmax);
  DCF_CHECK(Tc <= Tn, "dcf_hybrid_phase1: the coarse window (%lld level-%d rows) must not exceed the narrow one (%lld clips): the coarse levels run in its scratch", (long long)Tc, k, (long long)Tn);
  hipStream_t st = (hipStream_t)stream;
  if (!m->hyb) m->hyb = new dcf::HybridState();
  dcf::HybridState& h = *m->hyb;
  h.valid = false; h.k = k; h.Tn = (int)Tn; h.Tc = (int)Tc;
  int Tl[dcf::DCF_MAX_LEVELS];
  for (int j = 0; j < LC; ++j) Tl[j] = (int)(Tc >> j);
  // (the level tables of the coarse pyramid are rebuilt -- a synchronising upload -- only when its geometry changes)
  const bool same = h.pc.d_lt && h.pc.L == LC && h.pc.T0 == (int)Tc && h.pc.B == nq && (LC == 1 || (h.pch.d_lt && h.pch.L == LC - 1));
  if (!same) {
    if (dcf::make_plan(m, h.pc, Tl, LC, nq, m->reg_scales.data() + k, st)) return -1;
    if (LC > 1 && dcf::make_plan(m, h.pch, Tl + 1, LC - 1, nq, m->reg_scales.data() + k + 1, st)) return -1;
  }
  dcf::VideoSet vs;
  vs.nvid = 1; vs.vid[0] = vid_w; vs.shallow[0] = shallow_w; vs.mask[0] = mask_w; vs.text_cls[0] = nullptr; vs.nq[0] = nq;
  m->hyb_levels = k + 1;
  m->hyb_extra = dcf::hybrid_extra_bytes(c, nq, (int)Tc, LC, (int)Tn, L);
  m->hyb_feat_out = featk_out;
  const int rc = dcf::forward(m, vs, (int)Tn, nq, {text, text_mask, text_len, gate_w, nullptr, nullptr, nullptr}, st);
  m->hyb_levels = 0;
  m->hyb_extra = 0;
  m->hyb_feat_out = nullptr;
  if (rc == 0) DCF_CHECK(h.valid, "internal: hybrid phase 1 did not reach the hand-over");
  return rc;
}

int dcf_hybrid_phase2(dcf_model* m, const float* featk_c, const uint8_t* maskk_c, int64_t off_k, float* refk_out, void* stream) {
  DCF_CHECK(m && featk_c && maskk_c && refk_out, "dcf_hybrid_phase2: null argument");
  DCF_CHECK(m->hyb && m->hyb->valid, "dcf_hybrid_phase2: no phase 1 on this model (or another forward ran since)");
  DCF_CHECK(off_k >= 0 && off_k + (m->hyb->Tn >> m->hyb->k) <= m->hyb->Tc, "dcf_hybrid_phase2: the narrow window must lie inside the coarse one");
  return dcf::hybrid_phase2(m, featk_c, maskk_c, (int)off_k, refk_out, (hipStream_t)stream);
}

int dcf_hybrid_phase3(dcf_model* m, const float* refk_c, float* logits_n, float* offsets_n, uint8_t* masks_n, float* logits_c,
                      float* offsets_c, uint8_t* masks_c, void* stream) {
  DCF_CHECK(m && refk_c && logits_n && offsets_n && masks_n, "dcf_hybrid_phase3: null argument");
  DCF_CHECK(m->hyb && m->hyb->valid, "dcf_hybrid_phase3: no phase 1 / 2 on this model (or another forward ran since)");
  DCF_CHECK(m->cfg.n_levels - m->hyb->k <= 1 || (logits_c && offsets_c && masks_c), "dcf_hybrid_phase3: null coarse outputs");
  const int rc = dcf::hybrid_phase3(m, refk_c, logits_n, offsets_n, masks_n, logits_c, offsets_c, masks_c, (hipStream_t)stream);
  m->hyb->valid = false;
  return rc;
}

}  // extern "C"
