// The building blocks of a forward: carving the workspace, the level plans, the dense GEMM dispatch and the runners of an FFN,
// an encoder layer, a head and the fusion stack, each with the predicates that pick its kernels.
#include <algorithm>

#include "engine.h"

namespace dcf {

static void carve(Arena& a, const dcf_config& c, int T0, int B, int nq, int S, int Lk, int nvid, Buffers& b) {
  const size_t rows0 = (size_t)B * T0, rowsAll = (size_t)B * S;
  const size_t rowsF = std::max(rows0, (c.model_kind == 1 || c.second_fusion) ? rowsAll : (size_t)0);   // rows the fusion stack sees
  const bool strided = vid_stride_of(c) > 1;
  const int E = c.E, EH = c.E + TCN_HID;
  b.P1 = a.take<float>((size_t)nvid * T0 * E);
  b.P2 = a.take<float>((size_t)nvid * T0 * E);
  b.maskv = a.take<uint8_t>(nvid > 1 ? (size_t)nvid * T0 : 0);     // the videos' masks side by side (several videos only)
  b.tn = a.take<float>((size_t)nq * c.D);
  b.partial = a.take<float>((size_t)SCORE_SLICES * (nq + nvid) * T0);
  b.correl = a.take<float>((size_t)nq * T0);
  b.gate = a.take<float>(rows0);
  b.tile_flags = a.take<uint8_t>((size_t)B * ((T0 + 63) / 64));
  b.mask_all = a.take<uint8_t>(rowsAll);
  b.nbr_all = a.take<uint8_t>(rowsAll);
  b.mask_pre = a.take<uint8_t>(strided ? 2 * rows0 : 0);
  b.nbr_pre = a.take<uint8_t>(strided ? 2 * rows0 : 0);
  b.col5 = a.take<float>(strided ? rows0 / 2 * 5 * E : 0);
  b.kvmask = a.take<uint8_t>((size_t)B * Lk);
  b.X = a.take<float>(rows0 * E);
  for (int i = 0; i < 7; ++i) b.R[i] = a.take<float>((i < 3 ? rowsF : rows0) * E);
  b.stats = a.take<float>(rowsF * (size_t)((E + 63) / 64) * 2);
  for (int i = 0; i < 2; ++i) b.hstats[i] = a.take<float>(rowsAll * (size_t)((EH + 63) / 64) * 2);
  b.H2 = a.take<float>(rowsF * 2 * E);
  b.HID = a.take<float>(rowsF * 4 * E);
  b.F = a.take<float>(rowsAll * EH);
  b.HA = a.take<float>(rowsAll * EH);
  b.HB = a.take<float>(rowsAll * EH);
  b.HC = a.take<float>(rowsAll * EH);      // second trunk pair: two heads of equal shape run in lockstep (run_head_pair)
  b.HD = a.take<float>(rowsAll * EH);
  b.logits1 = a.take<float>(rowsAll);
  b.tcnA = a.take<float>(rows0 * TCN_HID);
  b.tcnB = a.take<float>(rows0 * TCN_HID);
  b.kvn = a.take<float>((size_t)B * Lk * c.TE);
  b.Kt = a.take<float>((size_t)B * Lk * E);
  b.Vt = a.take<float>((size_t)B * Lk * E);
  b.kvimg = a.take<unsigned short>((size_t)B * kv_image_halfs(2));
  b.kmadd = a.take<float>((size_t)B * 64);
}

// The workspace's buffers at `base`, or with base == nullptr the dry pass that only sizes them; returns the bytes they span.
// extra_ptr: with `extra` more bytes behind the buffers, handed out there.
size_t carve_at(char* base, const dcf_config& c, int T0, int B, int nq, int S, int Lk, int nvid, Buffers& b, size_t extra, char** extra_ptr) {
  Arena a{base, 0, 0, base == nullptr};
  carve(a, c, T0, B, nq, S, Lk, nvid, b);
  if (extra_ptr) *extra_ptr = a.take<char>(extra);
  return a.off;
}

int make_plan(dcf_model* m, Plan& p, const int* Tl, int n, int B, const float* scales, hipStream_t st) {
  p.T0 = Tl[0]; p.B = B; p.L = n;
  LevelTable& lt = p.lt;
  lt = LevelTable{};
  lt.n_levels = n; lt.B = B;
  int acc = 0;
  for (int l = 0; l < n; ++l) {
    lt.T[l] = Tl[l]; lt.off[l] = acc; lt.start[l] = B * acc; lt.scale[l] = scales ? scales[l] : 1.f;
    acc += Tl[l];
  }
  lt.S = acc; lt.start[n] = B * acc;
  if (!p.d_lt) DCF_HIP(hipMalloc(&p.d_lt, sizeof(LevelTable)));
  DCF_HIP(hipMemcpyAsync(p.d_lt, &p.lt, sizeof(LevelTable), hipMemcpyHostToDevice, st));
  DCF_HIP(hipStreamSynchronize(st));
  (void)m;
  return 0;
}

int get_plan(dcf_model* m, int T0, int B, int L, hipStream_t st, Plan** out) {
  for (auto& p : m->plans)
    if (p.T0 == T0 && p.B == B && p.L == L) { *out = &p; return 0; }
  Plan p;
  int Tl[DCF_MAX_LEVELS];
  for (int l = 0; l < L; ++l) Tl[l] = T0 >> l;
  TRY(make_plan(m, p, Tl, L, B, m->reg_scales.data(), st));          // (synchronises: p.lt is copied below, the upload reads the source)
  m->plans.push_back(p);
  *out = &m->plans.back();
  return 0;
}

// dense GEMM dispatch: bf16-split MFMA when the weight has split planes, fp32 MFMA otherwise
int run_gemm(dcf_model* m, GemmArgs* g, int count, GemmAMode mode, hipStream_t st) {
  bool split = m->gemm_terms != 0;
  int terms = 0;
  for (int i = 0; i < count && split; ++i) {
    auto it = m->wsplit.find(g[i].W);
    if (it == m->wsplit.end() || (g[i].ldw ? g[i].ldw : g[i].K) != m->wsplit_ldw[g[i].W]) { split = false; break; }
    const int t = m->wsplit_terms[g[i].W];
    if (terms && t != terms) { split = false; break; }
    terms = t;
    g[i].Ws = it->second;
    g[i].status = m->status;
  }
  if (split && mode == A_CHANMAJOR && (g[0].N % 128 != 0 || g[0].M % 4 != 0)) split = false;
  DCF_CHECK(split || mode != A_CHANMAJOR_H, "internal: a half operand needs the split-operand GEMM");
  for (int i = 0; i < count; ++i) DCF_CHECK(split || !(g[i].flags & G_ADALN), "internal: G_ADALN needs the split-operand GEMM");
  for (int i = 0; i < count; ++i) DCF_CHECK(split || !g[i].score_out, "internal: scores on the side need the split-operand GEMM");
  return split ? launch_gemm_split(g, count, mode, terms, st) : launch_gemm(g, count, mode, st);
}

// FFN (blocks.py:535-538): fc with the erf GELU in its epilogue, then proj (`go`: residual / LayerScale / mask epilogue)
// stats != nullptr: X holds the RAW rows, fc_w / fc_b are the LayerNorm-folded weight and bias and ln_s its row sums; the row
// statistics come from the GEMM that produced X (GemmArgs::stats_in)
// E = 256 in the f16x3 mode, from FFN_CHAIN_MIN_ROWS rows on: fc, GELU and proj as ONE kernel whose hidden activations stay in
// registers (ffn_chain.hip; 4 KiB per row neither written nor read back).  Below that the 128-row tiles leave CUs idle and
// the GEMM pair on 64-row tiles is faster (16 384 rows = 128 tiles, half the chip: 78 - 86 us against 63 + 40 for the pair;
// 8 192 rows: the same 80 us against 31 + 29).
constexpr int FFN_CHAIN_MIN_ROWS = 16384;
// (the row / width part of can_chain_ffn: what a producer needs to know to hand over row statistics)
static bool can_chain_ffn_rows(dcf_model* m, int rows, int E) {
  static const Setting off(nullptr, "DCF_NO_FFN_CHAIN", 0, Setting::PRESENT);     // developer switch: always the GEMM pair
  return !off.get() && E == 256 && rows >= FFN_CHAIN_MIN_ROWS && m->gemm_terms == GEMM_F16X3;
}
static bool can_chain_ffn(dcf_model* m, const float* fc_w, const GemmArgs& go, int rows, int E) {
  if (!can_chain_ffn_rows(m, rows, E)) return false;
  if (!m->wsplit.count(fc_w) || !m->wsplit.count(go.W) || m->wsplit_terms[fc_w] != GEMM_F16X3 || m->wsplit_terms[go.W] != GEMM_F16X3) return false;
  if (m->wsplit_ldw[fc_w] != E || m->wsplit_ldw[go.W] != 4 * E) return false;
  if (go.ln_w || !(go.flags & G_RES) || (go.flags & ~(G_RES | G_OUT_MASK)) || !go.R || !go.bias || go.a_scale > 0.f) return false;
  return true;
}
static int run_ffn_chain(dcf_model* m, const float* X, const float* fc_w, const float* fc_b, const GemmArgs& go, int rows, int E,
                         hipStream_t st, const float* stats, const float* ln_s) {
  FfnChainArgs a{};
  a.X = X; a.ldx = E; a.W1s = m->wsplit[fc_w]; a.b1 = fc_b; a.ln_s = ln_s; a.stats = stats; a.stats_slots = E / 64;
  a.W2s = m->wsplit[go.W]; a.b2 = go.bias; a.ls = go.ls; a.R = go.R; a.ldr = go.ldr;
  a.rowmask = (go.flags & G_OUT_MASK) ? go.rowmask : nullptr; a.C = go.C; a.ldc = go.ldc;
  a.stats_out = go.stats_out; a.stats_w = go.stats_w; a.status = m->status; a.M = rows;
  ProfScope prof("gemm_f16x3<ffn_chain>", st, 2.0 * rows * E * 4.0 * E * 2.0, (double)rows * E * 4.0 * 3.0);
  return launch_ffn_chain(a, st);
}

static int run_ffn(dcf_model* m, const float* X, const float* fc_w, const float* fc_b, GemmArgs go, float* HID, int rows, int E,
                   hipStream_t st, const float* stats = nullptr, const float* ln_s = nullptr) {
  if (can_chain_ffn(m, fc_w, go, rows, E)) return run_ffn_chain(m, X, fc_w, fc_b, go, rows, E, st, stats, ln_s);
  GemmArgs gf = gemm(X, E, fc_w, fc_b, HID, 4 * E, rows, 4 * E, E);
  gf.flags = G_GELU;
  if (stats) { gf.stats_in = stats; gf.ln_s = ln_s; gf.stats_slots = E / STATS_W; gf.stats_w = STATS_W; }
  TRY(run_gemm(m, &gf, 1, A_ROWS, st));
  return run_gemm(m, &go, 1, A_ROWS, st);
}

// can the LayerNorm between a producer GEMM (rows x n_prod, K = k_prod) and the ffn.fc that consumes it ride as row statistics?
static bool no_carry(const dcf_model* m) {
  static const Setting off(nullptr, "DCF_NO_LN_CARRY", 0, Setting::PRESENT);      // developer switch: standalone LayerNorm launches instead
  // ... or the model was told so (dcf_model_set_ln_carry: a row's mean dwarfed its spread, common.h LN_ILL_RATIO)
  return off.get() != 0 || m->no_ln_carry;
}
// (each GEMM is asked about with the arithmetic of ITS weight image: one of the two may have fallen back to bf16x6)
static bool can_carry_ln(dcf_model* m, const float* prod_w, const float* fc_wf, int rows, int n_prod, int k_prod, int E) {
  if (no_carry(m) || !fc_wf || !prod_w || m->gemm_terms == 0 || !m->wsplit.count(fc_wf) || !m->wsplit.count(prod_w)) return false;
  return gemm_can_carry_stats(rows, n_prod, k_prod, 1, m->wsplit_terms[prod_w]) &&
         gemm_can_carry_stats(rows, 4 * E, E, 1, m->wsplit_terms[fc_wf]);
}

// can this GEMM carry its LayerNorm in the epilogue?  (bf16-split path with planes for W, tile spanning the row)
// ... and is its K loop long enough to pay for the heavier epilogue (two workgroup-wide reductions on a 64-row tile)?  At
// K = 256 the fused kernel takes 117 us for 81920 rows against 55 + 39 us for the 128x256 kernel + the LayerNorm kernel (65
// against 28 + 20 us at 40960 rows); at K = 768 (embedding convolutions) 232 against ~280 us, at K = 1024 a tie (81920 rows,
// round 2: the unfused kernel was the 64x256 tile too).
bool can_fuse_ln(dcf_model* m, const float* W, int M, int N, int K, GemmAMode mode) {
  // ... and only below 64 K rows: from there on the unfused GEMM runs on the 128x256 tile, which beats the 64x256 tile the
  // fused epilogue needs by more than the LayerNorm pass costs.  Measured at 8 videos per forward (profiles/r03_notes.md):
  // 131072x256x1024 fused 327 us against 228 + 49 us; the k3 convolutions 261120x256x768 366 against 285 + 53 us and
  // 131072x256x768 238 against 146 + 53 us (the 128x256 k3 tile reaches 350 - 360 TFLOP/s, 0.43 of the f16x3 peak).
  if (M >= 65536) return false;
  return m->gemm_terms != 0 && m->wsplit.count(W) && m->wsplit_ldw[W] == K && K >= 512 && gemm_can_fuse_ln(M, N, K, mode);
}

// conv -> LayerNorm -> ReLU -> conv (head / embedding trunks): can the LayerNorm + ReLU ride in the second convolution's A
// staging, fed by row statistics from the first one's epilogue?  (both on a tile kernel that has the two instantiations)
bool can_norm_a(dcf_model* m, const float* W1, const float* W2, int M, int C, int* stats_w) {
  if (no_carry(m) || m->gemm_terms == 0 || !m->wsplit.count(W1) || !m->wsplit.count(W2)) return false;
  const int t1 = m->wsplit_terms[W1], t2 = m->wsplit_terms[W2];
  return t1 == t2 && gemm_can_norm_a(M, C, 3 * C, t1, stats_w) && !can_fuse_ln(m, W1, M, C, 3 * C, A_ROWS_TAP3);
}
void norm_a(GemmArgs& g, const float* stats, int C, int stats_w, const float* ln_g, const float* ln_b) {
  g.a_stats = stats; g.a_stats_slots = C / stats_w; g.a_ln_g = ln_g; g.a_ln_b = ln_b;
}

// From 32 768 rows on, f16x3, E = 256, 4 heads, window <= 9, stride 1: ln_attn, the depthwise convolutions, q / k / v_norm and the three
// projections of an encoder layer as ONE kernel (enc_chain.hip k_enc_qkv) instead of k_enc_pre + the grouped GEMM.
static bool can_chain_enc(dcf_model* m, const EncW& w, int rows, int stride, int64_t ldx) {
  static const Setting off(nullptr, "DCF_NO_ENC_CHAIN", 0, Setting::PRESENT);    // developer switch: the separate launches
  static const Setting min_rows("enc_chain_min_rows", "DCF_ENC_CHAIN_MIN_ROWS", 32768);   // dcf_debug_set_option (tests), then the developer switch
  const dcf_config& c = m->cfg;
  // (m->no_ln_carry: the kernel folds q / k / v_norm with one-pass statistics of the convolution outputs)
  return !off.get() && !m->no_ln_carry && m->gemm_terms == GEMM_F16X3 && w.qkv_chain[0] && w.qkv_chain[1] && w.qkv_chain[2] && stride == 1 &&
         enc_chain_supports(c.E, c.vid_heads, c.win > 0 ? c.win : 99) && rows >= min_rows.get() && ldx % 4 == 0;
}

static bool can_chain_enc_attn(dcf_model* m, const EncW& w, int rows, int64_t ldr) {
  static const Setting off(nullptr, "DCF_NO_ENC_ATTN", 0, Setting::PRESENT);     // developer switch: k_local_attn + the projection GEMM
  static const Setting min_rows("enc_attn_min_rows", "DCF_ENC_ATTN_MIN_ROWS", 32768);
  const dcf_config& c = m->cfg;
  return !off.get() && m->gemm_terms == GEMM_F16X3 && w.wp_chain && c.win > 0 && (c.win & 1) && enc_chain_supports(c.E, c.vid_heads, c.win) &&
         rows >= min_rows.get() && ldr % 4 == 0;
}

// the arguments of k_enc_pre for the input X [B*T_in][ldx] of an encoder layer; the caller sets the outputs Qc / Kc / Vc / Skip
EncPreArgs enc_pre_args(const EncW& w, const float* X, int64_t ldx, const uint8_t* mask_in, int B, int T_in, int E) {
  EncPreArgs ep{};
  ep.X = X; ep.ldx = ldx; ep.mask_in = mask_in; ep.ln_w = w.ln_attn_w; ep.ln_b = w.ln_attn_b;
  ep.dw_q = w.dw_q; ep.dw_k = w.dw_k; ep.dw_v = w.dw_v;
  ep.qn_w = w.qn_w; ep.qn_b = w.qn_b; ep.kn_w = w.kn_w; ep.kn_b = w.kn_b; ep.vn_w = w.vn_w; ep.vn_b = w.vn_b;
  ep.B = B; ep.T_in = T_in; ep.C = E;
  return ep;
}
// The unfused front of an encoder layer, shared by run_encoder's fallback and run_encoder_drop.  In two halves, because
// run_encoder may replace either by its chain kernel: k_enc_pre and the q / k / v projections -> R[4..6] ...
static int enc_unfused_qkv(dcf_model* m, const EncW& w, Buffers& b, const float* Xin, int64_t ldx, const uint8_t* mask_in, int B,
                           int T_in, int stride, hipStream_t st) {
  const int E = m->cfg.E, rows = B * (T_in / stride);
  EncPreArgs ep = enc_pre_args(w, Xin, ldx, mask_in, B, T_in, E);
  ep.Qc = b.R[0]; ep.Kc = b.R[1]; ep.Vc = b.R[2]; ep.Skip = stride == 2 ? b.R[3] : nullptr;
  TRY(launch_enc_pre(ep, stride, st));
  GemmArgs g3[3] = {gemm(b.R[0], E, w.wq, w.bq, b.R[4], E, rows, E, E), gemm(b.R[1], E, w.wk, w.bk, b.R[5], E, rows, E, E),
                    gemm(b.R[2], E, w.wv, w.bv, b.R[6], E, rows, E, E)};
  return run_gemm(m, g3, 3, A_ROWS, st);
}
// ... and the attention core R[4..6] -> R[0] over B sequences of To rows
static int enc_unfused_attention(dcf_model* m, Buffers& b, const uint8_t* mask_out, int B, int To, hipStream_t st) {
  const dcf_config& c = m->cfg;
  if (c.win > 0) {
    LocalAttnArgs la{b.R[4], b.R[5], b.R[6], mask_out, b.R[0], B, To, c.E, c.vid_heads, c.win};
    return launch_local_attn(la, st);
  }
  GlobalAttnArgs ga{b.R[4], b.R[5], b.R[6], mask_out, b.R[0], B, To, c.E, c.vid_heads};   // mha_win_size = 0: global self-attention (blocks.py:339-343)
  return launch_global_attn(ga, st);
}

// TransformerEncoder (vid_net) at one level.  Xin: [B*T_in][ldx]; output rows [B*T_out] at Xout (ld ldo).
int run_encoder(dcf_model* m, const EncW& w, Buffers& b, const float* Xin, int64_t ldx, const uint8_t* mask_in,
                const uint8_t* mask_out, int B, int T_in, int stride, float* Xout, int64_t ldo, hipStream_t st) {
  const dcf_config& c = m->cfg;
  const int E = c.E, To = T_in / stride, rows = B * To;
  if (can_chain_enc(m, w, rows, stride, ldx)) {
    EncQkvArgs ea{};
    ea.X = Xin; ea.ldx = ldx; ea.mask_in = mask_in; ea.ln_w = w.ln_attn_w; ea.ln_b = w.ln_attn_b;
    ea.dw[0] = w.dw_q; ea.dw[1] = w.dw_k; ea.dw[2] = w.dw_v;
    for (int i = 0; i < 3; ++i) { ea.W[i] = w.qkv_chain[i]; ea.fs[i] = w.qkv_s[i]; ea.fc[i] = w.qkv_c[i]; ea.out[i] = b.R[4 + i]; }
    ea.B = B; ea.T_in = T_in; ea.status = m->status;
    ProfScope prof("gemm_f16x3<enc_qkv>", st, 2.0 * rows * E * 3.0 * E, (double)rows * E * 4.0 * 4.0);
    TRY(launch_enc_qkv(ea, st));
  } else {
    TRY(enc_unfused_qkv(m, w, b, Xin, ldx, mask_in, B, T_in, stride, st));
  }
  // out = x' + ls_ffn * ((ffn) * mask)                                  (blocks.py:589-590)
  GemmArgs go = gemm(b.HID, 4 * E, w.pj_w, w.pj_b, Xout, ldo, rows, E, 4 * E);
  go.flags = G_RES | G_OUT_MASK; go.rowmask = mask_out; go.ls = w.ls_ffn; go.R = b.R[1]; go.ldr = E;
  // the window attention, attn.proj and the residual as one kernel (enc_chain.hip k_enc_attn) where the FFN takes x' with row statistics
  if (can_chain_enc_attn(m, w, rows, stride == 2 ? (int64_t)E : ldx)) {
    const bool carry = w.fc_wf && m->wsplit.count(w.fc_wf) && !no_carry(m) &&
                       (can_chain_ffn_rows(m, rows, E) || gemm_can_carry_stats(rows, 4 * E, E, 1, m->wsplit_terms[w.fc_wf]));
    EncAttnArgs aa{};
    aa.Q = b.R[4]; aa.K = b.R[5]; aa.V = b.R[6]; aa.mask = mask_out; aa.Wp = w.wp_chain; aa.bp = w.bp; aa.ls = w.ls_attn;
    if (stride == 2) { aa.R = b.R[3]; aa.ldr = E; } else { aa.R = Xin; aa.ldr = ldx; }
    aa.Y = b.R[1]; aa.ldy = E; aa.stats_out = carry ? b.stats : nullptr; aa.stats_w = STATS_W; aa.B = B; aa.T = To; aa.win = c.win; aa.status = m->status; aa.attn_single = c.attn_mode == 1;
    {
      ProfScope prof("gemm_f16x3<enc_attn>", st, 2.0 * rows * E * E + 4.0 * rows * E * c.win, (double)rows * E * 4.0 * 5.0);
      TRY(launch_enc_attn(aa, st));
    }
    if (carry) return run_ffn(m, b.R[1], w.fc_wf, w.fc_c, go, b.HID, rows, E, st, b.stats, w.fc_s);
    LnArgs ln{}; ln.X = b.R[1]; ln.ldx = E; ln.Y = b.R[2]; ln.ldy = E; ln.w = w.ln_ffn_w; ln.b = w.ln_ffn_b; ln.rows = rows; ln.C = E;
    TRY(launch_ln(ln, st));
    return run_ffn(m, b.R[2], w.fc_w, w.fc_b, go, b.HID, rows, E, st);
  }
  TRY(enc_unfused_attention(m, b, mask_out, B, To, st));
  // x' = skip * mask + ls_attn * (proj(ctx) + b)                       (blocks.py:586)
  GemmArgs gp = gemm(b.R[0], E, w.wp, w.bp, b.R[1], E, rows, E, E);
  gp.flags = G_RES | G_RES_MASK; gp.rowmask = mask_out; gp.ls = w.ls_attn;
  if (stride == 2) { gp.R = b.R[3]; gp.ldr = E; } else { gp.R = Xin; gp.ldr = ldx; }
  if (can_fuse_ln(m, w.wp, rows, E, E, A_ROWS)) {                 // ln_ffn(x') rides in the epilogue
    gp.ln_w = w.ln_ffn_w; gp.ln_b = w.ln_ffn_b; gp.Y = b.R[2]; gp.ldy = E;
    TRY(run_gemm(m, &gp, 1, A_ROWS, st));
  } else if (can_carry_ln(m, w.wp, w.fc_wf, rows, E, E, E)) {
    // ... or as row statistics: the projection writes (sum, sum of squares) of every x' row, ffn.fc runs on the raw x' with
    // ln_ffn folded into its weights and applies (mean, rstd) in its epilogue -- ln_ffn(x') is neither written nor read
    gp.stats_out = b.stats; gp.stats_w = STATS_W;
    TRY(run_gemm(m, &gp, 1, A_ROWS, st));
    return run_ffn(m, b.R[1], w.fc_wf, w.fc_c, go, b.HID, rows, E, st, b.stats, w.fc_s);
  } else {
    TRY(run_gemm(m, &gp, 1, A_ROWS, st));
    LnArgs ln{}; ln.X = b.R[1]; ln.ldx = E; ln.Y = b.R[2]; ln.ldy = E; ln.w = w.ln_ffn_w; ln.b = w.ln_ffn_b; ln.rows = rows; ln.C = E;
    TRY(launch_ln(ln, st));
  }
  TRY(run_ffn(m, b.R[2], w.fc_w, w.fc_b, go, b.HID, rows, E, st));
  return 0;
}

// From 30 000 pyramid rows on (one video of T = 16 384 has 32 640), in the f16x3 mode: trunk and output convolution of a head as
// ONE kernel, the trunk activations in registers (head_chain.hip).  One video per forward: 1.69 - 1.72 against 1.73 - 1.76 ms with
// the GEMM launches (268 tiles of 122 rows: one round of workgroups and a sliver); two videos per forward: +6 %.
static bool can_chain_head(dcf_model* m, const HeadW& h, int rows, int Cin, int NO) {
  static const Setting min_rows(nullptr, "DCF_HEAD_CHAIN_MIN_ROWS", 30000);     // developer switch
  static const Setting off(nullptr, "DCF_NO_HEAD_CHAIN", 0, Setting::PRESENT);     // developer switch: GEMM + LayerNorm + output-convolution launches
  if (off.get() || rows < min_rows.get() || m->gemm_terms != GEMM_F16X3 || !h.chain[0] || !h.chain[1] || !h.out_chain) return false;
  if (h.conv.size() != 2 || !head_chain_supports(Cin, NO)) return false;
  for (int i = 0; i < 2; ++i)
    if (!m->wsplit.count(h.conv[i]) || m->wsplit_terms[h.conv[i]] != GEMM_F16X3) return false;
  return true;
}
static HeadChainArgs head_chain_args(dcf_model* m, const HeadW& h, Buffers& b, const Plan& pl, int NO, int mode, int query_major, float* out) {
  HeadChainArgs a{};
  a.X = b.F; a.ldx = m->cfg.E + TCN_HID; a.nbr = b.nbr_all; a.W1c = h.chain[0]; a.W2c = h.chain[1];
  a.ln1_w = h.ln_w[0]; a.ln1_b = h.ln_b[0]; a.ln2_w = h.ln_w[1]; a.ln2_b = h.ln_b[1];
  a.Wout = h.out_w; a.Woc = h.out_chain; a.bout = h.out_b; a.lt = pl.d_lt; a.out = out; a.rows = pl.B * pl.lt.S; a.NO = NO; a.mode = mode;
  a.query_major = query_major; a.status = m->status;
  return a;
}
// algorithmic work of the launches a head kernel replaces: two k3 convolutions (C x 3C) and the output convolution; bytes: the
// input rows once, the outputs once
static int run_head_chain(dcf_model* m, const HeadChainArgs* a, int count, int Cin, hipStream_t st) {
  double flops = 0., bytes = 0.;
  for (int i = 0; i < count; ++i) {
    flops += 2.0 * a[i].rows * Cin * 3.0 * Cin * 2.0 + 2.0 * a[i].rows * 3.0 * Cin * a[i].NO;
    bytes += (double)a[i].rows * (Cin + a[i].NO) * 4.0;
  }
  ProfScope prof("gemm_f16x3<head_chain>", st, flops, bytes);
  return launch_head_chain(a, count, Cin, st);
}

// one head trunk (n x [k3 conv, LN, ReLU]) + output conv over the whole pyramid
// rows [row0, row0 + rows) of the pyramid (a whole pyramid, or one level)
int run_head(dcf_model* m, const HeadW& h, Buffers& b, const Plan& pl, int Cin, int NO, int mode, int query_major, float* out,
             hipStream_t st, int row0, int rows) {
  if (row0 == 0 && rows < 0 && can_chain_head(m, h, pl.B * pl.lt.S, Cin, NO)) {
    const HeadChainArgs a = head_chain_args(m, h, b, pl, NO, mode, query_major, out);
    return run_head_chain(m, &a, 1, Cin, st);
  }
  const int rowsAll = rows >= 0 ? rows : pl.B * pl.lt.S;
  const int ldf = m->cfg.E + TCN_HID;
  const float* in = b.F + (int64_t)row0 * ldf;
  int64_t ldin = ldf;
  float* HA = b.HA + (int64_t)row0 * Cin;
  float* HB = b.HB + (int64_t)row0 * Cin;
  const uint8_t* nbr = b.nbr_all + row0;
  const float *last_ln_w = nullptr, *last_ln_b = nullptr;
  float* hst = b.hstats[0] + (int64_t)row0 * ((Cin + 63) / 64) * 2;
  int pending = -1, pend_w = 0;                                  // layer whose LayerNorm + ReLU the next convolution applies on load
  for (size_t i = 0; i < h.conv.size(); ++i) {
    GemmArgs g = gemm(in, ldin, h.conv[i], nullptr, HA, Cin, rowsAll, Cin, 3 * Cin);
    g.cin = Cin; g.nbr = nbr;
    float* outp = (in == HB) ? HA : HB;                          // ping-pong between the two trunk buffers
    if (pending >= 0) { norm_a(g, hst, Cin, pend_w, h.ln_w[pending], h.ln_b[pending]); pending = -1; }
    int sw = 0;
    if (can_fuse_ln(m, h.conv[i], rowsAll, Cin, 3 * Cin, A_ROWS_TAP3) && !g.a_stats) {
      g.C = nullptr; g.ln_w = h.ln_w[i]; g.ln_b = h.ln_b[i]; g.Y = outp; g.ldy = Cin; g.ln_relu = 1;
      TRY(run_gemm(m, &g, 1, A_ROWS_TAP3, st));
    } else if (i + 1 < h.conv.size() && !g.a_stats && can_norm_a(m, h.conv[i], h.conv[i + 1], rowsAll, Cin, &sw)) {
      g.C = outp; g.stats_out = hst; g.stats_w = sw;             // raw output + row statistics: the next convolution normalises it
      TRY(run_gemm(m, &g, 1, A_ROWS_TAP3, st));
      pending = (int)i; pend_w = sw;
    } else {
      g.C = outp;                                                // raw conv output, normalised in place ...
      TRY(run_gemm(m, &g, 1, A_ROWS_TAP3, st));
      if (i + 1 == h.conv.size()) {                              // ... or, for the last layer, by the output convolution on load
        last_ln_w = h.ln_w[i]; last_ln_b = h.ln_b[i];
      } else {
        LnArgs ln{}; ln.X = outp; ln.ldx = Cin; ln.Y = outp; ln.ldy = Cin; ln.w = h.ln_w[i]; ln.b = h.ln_b[i];
        ln.rows = rowsAll; ln.C = Cin; ln.relu = 1;
        TRY(launch_ln(ln, st));
      }
    }
    in = outp; ldin = Cin;
  }
  ConvOutArgs co{};
  co.ln_w = last_ln_w; co.ln_b = last_ln_b;
  co.X = in; co.ldx = ldin; co.nbr = nbr; co.W = h.out_w; co.bias = h.out_b; co.lt = pl.d_lt;
  co.out = query_major ? out : out + row0;
  co.rows = rowsAll; co.C = Cin; co.NO = NO; co.row0 = row0; co.mode = mode; co.query_major = query_major;
  TRY(launch_conv_out(co, st));
  return 0;
}

// Two head trunks of the same shape on the same pyramid (cls_head2 and reg_head): each pair of k3 convolutions is one
// grid of twice the workgroups (blockIdx.z picks the operand set), so the kernel runs two rounds of workgroups whose
// prologues and epilogues overlap instead of two single-round launches.
int run_head_pair(dcf_model* m, const HeadW& h1, const HeadW& h2, Buffers& b, const Plan& pl, int Cin, int NO1, int mode1,
                  float* out1, int NO2, int mode2, float* out2, hipStream_t st) {
  const int rowsAll = pl.B * pl.lt.S;
  if (can_chain_head(m, h1, rowsAll, Cin, NO1) && can_chain_head(m, h2, rowsAll, Cin, NO2)) {
    const HeadChainArgs a[2] = {head_chain_args(m, h1, b, pl, NO1, mode1, 1, out1), head_chain_args(m, h2, b, pl, NO2, mode2, 1, out2)};
    return run_head_chain(m, a, 2, Cin, st);      // one grid for the two heads
  }
  bool pair = h1.conv.size() == h2.conv.size() && !h1.conv.empty() && m->gemm_terms != 0;
  for (size_t i = 0; pair && i < h1.conv.size(); ++i)
    pair = !can_fuse_ln(m, h1.conv[i], rowsAll, Cin, 3 * Cin, A_ROWS_TAP3) && m->wsplit.count(h1.conv[i]) && m->wsplit.count(h2.conv[i]);
  if (!pair) {
    TRY(run_head(m, h1, b, pl, Cin, NO1, mode1, 1, out1, st));
    return run_head(m, h2, b, pl, Cin, NO2, mode2, 1, out2, st);
  }
  const int ldf = m->cfg.E + TCN_HID;
  const float* in[2] = {b.F, b.F};
  int64_t ldin = ldf;
  float* buf[2][2] = {{b.HA, b.HB}, {b.HC, b.HD}};
  const HeadW* hs[2] = {&h1, &h2};
  int pending = -1, pend_w = 0;
  for (size_t i = 0; i < h1.conv.size(); ++i) {
    float* outp[2] = {buf[0][i & 1], buf[1][i & 1]};
    GemmArgs g[2];
    for (int k = 0; k < 2; ++k) {
      g[k] = gemm(in[k], ldin, hs[k]->conv[i], nullptr, outp[k], Cin, rowsAll, Cin, 3 * Cin);
      g[k].cin = Cin; g[k].nbr = b.nbr_all;
      if (pending >= 0) norm_a(g[k], b.hstats[k], Cin, pend_w, hs[k]->ln_w[pending], hs[k]->ln_b[pending]);
    }
    const bool was_pending = pending >= 0;
    pending = -1;
    int sw = 0;
    // the LayerNorm + ReLU between two layers rides in the next layer's A staging when both run on a kernel that can
    const bool carry = !was_pending && i + 1 < h1.conv.size() && can_norm_a(m, h1.conv[i], h1.conv[i + 1], rowsAll, Cin, &sw) &&
                       can_norm_a(m, h2.conv[i], h2.conv[i + 1], rowsAll, Cin, &sw);
    if (carry)
      for (int k = 0; k < 2; ++k) { g[k].stats_out = b.hstats[k]; g[k].stats_w = sw; }
    TRY(run_gemm(m, g, 2, A_ROWS_TAP3, st));
    if (carry) { pending = (int)i; pend_w = sw; }
    for (int k = 0; k < 2; ++k) {
      if (i + 1 < h1.conv.size() && !carry) {                    // the last layer is normalised by the output convolution on load
        LnArgs ln{}; ln.X = outp[k]; ln.ldx = Cin; ln.Y = outp[k]; ln.ldy = Cin; ln.w = hs[k]->ln_w[i]; ln.b = hs[k]->ln_b[i];
        ln.rows = rowsAll; ln.C = Cin; ln.relu = 1;
        TRY(launch_ln(ln, st));
      }
      in[k] = outp[k];
    }
    ldin = Cin;
  }
  const int NOs[2] = {NO1, NO2}, modes[2] = {mode1, mode2};
  float* outs[2] = {out1, out2};
  for (int k = 0; k < 2; ++k) {
    ConvOutArgs co{};
    co.X = in[k]; co.ldx = ldin; co.nbr = b.nbr_all; co.W = hs[k]->out_w; co.bias = hs[k]->out_b; co.lt = pl.d_lt;
    co.out = outs[k]; co.rows = rowsAll; co.C = Cin; co.NO = NOs[k]; co.row0 = 0; co.mode = modes[k]; co.query_major = 1;
    co.ln_w = hs[k]->ln_w.back(); co.ln_b = hs[k]->ln_b.back();
    TRY(launch_conv_out(co, st));
  }
  return 0;
}

// From 16 384 level-0 rows on (one video of T = 16 384), in the f16x3 mode, E = 256, 4 heads, <= 64 text tokens: the attention half
// of a fusion layer as ONE kernel (dec_chain.hip).
static bool can_chain_dec(dcf_model* m, const DecW& w, const LevelTable* lt, int rows, int64_t ldx, int Lk) {
  static const Setting off(nullptr, "DCF_NO_DEC_CHAIN", 0, Setting::PRESENT);    // developer switch: the separate launches
  // dcf_debug_set_option (tests), then the developer switch (one video per call: 1.70 against 1.74 ms)
  static const Setting min_rows("dec_chain_min_rows", "DCF_DEC_CHAIN_MIN_ROWS", 16384);
  const dcf_config& c = m->cfg;
  return !off.get() && !lt && m->gemm_terms == GEMM_F16X3 && w.wq_chain && w.wp_chain && dec_chain_supports(c.E, c.fusion_heads, Lk) &&
         c.TE % 32 == 0 && rows >= min_rows.get() && ldx % 4 == 0;
}

// XAttNFusion._forward (fusion.py:56-66): n x TransformerDecoder (blocks.py:632-650) + ln_out.
// X [rows][ldx] is updated in place; the final ln_out goes to out [rows][ld_out].  Either one level of B sequences
// of T rows (lt == nullptr) or the whole pyramid (lt != nullptr: rows ordered [level][b][t], neighbour flags `nbr`
// delimit the sequences for the depthwise conv, the attention core is launched per level).
// carry_out != nullptr: the caller can take fusion.ln_out as row statistics (b.stats of the raw stream left in X) instead of
// the normalised rows in `out`; *carry_out says which of the two happened.
int run_fusion(dcf_model* m, Buffers& b, float* X, int64_t ldx, int B, int T, const LevelTable* lt, const uint8_t* mask,
               const uint8_t* nbr, const TextMeta* dm, int Lk, float* out, int64_t ld_out, hipStream_t st, bool* carry_out) {
  if (carry_out) *carry_out = false;
  const dcf_config& c = m->cfg;
  const int E = c.E;
  const int rows = lt ? lt->start[lt->n_levels] : B * T;
  for (size_t li = 0; li < m->dec.size(); ++li) {
    const DecW& w = m->dec[li];
    bool carry = false;
    const bool chain = can_chain_dec(m, w, lt, rows, ldx, Lk);
    TextLnArgs tl{*dm, b.kvn, b.kvmask, w.ln_kv_w, w.ln_kv_b, Lk, c.TE};
    TRY(launch_text_ln(tl, B, st));
    GemmArgs gkv[2] = {gemm(b.kvn, c.TE, w.wk, w.bk, b.Kt, E, B * Lk, E, c.TE), gemm(b.kvn, c.TE, w.wv, w.bv, b.Vt, E, B * Lk, E, c.TE)};
    TRY(run_gemm(m, gkv, 2, A_ROWS, st));
    if (chain) {
      // q3 = adaln(q) * scale + shift straight from the raw stream: ln_xattn_q, the depthwise convolution, q_norm, the query
      // projection, the cross attention and the modulating projection in one kernel; ln_ffn(q3) as row statistics where the FFN
      // can take them, by the LayerNorm kernel otherwise
      const int lk2 = Lk <= 32 ? 1 : 2;
      TRY(launch_kv_image(b.Kt, b.Vt, b.kvmask, B, Lk, lk2, b.kvimg, b.kmadd, st));
      carry = !no_carry(m) && w.fc_wf && m->wsplit.count(w.fc_wf) &&
              (can_chain_ffn_rows(m, rows, E) || gemm_can_carry_stats(rows, 4 * E, E, 1, m->wsplit_terms[w.fc_wf]));
      DecChainArgs da{};
      da.X = X; da.ldx = ldx; da.mask = mask; da.ln_q_w = w.ln_q_w; da.ln_q_b = w.ln_q_b; da.dw = w.dw; da.qn_w = w.qn_w; da.qn_b = w.qn_b;
      da.Wq = w.wq_chain; da.bq = w.bq; da.KV = b.kvimg; da.kmask = b.kmadd; da.Wp = w.wp_chain; da.bp = w.bp_il;
      da.Q3 = b.R[2]; da.ldq = E; da.stats_out = carry ? b.stats : nullptr; da.stats_w = STATS_W;
      da.B = B; da.T = T; da.affine = c.xattn_affine; da.lk2 = lk2; da.status = m->status; da.attn_single = c.attn_mode == 1;
      {
        ProfScope prof("gemm_f16x3<dec_chain>", st, 2.0 * rows * E * 3.0 * E + 4.0 * rows * E * Lk, (double)rows * E * 4.0 * 2.0);
        TRY(launch_dec_chain(da, st));
      }
      if (!carry) {
        LnArgs ln{}; ln.X = b.R[2]; ln.ldx = E; ln.Y = b.R[0]; ln.ldy = E; ln.w = w.ln_ffn_w; ln.b = w.ln_ffn_b; ln.rows = rows; ln.C = E;
        TRY(launch_ln(ln, st));
      }
    } else {
    DecPreArgs dp{X, ldx, mask, w.ln_q_w, w.ln_q_b, w.dw, w.qn_w, w.qn_b, b.R[0], b.R[1], lt ? 1 : B, lt ? rows : T, E};
    dp.nbr = lt ? nbr : nullptr;
    dp.affine = c.xattn_affine;
    TRY(launch_dec_pre(dp, st));
    GemmArgs gq = gemm(b.R[0], E, w.wq, w.bq, b.R[2], E, rows, E, E);
    TRY(run_gemm(m, &gq, 1, A_ROWS, st));
    if (lt) {
      for (int l = 0; l < lt->n_levels; ++l) {
        XAttnArgs xa{b.R[2] + (int64_t)lt->start[l] * E, b.Kt, b.Vt, b.kvmask, b.R[0] + (int64_t)lt->start[l] * E, B, lt->T[l], Lk, E, c.fusion_heads, m->status, c.attn_mode == 1};
        TRY(launch_xattn(xa, st));
      }
    } else {
      XAttnArgs xa{b.R[2], b.Kt, b.Vt, b.kvmask, b.R[0], B, T, Lk, E, c.fusion_heads, m->status, c.attn_mode == 1};
      TRY(launch_xattn(xa, st));
    }
    if (m->gemm_terms != 0 && w.wp_il && m->wsplit.count(w.wp_il) && gemm_can_fuse_adaln(rows, 2 * E, E)) {
      // q3 = Xa * scale + shift in the epilogue of the projection (blocks.py:643-646): the (rows, 2E) scale / shift tensor is
      // never written; Xn = ln_ffn(q3) by the LayerNorm kernel
      GemmArgs gh = gemm(b.R[0], E, w.wp_il, w.bp_il, b.R[2], E, rows, 2 * E, E);
      gh.flags = G_ADALN; gh.R = b.R[1]; gh.ldr = E;
      carry = can_carry_ln(m, w.wp_il, w.fc_wf, rows, 2 * E, E, E);            // ln_ffn(q3) as row statistics (see run_encoder)
      if (carry) { gh.stats_out = b.stats; gh.stats_w = STATS_W; }
      TRY(run_gemm(m, &gh, 1, A_ROWS, st));
      if (!carry) {
        LnArgs ln{}; ln.X = b.R[2]; ln.ldx = E; ln.Y = b.R[0]; ln.ldy = E; ln.w = w.ln_ffn_w; ln.b = w.ln_ffn_b; ln.rows = rows; ln.C = E;
        TRY(launch_ln(ln, st));
      }
    } else {
      GemmArgs gh = gemm(b.R[0], E, w.wp, w.bp, b.H2, 2 * E, rows, 2 * E, E);
      TRY(run_gemm(m, &gh, 1, A_ROWS, st));
      TRY(launch_dec_mid(b.R[1], b.H2, w.ln_ffn_w, w.ln_ffn_b, b.R[2], b.R[0], rows, E, st));
    }
    }   // (!chain)
    GemmArgs go = gemm(b.HID, 4 * E, w.pj_w, w.pj_b, X, ldx, rows, E, 4 * E);
    go.flags = G_RES | G_OUT_MASK; go.rowmask = mask; go.ls = w.ls_ffn; go.R = b.R[2]; go.ldr = E;
    const float* fc_in = carry ? b.R[2] : b.R[0];
    const float *fc_w = carry ? w.fc_wf : w.fc_w, *fc_b = carry ? w.fc_c : w.fc_b;
    if (li + 1 == m->dec.size() && m->fus_out_w && can_fuse_ln(m, w.pj_w, rows, E, 4 * E, A_ROWS)) {
      // last layer: only ln_out(x) is consumed afterwards (fusion.py:64-66), the raw stream is not written
      GemmArgs gf = gemm(fc_in, E, fc_w, fc_b, b.HID, 4 * E, rows, 4 * E, E);
      gf.flags = G_GELU;
      if (carry) { gf.stats_in = b.stats; gf.ln_s = w.fc_s; gf.stats_slots = E / STATS_W; gf.stats_w = STATS_W; }
      TRY(run_gemm(m, &gf, 1, A_ROWS, st));
      go.C = nullptr; go.ln_w = m->fus_out_w; go.ln_b = m->fus_out_b; go.Y = out; go.ldy = ld_out;
      TRY(run_gemm(m, &go, 1, A_ROWS, st));
      return 0;
    }
    if (li + 1 == m->dec.size() && carry_out && m->fus_out_w && ldx == E &&
        m->embd_fc_wf && m->wsplit.count(m->embd_fc_wf) && !no_carry(m) &&
        m->wsplit.count(w.pj_w) && gemm_can_carry_stats(rows, E, 4 * E, 1, m->wsplit_terms[w.pj_w]) &&
        gemm_can_carry_stats(rows, E, E, 1, m->wsplit_terms[m->embd_fc_wf])) {
      // last layer: ffn.proj leaves the raw stream in X together with its row statistics, vid_net.embd_fc (ln_out folded into its
      // weights) applies them: ln_out(x) is neither written nor read (fusion.py:64-66 -> video_net.py:131)
      go.stats_out = b.stats; go.stats_w = STATS_W;
      // (the fc half reads b.stats before the proj half overwrites it: stream order in the GEMM pair; in the one-kernel form a
      // wave reads the statistics of its own rows at its start and writes them at its end)
      TRY(run_ffn(m, fc_in, fc_w, fc_b, go, b.HID, rows, E, st, carry ? b.stats : nullptr, w.fc_s));
      *carry_out = true;
      return 0;
    }
    TRY(run_ffn(m, fc_in, fc_w, fc_b, go, b.HID, rows, E, st, carry ? b.stats : nullptr, w.fc_s));
  }
  if (!m->fus_out_w) return 0;          // dcf_op_decoder: the bare layer stack, result left in X
  LnArgs ln{}; ln.X = X; ln.ldx = ldx; ln.Y = out; ln.ldy = ld_out; ln.w = m->fus_out_w; ln.b = m->fus_out_b; ln.rows = rows; ln.C = E;
  TRY(launch_ln(ln, st));
  return 0;
}

// ---- the training forward with dropout (dcf_model_set_dropout; contract in dropout.h / include/decafnet_hip.h).  Every site's
// tensor is materialised: the unfused kernel sequence of run_encoder / run_fusion, the dropout kernels between them.
static DropSite drop_at(const dcf_model* m, int rate, uint32_t site) {
  DropSite d;
  d.site = site; d.p = m->drop->p[rate]; d.scale = m->drop->scale[rate];
  return d;
}

// TransformerEncoder.forward (blocks.py:578-591) with proj_drop (sub 0), the FFN's two dropouts (1, 2) and both drop-paths (3, 4)
// of site group / layer `site0`; arguments as run_encoder.  Dropout tensors are (B', E / 4E, T_in / stride).
int run_encoder_drop(dcf_model* m, const EncW& w, Buffers& b, const float* Xin, int64_t ldx, const uint8_t* mask_in,
                     const uint8_t* mask_out, int B, int T_in, int stride, float* Xout, int64_t ldo, uint32_t site0,
                     hipStream_t st) {
  const dcf_config& c = m->cfg;
  const int E = c.E, To = T_in / stride, rows = B * To;
  const auto& d = *m->drop;
  TRY(enc_unfused_qkv(m, w, b, Xin, ldx, mask_in, B, T_in, stride, st));
  TRY(enc_unfused_attention(m, b, mask_out, B, To, st));
  // h = proj(ctx) -> R4;  x' = skip * mask + drop_path_attn(ls_attn * proj_drop(h))          (blocks.py:392, :586)
  GemmArgs gp = gemm(b.R[0], E, w.wp, w.bp, b.R[4], E, rows, E, E);
  TRY(run_gemm(m, &gp, 1, A_ROWS, st));
  DropResArgs ra{};
  ra.out = b.R[1]; ra.ldo = E;
  if (stride == 2) { ra.R = b.R[3]; ra.ldr = E; } else { ra.R = Xin; ra.ldr = ldx; }
  ra.H = b.R[4]; ra.ldh = E; ra.rowmask = mask_out; ra.res_mask = 1; ra.out_mask = 0; ra.ls = w.ls_attn;
  ra.rows = rows; ra.C = E; ra.T = To; ra.b0 = d.b0; ra.seed = d.seed;
  ra.drop = drop_at(m, DROP_R_VPROJ, site0 | DROP_PROJ); ra.path = drop_at(m, DROP_R_VPATH, site0 | DROP_PATH_ATTN);
  TRY(launch_drop_residual(ra, st));
  // FFN: dropout(gelu(fc(ln_ffn(x')))) -> proj -> R4;  out = x' + drop_path_ffn(ls_ffn * dropout(.) * mask)   (blocks.py:535-538, :589-590)
  LnArgs ln{}; ln.X = b.R[1]; ln.ldx = E; ln.Y = b.R[2]; ln.ldy = E; ln.w = w.ln_ffn_w; ln.b = w.ln_ffn_b; ln.rows = rows; ln.C = E;
  TRY(launch_ln(ln, st));
  GemmArgs gf = gemm(b.R[2], E, w.fc_w, w.fc_b, b.HID, 4 * E, rows, 4 * E, E);
  gf.flags = G_GELU;
  TRY(run_gemm(m, &gf, 1, A_ROWS, st));
  TRY(launch_dropout(b.HID, 4 * E, rows, 4 * E, To, d.b0, d.seed, drop_at(m, DROP_R_VPROJ, site0 | DROP_FFN_HID), st));
  GemmArgs go = gemm(b.HID, 4 * E, w.pj_w, w.pj_b, b.R[4], E, rows, E, 4 * E);
  TRY(run_gemm(m, &go, 1, A_ROWS, st));
  ra.out = Xout; ra.ldo = ldo; ra.R = b.R[1]; ra.ldr = E; ra.res_mask = 0; ra.out_mask = 1; ra.ls = w.ls_ffn;
  ra.drop = drop_at(m, DROP_R_VPROJ, site0 | DROP_FFN_OUT); ra.path = drop_at(m, DROP_R_VPATH, site0 | DROP_PATH_FFN);
  return launch_drop_residual(ra, st);
}

// XAttNFusion._forward (fusion.py:56-66) on one level of B sequences of T rows with the decoders' proj_drop on the (B', 2E, T)
// scale / shift tensor (sub 0), the FFN's two dropouts (1, 2) and drop_path_ffn (4); X updated in place, ln_out -> out
int run_fusion_drop(dcf_model* m, Buffers& b, float* X, int64_t ldx, int B, int T, const uint8_t* mask, const TextMeta* dm,
                    int Lk, float* out, int64_t ld_out, hipStream_t st) {
  const dcf_config& c = m->cfg;
  const int E = c.E, rows = B * T;
  const auto& d = *m->drop;
  for (size_t li = 0; li < m->dec.size(); ++li) {
    const DecW& w = m->dec[li];
    const uint32_t site0 = drop_site(DROP_G_FUSION, (uint32_t)li, 0);
    TextLnArgs tl{*dm, b.kvn, b.kvmask, w.ln_kv_w, w.ln_kv_b, Lk, c.TE};
    TRY(launch_text_ln(tl, B, st));
    GemmArgs gkv[2] = {gemm(b.kvn, c.TE, w.wk, w.bk, b.Kt, E, B * Lk, E, c.TE), gemm(b.kvn, c.TE, w.wv, w.bv, b.Vt, E, B * Lk, E, c.TE)};
    TRY(run_gemm(m, gkv, 2, A_ROWS, st));
    DecPreArgs dp{X, ldx, mask, w.ln_q_w, w.ln_q_b, w.dw, w.qn_w, w.qn_b, b.R[0], b.R[1], B, T, E};
    dp.nbr = nullptr;
    dp.affine = c.xattn_affine;
    TRY(launch_dec_pre(dp, st));
    GemmArgs gq = gemm(b.R[0], E, w.wq, w.bq, b.R[2], E, rows, E, E);
    TRY(run_gemm(m, &gq, 1, A_ROWS, st));
    XAttnArgs xa{b.R[2], b.Kt, b.Vt, b.kvmask, b.R[0], B, T, Lk, E, c.fusion_heads, m->status, c.attn_mode == 1};
    TRY(launch_xattn(xa, st));
    // (scale | shift) = proj_drop(proj(ctx)) -> H2;  q3 = adaln(q) * scale + shift -> R2, ln_ffn(q3) -> R0   (blocks.py:392, :643-646)
    GemmArgs gh = gemm(b.R[0], E, w.wp, w.bp, b.H2, 2 * E, rows, 2 * E, E);
    TRY(run_gemm(m, &gh, 1, A_ROWS, st));
    TRY(launch_dropout(b.H2, 2 * E, rows, 2 * E, T, d.b0, d.seed, drop_at(m, DROP_R_FPROJ, site0 | DROP_PROJ), st));
    TRY(launch_dec_mid(b.R[1], b.H2, w.ln_ffn_w, w.ln_ffn_b, b.R[2], b.R[0], rows, E, st));
    GemmArgs gf = gemm(b.R[0], E, w.fc_w, w.fc_b, b.HID, 4 * E, rows, 4 * E, E);
    gf.flags = G_GELU;
    TRY(run_gemm(m, &gf, 1, A_ROWS, st));
    TRY(launch_dropout(b.HID, 4 * E, rows, 4 * E, T, d.b0, d.seed, drop_at(m, DROP_R_FPROJ, site0 | DROP_FFN_HID), st));
    GemmArgs go = gemm(b.HID, 4 * E, w.pj_w, w.pj_b, b.R[1], E, rows, E, 4 * E);
    TRY(run_gemm(m, &go, 1, A_ROWS, st));
    // q = q3 + drop_path_ffn(ls_ffn * dropout(proj(.)) * mask)                                              (blocks.py:648-649)
    DropResArgs ra{};
    ra.out = X; ra.ldo = ldx; ra.R = b.R[2]; ra.ldr = E; ra.H = b.R[1]; ra.ldh = E; ra.rowmask = mask; ra.res_mask = 0; ra.out_mask = 1;
    ra.ls = w.ls_ffn; ra.rows = rows; ra.C = E; ra.T = T; ra.b0 = d.b0; ra.seed = d.seed;
    ra.drop = drop_at(m, DROP_R_FPROJ, site0 | DROP_FFN_OUT); ra.path = drop_at(m, DROP_R_FPATH, site0 | DROP_PATH_FFN);
    TRY(launch_drop_residual(ra, st));
  }
  LnArgs ln{}; ln.X = X; ln.ldx = ldx; ln.Y = out; ln.ldy = ld_out; ln.w = m->fus_out_w; ln.b = m->fus_out_b; ln.rows = rows; ln.C = E;
  return launch_ln(ln, st);
}

// From 16 384 level-0 rows on (one video of T = 16 384), in the f16x3 mode at E = 256 with two stride-1 embedding convolutions:
// embd_fc, both convolutions, their LayerNorms and + pe * mask as ONE kernel (embd_chain.h).  Not for late fusion (embd_fc takes
// the gated input there), the dropout forward, an armed debug tap, or a model whose folded weight left the fp16 range.
bool can_chain_embd(dcf_model* m, int rows0) {
  static const Setting off(nullptr, "DCF_NO_EMBD_CHAIN", 0, Setting::PRESENT);    // developer switch: the separate launches
  static const Setting min_rows("embd_chain_min_rows", "DCF_EMBD_CHAIN_MIN_ROWS", 16384);
  const dcf_config& c = m->cfg;
  return !off.get() && debug_option("embd_chain", 1) != 0 && m->gemm_terms == GEMM_F16X3 && c.E == 256 && c.model_kind != 1 &&
         vid_stride_of(c) == 1 && c.n_embd_convs == 2 && !m->drop && !m->keep_debug && m->embd_chain_w1[0] && m->embd_chain_w1[1] &&
         m->embd_chain_w2 && rows0 >= min_rows.get();
}
// priced at the two convolutions and at the rows in and out once: the folded embd_fc product is work the kernel does not do
int run_embd_chain(dcf_model* m, const float* X, int64_t ldx, const uint8_t* nbr, int rows, int T, bool ln_in, const float* pe, float* Y,
                   int64_t ldy, hipStream_t st) {
  const int E = m->cfg.E, v = ln_in ? 0 : 1;
  EmbdChainArgs a{};
  a.X = X; a.ldx = ldx; a.nbr = nbr; a.W1c = m->embd_chain_w1[v]; a.W2c = m->embd_chain_w2; a.cb = m->embd_chain_cb[v];
  a.ln1_w = m->embd_ln_w[0]; a.ln1_b = m->embd_ln_b[0]; a.ln2_w = m->embd_ln_w[1]; a.ln2_b = m->embd_ln_b[1];
  a.pe = pe; a.Y = Y; a.ldy = ldy; a.rows = rows; a.T = T; a.ln_in = ln_in ? 1 : 0; a.status = m->status;
  ProfScope prof("gemm_f16x3<embd_chain>", st, 2.0 * rows * 256.0 * 768.0 * 2.0, (double)rows * E * 4.0 * 2.0);
  return launch_embd_chain(a, st);
}

RefineArgs refine_args(dcf_model* m) {
  static const Setting stack("tcn_stack", "DCF_TCN_STACK", -1);     // developer switch: leading TCN layers per launch
  RefineArgs ra{};
  ra.w_in = m->tcn_in_w; ra.b_in = m->tcn_in_b;
  ra.host_w_dil = m->tcn_wd.data(); ra.host_b_dil = m->tcn_bd.data(); ra.host_w_pw = m->tcn_wp.data();
  ra.host_b_pw = m->tcn_bp.data(); ra.host_ln_w = m->tcn_lnw.data(); ra.host_ln_b = m->tcn_lnb.data();
  ra.w_out = m->tcn_out_w; ra.b_out = m->tcn_out_b;
  ra.host_frag = (!m->tcn_frag.empty() && debug_option("tcn_frag", 1) != 0) ? m->tcn_frag.data() : nullptr;
  ra.stack_layers = stack.get();                                       // (dcf_debug_set_option: 0 = layer by layer)
  ra.f16 = m->gemm_terms == GEMM_F16X3; ra.status = m->status;
  return ra;
}

}  // namespace dcf
