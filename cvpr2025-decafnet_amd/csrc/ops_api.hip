// Post-processing and single-operator entry points of the C ABI: what the tests and autograd.py call outside a forward.
#include <algorithm>

#include "../../include/decafnet_hip_embd.h"
#include "engine.h"

namespace dcf {
// one GEMM on the split-operand kernels, the weight's planes made for this call in stream-ordered scratch
static int split_gemm_once(GemmArgs g, GemmAMode mode, int nterms, hipStream_t st) {
  StreamScratch sc(st);
  unsigned short* planes = nullptr;
  if (sc.take(&planes, (size_t)3 * g.N * g.K)) return -1;
  int rc = launch_split_planes(g.W, planes, g.N, g.K, g.K, st, nterms);
  g.Ws = planes;
  if (rc == 0) rc = launch_gemm_split(&g, 1, mode, nterms, st);
  return sc.end(rc);
}
// a k3 convolution from the reference's (N, Cin, 3) weight: on the fp32 kernel (nterms = 0) or the split-operand one
static int conv3_once(const float* X, const uint8_t* mask, const float* W_ock, float* Y, int B, int T, int Cin, int N, int nterms,
                      hipStream_t st) {
  const int rows = B * T;
  StreamScratch sc(st);
  float* wp = nullptr;
  uint8_t* nbr = nullptr;
  unsigned short* planes = nullptr;              // stays null on the fp32 kernel
  if (sc.take(&wp, (size_t)N * Cin * 3) || sc.take(&nbr, (size_t)rows)) return -1;
  if (nterms && sc.take(&planes, (size_t)3 * N * Cin * 3)) return -1;
  launch_permute3(W_ock, wp, N, Cin, 3, 0, 2, 1, st);
  int rc = launch_rowflags(mask, nbr, T, rows, st);
  if (rc == 0 && nterms) rc = launch_split_planes(wp, planes, N, 3 * Cin, 3 * Cin, st, nterms);
  if (rc == 0) {
    GemmArgs g = gemm(X, Cin, wp, nullptr, Y, N, rows, N, 3 * Cin);
    g.cin = Cin; g.nbr = nbr; g.Ws = planes;
    rc = nterms ? launch_gemm_split(&g, 1, A_ROWS_TAP3, nterms, st) : launch_gemm(&g, 1, A_ROWS_TAP3, st);
  }
  return sc.end(rc);
}
}  // namespace dcf

extern "C" {

// ---- post-processing -------------------------------------------------------------------------
int dcf_collect_segments(const float* logits, const float* offsets, const uint8_t* masks, int32_t nq, int64_t T,
                         int32_t n_levels, float pre_nms_thresh, int32_t pre_nms_topk, float seg_len_thresh,
                         float* segs_out, float* scores_out, int32_t* counts_out, void* stream) {
  return dcf_collect_segments_ext(logits, offsets, masks, nullptr, nq, T, n_levels, pre_nms_thresh, pre_nms_topk, seg_len_thresh,
                                  segs_out, scores_out, counts_out, stream);
}

int dcf_collect_segments_ext(const float* logits, const float* offsets, const uint8_t* masks, const float* ext_scores,
                             int32_t nq, int64_t T, int32_t n_levels, float pre_nms_thresh, int32_t pre_nms_topk,
                             float seg_len_thresh, float* segs_out, float* scores_out, int32_t* counts_out, void* stream) {
  DCF_CHECK(logits && offsets && masks && segs_out && scores_out && counts_out, "dcf_collect_segments: null argument");
  DCF_CHECK(n_levels >= 1 && n_levels <= 16, "dcf_collect_segments: n_levels out of range");
  dcf::CollectArgs a{};
  a.logits = logits; a.offsets = offsets; a.masks = masks;
  a.ext = ext_scores; a.T = (int)T;
  int acc = 0;
  for (int l = 0; l < n_levels; ++l) { a.off[l] = acc; acc += (int)(T >> l); }
  a.off[n_levels] = acc;
  a.S = acc; a.n_levels = n_levels;
  a.pre_nms_thresh = pre_nms_thresh; a.seg_len_thresh = seg_len_thresh; a.pre_nms_topk = pre_nms_topk;
  a.segs = segs_out; a.scores = scores_out; a.counts = counts_out;
  dcf::StreamScratch sc((hipStream_t)stream);
  uint32_t* keys = nullptr;
  if (dcf::collect_needs_scratch(acc) && sc.take(&keys, (size_t)nq * acc)) return -1;
  a.keys = keys;
  return sc.end(dcf::launch_collect(a, nq, (hipStream_t)stream));
}

int dcf_nms_1d(const float* segs, const float* scores, const int32_t* counts, int32_t nq, int32_t n_max,
               int32_t stride, float iou_thresh, int64_t* keep_out, int32_t* keep_counts_out, void* stream) {
  DCF_CHECK(keep_out && keep_counts_out && (n_max == 0 || (segs && scores)), "dcf_nms_1d: null argument");
  dcf::NmsArgs a{segs, scores, counts, n_max, stride, iou_thresh, (long long*)keep_out, keep_counts_out};
  return dcf::launch_nms(a, nq, (hipStream_t)stream);
}

int dcf_softnms_1d(const float* segs, const float* scores, const int32_t* counts, int32_t nq, int32_t n_max,
                   int32_t stride, float iou_thresh, float sigma, float min_score, int32_t method,
                   int32_t max_iters, float* dets_out, int64_t* inds_out, int32_t* out_counts, void* stream) {
  DCF_CHECK(dets_out && inds_out && out_counts && (n_max == 0 || (segs && scores)), "dcf_softnms_1d: null argument");
  dcf::SoftNmsArgs a{segs, scores, counts, n_max, stride, iou_thresh, sigma, min_score, method, max_iters, dets_out,
                     (long long*)inds_out, out_counts};
  return dcf::launch_softnms(a, nq, (hipStream_t)stream);
}

int dcf_segment_voting(const float* nms_segs, int32_t nms_ld, const int32_t* n1_counts, int32_t n1_max,
                       int32_t n1_stride, const float* all_segs, const float* all_scores,
                       const int32_t* n2_counts, int32_t n2_max, int32_t n2_stride, float iou_thresh,
                       int32_t nq, float* out, void* stream) {
  DCF_CHECK(nms_segs && all_segs && all_scores && out, "dcf_segment_voting: null argument");
  dcf::VotingArgs a{nms_segs, nms_ld, n1_counts, n1_max, n1_stride, all_segs, all_scores, n2_counts, n2_max, n2_stride,
                    iou_thresh, out};
  return dcf::launch_voting(a, nq, (hipStream_t)stream);
}

// ---- single operators ---------------------------------------------------------------------------
int dcf_op_linear(const float* A, const float* W, const float* bias, float* C, int32_t M, int32_t N, int32_t K,
                  int32_t act, void* stream) {
  dcf::GemmArgs g = dcf::gemm(A, K, W, bias, C, N, M, N, K);
  g.flags = act == 1 ? dcf::G_GELU : act == 2 ? dcf::G_RELU : 0;
  return dcf::launch_gemm(&g, 1, dcf::A_ROWS, (hipStream_t)stream);
}

int dcf_op_linear_split(const float* A, const float* W, const float* bias, float* C, int32_t M, int32_t N, int32_t K,
                        int32_t act, int32_t nterms, void* stream) {
  dcf::GemmArgs g = dcf::gemm(A, K, W, bias, C, N, M, N, K);
  g.flags = act == 1 ? dcf::G_GELU : act == 2 ? dcf::G_RELU : 0;
  return dcf::split_gemm_once(g, dcf::A_ROWS, nterms, (hipStream_t)stream);
}

int dcf_op_linear_cm(const float* A_cm, const float* W, const float* bias, float* C, int32_t M, int32_t N, int32_t K,
                     void* stream) {
  dcf::GemmArgs g = dcf::gemm(A_cm, M, W, bias, C, N, M, N, K);
  return dcf::launch_gemm(&g, 1, dcf::A_CHANMAJOR, (hipStream_t)stream);
}

int dcf_op_linear_ln(const float* A, const float* W, const float* bias, const float* ln_w, const float* ln_b, float* C, float* Y,
                     int32_t M, int32_t N, int32_t K, int32_t relu, int32_t nterms, void* stream) {
  DCF_CHECK(dcf::gemm_can_fuse_ln(M, N, K, dcf::A_ROWS), "dcf_op_linear_ln: %dx%dx%d cannot carry a fused LayerNorm (N = 256, M >= 28672)", M, N, K);
  dcf::GemmArgs g = dcf::gemm(A, K, W, bias, C, N, M, N, K);
  g.ln_w = ln_w; g.ln_b = ln_b; g.Y = Y; g.ldy = N; g.ln_relu = relu;
  return dcf::split_gemm_once(g, dcf::A_ROWS, nterms, (hipStream_t)stream);
}

int dcf_op_linear_ln_carry(const float* A, const float* W1, const float* b1, const float* R, const float* ln_w, const float* ln_b,
                           const float* W2, const float* b2, float* X, float* Y, int32_t M, int32_t N1, int32_t K1, int32_t N2,
                           int32_t gelu, int32_t nterms, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  DCF_CHECK(A && W1 && ln_w && ln_b && W2 && X && Y, "dcf_op_linear_ln_carry: null argument");
  DCF_CHECK(N1 % 64 == 0 && dcf::gemm_can_carry_stats(M, N1, K1, 1, nterms) && dcf::gemm_can_carry_stats(M, N2, N1, 1, nterms),
            "dcf_op_linear_ln_carry: %dx%dx%d -> %d runs on the k-sliced kernel (no row statistics there)", M, N1, K1, N2);
  dcf::StreamScratch sc(st);
  unsigned short *p1 = nullptr, *p2 = nullptr;
  float *wf = nullptr, *stats = nullptr;
  if (sc.take(&p1, (size_t)3 * N1 * K1) || sc.take(&p2, (size_t)3 * N2 * N1)) return -1;
  if (sc.take(&wf, (size_t)N2 * N1 + 2 * (size_t)N2) || sc.take(&stats, (size_t)M * (N1 / 64) * 2)) return -1;
  float* sv = wf + (size_t)N2 * N1;
  dcf::launch_fold_ln(W2, b2, ln_w, ln_b, wf, sv, sv + N2, N2, N1, st);
  int rc = dcf::launch_split_planes(W1, p1, N1, K1, K1, st, nterms);
  if (rc == 0) rc = dcf::launch_split_planes(wf, p2, N2, N1, N1, st, nterms);
  if (rc == 0) {
    dcf::GemmArgs g = dcf::gemm(A, K1, W1, b1, X, N1, M, N1, K1);
    g.Ws = p1; g.stats_out = stats; g.stats_w = 64;
    if (R) { g.flags = dcf::G_RES; g.R = R; g.ldr = N1; }
    rc = dcf::launch_gemm_split(&g, 1, dcf::A_ROWS, nterms, st);
  }
  if (rc == 0) {
    dcf::GemmArgs g = dcf::gemm(X, N1, wf, sv + N2, Y, N2, M, N2, N1);
    g.Ws = p2; g.flags = gelu ? dcf::G_GELU : 0;
    g.stats_in = stats; g.ln_s = sv; g.stats_slots = N1 / 64; g.stats_w = 64;
    rc = dcf::launch_gemm_split(&g, 1, dcf::A_ROWS, nterms, st);
  }
  return sc.end(rc);
}

int dcf_op_ffn(const float* X, const float* ln_w, const float* ln_b, const float* W1, const float* b1, const float* W2, const float* b2,
               const float* ls, const uint8_t* mask, float* C, float* stats_out, int32_t M, int32_t E, int32_t chain, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  DCF_CHECK(X && W1 && b1 && W2 && b2 && C && M > 0 && E % 64 == 0, "dcf_op_ffn: bad argument");
  DCF_CHECK(!chain || E == 256, "dcf_op_ffn: the one-kernel form exists for E = 256 only");
  DCF_CHECK(chain >= 0 && chain <= 3, "dcf_op_ffn: chain = %d (0 .. 3)", chain);
  // (the one-kernel form reads a row twice -- as X and, a tile later, as the residual -- and the retry below re-reads X after C is written)
  DCF_CHECK(C != X, "dcf_op_ffn: C must not alias X");
  DCF_CHECK(!stats_out || chain || dcf::gemm_can_carry_stats(M, E, 4 * E, 1, dcf::GEMM_F16X3), "dcf_op_ffn: %d rows run on a kernel without row statistics", M);
  const int H = 4 * E, nterms = dcf::GEMM_F16X3;
  dcf::StreamScratch sc(st);
  unsigned short *p1 = nullptr, *p2 = nullptr;
  float *wf = nullptr, *stats = nullptr, *xn = nullptr, *hid = nullptr;
  if (sc.take(&p1, (size_t)3 * H * E) || sc.take(&p2, (size_t)3 * H * E)) return -1;
  const float *fc_w = W1, *fc_b = b1, *fc_s = nullptr, *fc_in = X;
  int rc = 0;
  if (ln_w && chain) {           // the LayerNorm rides as row statistics, its gain folded into the fc weight (GemmArgs::stats_in)
    if (sc.take(&wf, (size_t)H * E + 2 * (size_t)H) || sc.take(&stats, (size_t)M * (E / 64) * 2)) return -1;
    float* sv = wf + (size_t)H * E;
    dcf::launch_fold_ln(W1, b1, ln_w, ln_b, wf, sv, sv + H, H, E, st);
    rc = dcf::launch_row_stats(X, E, stats, M, E, 64, st);
    fc_w = wf; fc_s = sv; fc_b = sv + H;
  } else if (ln_w) {
    if (sc.take(&xn, (size_t)M * E)) return -1;
    dcf::LnArgs ln{}; ln.X = X; ln.ldx = E; ln.Y = xn; ln.ldy = E; ln.w = ln_w; ln.b = ln_b; ln.rows = M; ln.C = E;
    rc = dcf::launch_ln(ln, st);
    fc_in = xn;
  }
  if (rc == 0) rc = dcf::launch_split_planes(fc_w, p1, H, E, E, st, nterms);
  if (rc == 0) rc = dcf::launch_split_planes(W2, p2, E, H, H, st, nterms);
  if (rc == 0 && chain) {
    dcf::FfnChainArgs a{};
    a.X = X; a.ldx = E; a.W1s = p1; a.b1 = fc_b; a.ln_s = fc_s; a.stats = stats; a.stats_slots = E / 64; a.W2s = p2; a.b2 = b2; a.ls = ls;
    a.R = X; a.ldr = E; a.rowmask = mask; a.C = C; a.ldc = E; a.stats_out = stats_out; a.stats_w = 64; a.M = M;
    a.variant = chain == 1 ? 0 : chain - 1;        // chain 2: the four-wave kernel, 3: the eight-wave kernel
    // the sticky numerics word of this call (bit 1: common.h LN_ILL_RATIO): only a folded LayerNorm can raise it, and only then
    // does the call pay for the word and the wait
    unsigned* word = nullptr;
    unsigned flag = 0u;
    if (ln_w) {
      if (sc.take(&word, 1)) return -1;
      if (hipMemsetAsync(word, 0, sizeof(unsigned), st) != hipSuccess) { rc = -1; dcf::set_error("dcf_op_ffn: hipMemsetAsync failed"); }
    }
    a.status = word;
    if (rc == 0) rc = dcf::launch_ffn_chain(a, st);
    if (rc == 0 && word) {
      if (hipMemcpyAsync(&flag, word, sizeof(flag), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        rc = -1; dcf::set_error("dcf_op_ffn: reading the numerics word failed");
      }
    }
    if (rc == 0 && ln_w && (flag & 2u)) {
      // a row's mean dwarfs its spread: the folded one-pass statistics are not trustworthy for it -- what the engine does after
      // dcf_model_set_ln_carry(m, 0): the two-pass LayerNorm as its own launch, the same kernel on its output
      if (sc.take(&xn, (size_t)M * E)) return -1;
      dcf::LnArgs ln{}; ln.X = X; ln.ldx = E; ln.Y = xn; ln.ldy = E; ln.w = ln_w; ln.b = ln_b; ln.rows = M; ln.C = E;
      rc = dcf::launch_ln(ln, st);
      if (rc == 0) rc = dcf::launch_split_planes(W1, p1, H, E, E, st, nterms);
      a.X = xn; a.b1 = b1; a.ln_s = nullptr; a.stats = nullptr; a.status = nullptr;
      if (rc == 0) rc = dcf::launch_ffn_chain(a, st);
    }
  } else if (rc == 0) {
    if (sc.take(&hid, (size_t)M * H)) return -1;
    dcf::GemmArgs gf = dcf::gemm(fc_in, E, fc_w, fc_b, hid, H, M, H, E);
    gf.Ws = p1; gf.flags = dcf::G_GELU;
    rc = dcf::launch_gemm_split(&gf, 1, dcf::A_ROWS, nterms, st);
    if (rc == 0) {
      dcf::GemmArgs go = dcf::gemm(hid, H, W2, b2, C, E, M, E, H);
      go.Ws = p2; go.flags = dcf::G_RES | (mask ? dcf::G_OUT_MASK : 0); go.rowmask = mask; go.ls = ls; go.R = X; go.ldr = E;
      if (stats_out) { go.stats_out = stats_out; go.stats_w = 64; }
      rc = dcf::launch_gemm_split(&go, 1, dcf::A_ROWS, nterms, st);
    }
  }
  return sc.end(rc);
}

int dcf_op_linear_cm_split(const float* A_cm, const float* W, const float* bias, float* C, int32_t M, int32_t N, int32_t K,
                           int32_t nterms, void* stream) {
  return dcf::split_gemm_once(dcf::gemm(A_cm, M, W, bias, C, N, M, N, K), dcf::A_CHANMAJOR, nterms, (hipStream_t)stream);
}

int dcf_op_conv3(const float* X, const uint8_t* mask, const float* W_ock, float* Y, int32_t B, int32_t T, int32_t Cin, int32_t N, void* stream) {
  return dcf::conv3_once(X, mask, W_ock, Y, B, T, Cin, N, 0, (hipStream_t)stream);
}

int dcf_op_conv3_split(const float* X, const uint8_t* mask, const float* W_ock, float* Y, int32_t B, int32_t T, int32_t Cin,
                       int32_t N, int32_t nterms, void* stream) {
  return dcf::conv3_once(X, mask, W_ock, Y, B, T, Cin, N, nterms, (hipStream_t)stream);
}

int dcf_op_head(const float* X, const uint8_t* mask, const float* W1, const float* ln1_w, const float* ln1_b, const float* W2,
                const float* ln2_w, const float* ln2_b, const float* Wout, const float* bout, float* out, int32_t B, int32_t T,
                int32_t C, int32_t NO, float scale, int32_t chain, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  DCF_CHECK(X && mask && W1 && ln1_w && ln1_b && W2 && ln2_w && ln2_b && Wout && bout && out && B > 0 && T > 0, "dcf_op_head: null argument");
  DCF_CHECK((NO == 1 || NO == 2) && C % 32 == 0, "dcf_op_head: NO = %d, C = %d", NO, C);
  DCF_CHECK(!chain || dcf::head_chain_supports(C, NO), "dcf_op_head: the one-kernel form exists for C = 256 / 288 only");
  const int rows = B * T, nterms = dcf::GEMM_F16X3;
  float *wp[2] = {nullptr, nullptr}, *wo = nullptr, *ha = nullptr, *hb = nullptr;
  uint8_t* nbr = nullptr;
  unsigned short *img[2] = {nullptr, nullptr}, *woc = nullptr;
  dcf::StreamScratch sc(st);
  dcf::LevelTable lt{}, *d_lt = nullptr;
  lt.n_levels = 1; lt.B = B; lt.S = T; lt.T[0] = T; lt.start[0] = 0; lt.start[1] = rows; lt.off[0] = 0; lt.scale[0] = scale;
  if (sc.take(&d_lt, 1)) return -1;
  DCF_HIP(hipMemcpyAsync(d_lt, &lt, sizeof(lt), hipMemcpyHostToDevice, st));
  DCF_HIP(hipStreamSynchronize(st));                        // (lt is a stack object)
  if (sc.take(&nbr, (size_t)rows) || sc.take(&wo, (size_t)NO * C * 3)) return -1;
  const size_t img_halfs = chain ? dcf::head_chain_image_halfs(C) : (size_t)3 * C * C * 3;
  const float* Ws[2] = {W1, W2};
  int rc = dcf::launch_rowflags(mask, nbr, T, rows, st);
  for (int i = 0; i < 2 && rc == 0; ++i) {
    if (sc.take(&wp[i], (size_t)C * C * 3) || sc.take(&img[i], img_halfs)) return -1;
    dcf::launch_permute3(Ws[i], wp[i], C, C, 3, 0, 2, 1, st);
    rc = chain ? dcf::launch_split_chain3(wp[i], img[i], C, st) : dcf::launch_split_planes(wp[i], img[i], C, 3 * C, 3 * C, st, nterms);
  }
  dcf::launch_permute3(Wout, wo, NO, C, 3, 0, 2, 1, st);
  const int mode = scale != 0.f ? 1 : 0;                    // scale = 0: raw logits (ClsHead); otherwise relu(scale * y) (RegHead)
  if (rc == 0 && chain) {
    if (sc.take(&woc, dcf::head_chain_out_image_halfs(C))) return -1;
    rc = dcf::launch_split_chain_out(wo, NO, woc, C, st);
  }
  if (rc == 0 && chain) {
    dcf::HeadChainArgs a{};
    a.X = X; a.ldx = C; a.nbr = nbr; a.W1c = img[0]; a.W2c = img[1]; a.ln1_w = ln1_w; a.ln1_b = ln1_b; a.ln2_w = ln2_w; a.ln2_b = ln2_b;
    a.Wout = wo; a.Woc = woc; a.bout = bout; a.lt = d_lt; a.out = out; a.rows = rows; a.NO = NO; a.mode = mode; a.query_major = 0;
    rc = dcf::launch_head_chain(&a, 1, C, st);
  } else if (rc == 0) {
    if (sc.take(&ha, (size_t)rows * C) || sc.take(&hb, (size_t)rows * C)) return -1;
    const float* in = X;
    float* bufs[2] = {ha, hb};
    const float *lw[2] = {ln1_w, ln2_w}, *lb[2] = {ln1_b, ln2_b};
    for (int i = 0; i < 2 && rc == 0; ++i) {
      dcf::GemmArgs g = dcf::gemm(in, C, wp[i], nullptr, bufs[i], C, rows, C, 3 * C);
      g.cin = C; g.nbr = nbr; g.Ws = img[i];
      rc = dcf::launch_gemm_split(&g, 1, dcf::A_ROWS_TAP3, nterms, st);
      if (rc == 0) {
        dcf::LnArgs ln{}; ln.X = bufs[i]; ln.ldx = C; ln.Y = bufs[i]; ln.ldy = C; ln.w = lw[i]; ln.b = lb[i]; ln.rows = rows; ln.C = C; ln.relu = 1;
        rc = dcf::launch_ln(ln, st);
      }
      in = bufs[i];
    }
    if (rc == 0) {
      dcf::ConvOutArgs co{};
      co.X = in; co.ldx = C; co.nbr = nbr; co.W = wo; co.bias = bout; co.lt = d_lt; co.out = out; co.rows = rows; co.C = C; co.NO = NO;
      co.row0 = 0; co.mode = mode; co.query_major = 0;
      rc = dcf::launch_conv_out(co, st);
    }
  }
  return sc.end(rc);
}

int dcf_op_layernorm(const float* X, const float* w, const float* b, float* Y, int32_t rows, int32_t C, int32_t relu,
                     void* stream) {
  dcf::LnArgs a{};
  a.X = X; a.ldx = C; a.Y = Y; a.ldy = C; a.w = w; a.b = b; a.rows = rows; a.C = C; a.relu = relu;
  return dcf::launch_ln(a, (hipStream_t)stream);
}

int dcf_op_xattn(const float* Q, const float* K, const float* V, const uint8_t* kvmask, float* O, int32_t B, int32_t T,
                 int32_t Lk, int32_t C, int32_t heads, void* stream) {
  dcf::XAttnArgs a{Q, K, V, kvmask, O, B, T, Lk, C, heads};
  return dcf::launch_xattn(a, (hipStream_t)stream);
}

int dcf_op_local_attn(const float* Q, const float* K, const float* V, const uint8_t* mask, float* O, int32_t B, int32_t T,
                      int32_t C, int32_t heads, int32_t window, void* stream) {
  if (window == 0) {
    dcf::GlobalAttnArgs g{Q, K, V, mask, O, B, T, C, heads};
    return dcf::launch_global_attn(g, (hipStream_t)stream);
  }
  dcf::LocalAttnArgs a{Q, K, V, mask, O, B, T, C, heads, window};
  return dcf::launch_local_attn(a, (hipStream_t)stream);
}

int dcf_op_local_attn_bwd(const float* Q, const float* K, const float* V, const uint8_t* mask, const float* dO, float* dQ, float* dK,
                          float* dV, int32_t B, int32_t T, int32_t C, int32_t heads, int32_t window, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  dcf::LocalAttnGradArgs a{Q, K, V, mask, dO, dQ, dK, dV, nullptr, B, T, C, heads, window};
  DCF_CHECK(B > 0 && T > 0 && heads > 0, "dcf_op_local_attn_bwd: empty batch (B=%d T=%d heads=%d)", B, T, heads);
  if (!dK && !dV) return dcf::launch_local_attn_bwd(a, st);
  // the row statistics the key-side gather reads: stream-ordered scratch, no host wait
  dcf::StreamScratch sc(st);
  if (sc.take(&a.stats, dcf::local_attn_grad_stats_floats((int64_t)B * T, heads))) return -1;
  return sc.end(dcf::launch_local_attn_bwd(a, st));
}

int dcf_op_sidekick(const float* shallow, const float* text_cls, float* correl, int32_t D, int32_t T, int32_t nq,
                    int32_t norm, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  dcf::StreamScratch sc(st);
  float *tn = nullptr, *partial = nullptr;
  if (sc.take(&tn, (size_t)nq * D) || sc.take(&partial, (size_t)dcf::SCORE_SLICES * (nq + 1) * T)) return -1;
  return sc.end(dcf::launch_sidekick(dcf::score_args(shallow, text_cls, tn, partial, correl, D, T, nq, norm), st));
}

int dcf_op_gate(const float* correl, const uint8_t* vid_mask, float* gate, uint8_t* mask_out, int32_t T, int32_t nq,
                int32_t sn, double sratio, int32_t msf, void* stream) {
  dcf::GateArgs a{correl, vid_mask, gate, mask_out, T, nq, 0, sn, msf, sratio};
  return dcf::launch_gate(a, (hipStream_t)stream);
}

// ---- composite blocks on a scratch model (parity tests against the reference's operator fixtures) ----------------
namespace dcf {
// a scratch model holds only the bound parameters of one block: never finalized, its packed images are dropped after every call
static int scratch_begin(dcf_model* m, const char* what, hipStream_t st) {
  DCF_CHECK(m && !m->finalized, "%s: needs a scratch model (dcf_model_create + dcf_model_bind of the block's parameters, not finalized)", what);
  return init_gemm_mode(m, st);
}
static int scratch_end(dcf_model* m, hipStream_t st, int rc) {
  (void)hipStreamSynchronize(st);
  free_packed(m);
  m->dec.clear();
  m->fus_out_w = m->fus_out_b = nullptr;
  return rc;
}
struct ScratchArena {
  char* base = nullptr;
  ~ScratchArena() { if (base) (void)hipFree(base); }
};
}  // namespace dcf

int dcf_op_encoder(dcf_model* m, const char* prefix, const float* X, const uint8_t* mask, int32_t B, int32_t T, int32_t stride,
                   float* Y, uint8_t* mask_out, void* stream) {
  using namespace dcf;
  hipStream_t st = (hipStream_t)stream;
  DCF_CHECK(prefix && X && mask && Y && mask_out && B >= 1 && T >= 1 && (stride == 1 || stride == 2) && T % stride == 0, "dcf_op_encoder: bad arguments");
  if (scratch_begin(m, "dcf_op_encoder", st)) return -1;
  const dcf_config& c = m->cfg;
  const int half = c.win / 2;
  DCF_CHECK(half == 0 || (T / stride) % half == 0, "dcf_op_encoder: T / stride = %d must be a multiple of win//2 = %d (blocks.py:216)", T / stride, half);
  EncW w{};
  int rc = resolve_encoder(m, prefix, c.E, st, w);
  ScratchArena sa;
  if (rc == 0) {
    Buffers b{};
    const size_t need = carve_at(nullptr, c, T, B, B, T, 1, 1, b);
    if (hipMalloc(&sa.base, need) != hipSuccess) { set_error("dcf_op_encoder: out of memory"); rc = -1; }
    if (rc == 0) {
      carve_at(sa.base, c, T, B, B, T, 1, 1, b);
      if (stride == 2) rc = launch_mask_down(mask, mask_out, B * T / 2, st);
      else if (hipMemcpyAsync(mask_out, mask, (size_t)B * T, hipMemcpyDeviceToDevice, st) != hipSuccess) rc = -1;
      if (rc == 0) rc = run_encoder(m, w, b, X, c.E, mask, mask_out, B, T, stride, Y, c.E, st);
    }
  }
  return scratch_end(m, st, rc);
}

int dcf_op_enc_pre(dcf_model* m, const char* prefix, const float* X, const uint8_t* mask, int32_t B, int32_t T, int32_t stride,
                   float* Qc, float* Kc, float* Vc, float* Skip, void* stream) {
  using namespace dcf;
  hipStream_t st = (hipStream_t)stream;
  DCF_CHECK(prefix && X && mask && Qc && Kc && Vc && B >= 1 && T >= 1 && (stride == 1 || (stride == 2 && Skip)) && T % stride == 0, "dcf_op_enc_pre: bad arguments");
  if (scratch_begin(m, "dcf_op_enc_pre", st)) return -1;
  EncW w{};
  int rc = resolve_encoder(m, prefix, m->cfg.E, st, w);
  if (rc == 0) {
    EncPreArgs ep = enc_pre_args(w, X, m->cfg.E, mask, B, T, m->cfg.E);
    ep.Qc = Qc; ep.Kc = Kc; ep.Vc = Vc; ep.Skip = stride == 2 ? Skip : nullptr;
    rc = launch_enc_pre(ep, stride, st);
  }
  return scratch_end(m, st, rc);
}

int dcf_op_decoder(dcf_model* m, const char* prefix, float* X, const uint8_t* mask, int32_t B, int32_t T,
                   const float* const* text, const uint8_t* const* text_mask, const int32_t* text_len, void* stream) {
  using namespace dcf;
  hipStream_t st = (hipStream_t)stream;
  DCF_CHECK(prefix && X && mask && text && text_len && B >= 1 && B <= DCF_MAX_BATCH && T >= 1, "dcf_op_decoder: bad arguments");
  if (scratch_begin(m, "dcf_op_decoder", st)) return -1;
  const dcf_config& c = m->cfg;
  DecW w{};
  int rc = resolve_decoder(m, prefix, c.E, c.TE, st, w);
  ScratchArena sa;
  if (rc == 0) {
    m->dec.assign(1, w);
    m->fus_out_w = m->fus_out_b = nullptr;
    int Lk = 1;
    TextMeta tm{};
    for (int i = 0; i < B; ++i) {
      tm.text[i] = text[i]; tm.text_mask[i] = text_mask ? text_mask[i] : nullptr; tm.len[i] = text_len[i];
      Lk = std::max(Lk, (int)text_len[i]);
    }
    Buffers b{};
    const size_t need = carve_at(nullptr, c, T, B, B, T, Lk, 1, b);
    if (hipMalloc(&sa.base, need) != hipSuccess) { set_error("dcf_op_decoder: out of memory"); rc = -1; }
    if (rc == 0) carve_at(sa.base, c, T, B, B, T, Lk, 1, b);
    if (rc == 0) rc = run_fusion(m, b, X, c.E, B, T, nullptr, mask, nullptr, &tm, Lk, X, c.E, st);
  }
  return scratch_end(m, st, rc);
}

int dcf_op_tcn(dcf_model* m, const char* prefix, const float* x, const uint8_t* mask, int32_t B, int32_t T, int32_t n_in,
               int32_t n_layers, float* Y, void* stream) {
  using namespace dcf;
  hipStream_t st = (hipStream_t)stream;
  DCF_CHECK(prefix && x && mask && Y && B >= 1 && T >= 1 && n_in >= 1 && n_in <= DCF_MAX_LEVELS && n_layers >= 0, "dcf_op_tcn: bad arguments");
  if (scratch_begin(m, "dcf_op_tcn", st)) return -1;
  int rc = resolve_tcn(m, prefix, n_in, n_layers, st);
  float* buf = nullptr;
  if (rc == 0 && hipMalloc(&buf, (size_t)2 * B * T * TCN_HID * sizeof(float)) != hipSuccess) { set_error("dcf_op_tcn: out of memory"); rc = -1; }
  if (rc == 0) {
    LevelTable lt{};
    lt.n_levels = n_in; lt.B = B; lt.T[0] = T; lt.S = T;
    RefineArgs ra = refine_args(m);
    ra.stacked = x; ra.mask_all = mask;
    ra.bufA = buf; ra.bufB = buf + (size_t)B * T * TCN_HID; ra.F = Y; ra.ldf = TCN_HID; ra.E = 0;
    ra.B = B; ra.T0 = T; ra.n_levels = n_in; ra.n_layers = n_layers;
    rc = launch_refine(ra, lt, st);
  }
  rc = scratch_end(m, st, rc);
  if (buf) (void)hipFree(buf);
  return rc;
}

// ---- the embedding-stage extension (include/decafnet_hip_embd.h): on a finalized model's own parameters
int dcf_embd_ext_version(void) { return DCF_EMBD_EXT_VERSION; }

static int embd_op_check(const dcf_model* m, const char* what, const float* X, int64_t ldx, const uint8_t* mask, int B, int T, const float* Y, int64_t ldy) {
  DCF_CHECK(m && X && mask && Y && B >= 1 && T >= 1 && (int64_t)B * T < (1ll << 31), "%s: null argument or bad B / T", what);
  DCF_CHECK(m->finalized, "%s: the model is not finalized", what);
  const dcf_config& c = m->cfg;
  DCF_CHECK(c.model_kind != 1 && dcf::vid_stride_of(c) == 1 && c.n_embd_convs == 2 && c.E == 256 && m->gemm_terms == dcf::GEMM_F16X3,
            "%s: needs an early-fusion model with E = 256, vid_net.stride 1 and two embedding convolutions in the f16x3 mode", what);
  DCF_CHECK(X != Y && ldx >= c.E && ldy >= c.E && ldx % 4 == 0 && ldy % 4 == 0, "%s: X and Y must differ, pitches multiples of 4 and >= E", what);
  return 0;
}

int dcf_op_embd_chain(dcf_model* m, const float* X, int64_t ldx, const uint8_t* mask, int32_t B, int32_t T, int32_t ln_in,
                      const float* pe, float* Y, int64_t ldy, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (embd_op_check(m, "dcf_op_embd_chain", X, ldx, mask, B, T, Y, ldy)) return -1;
  DCF_CHECK(m->embd_chain_w1[0] && m->embd_chain_w1[1] && m->embd_chain_w2,
            "dcf_op_embd_chain: the model has no images of the folded embedding stage (a folded weight left the scaled fp16 range)");
  const int rows = B * T;
  dcf::StreamScratch sc(st);
  uint8_t* nbr = nullptr;
  if (sc.take(&nbr, (size_t)rows)) return -1;
  int rc = dcf::launch_rowflags(mask, nbr, T, rows, st);
  if (rc == 0) rc = dcf::run_embd_chain(m, X, ldx, nbr, rows, T, ln_in != 0, pe, Y, ldy, st);
  return sc.end(rc);
}

int dcf_op_embd_launches(dcf_model* m, const float* X, int64_t ldx, const uint8_t* mask, int32_t B, int32_t T, int32_t ln_in,
                         const float* pe, float* Y, int64_t ldy, void* stream) {
  using namespace dcf;
  hipStream_t st = (hipStream_t)stream;
  if (embd_op_check(m, "dcf_op_embd_launches", X, ldx, mask, B, T, Y, ldy)) return -1;
  const int rows = B * T, E = m->cfg.E;
  StreamScratch sc(st);
  uint8_t* nbr = nullptr;
  float *t0 = nullptr, *t1 = nullptr;
  if (sc.take(&nbr, (size_t)rows) || sc.take(&t0, (size_t)rows * E) || sc.take(&t1, (size_t)rows * E)) return -1;
  int rc = launch_rowflags(mask, nbr, T, rows, st);
  const float* xin = X;
  int64_t ldin = ldx;
  if (rc == 0 && ln_in) {
    LnArgs ln{}; ln.X = X; ln.ldx = ldx; ln.Y = t0; ln.ldy = E; ln.w = m->fus_out_w; ln.b = m->fus_out_b; ln.rows = rows; ln.C = E;
    rc = launch_ln(ln, st);
    xin = t0; ldin = E;
  }
  if (rc == 0) {
    GemmArgs ge = gemm(xin, ldin, m->embd_fc_w, m->embd_fc_b, t1, E, rows, E, E);
    ge.flags = G_AMASK; ge.rowmask = mask;
    rc = run_gemm(m, &ge, 1, A_ROWS, st);
  }
  for (int i = 0; i < 2 && rc == 0; ++i) {
    GemmArgs g = gemm(t1, E, m->embd_conv[i], nullptr, t0, E, rows, E, 3 * E);
    g.cin = E; g.nbr = nbr;
    rc = run_gemm(m, &g, 1, A_ROWS_TAP3, st);
    if (rc) break;
    LnArgs ln{}; ln.X = t0; ln.ldx = E; ln.Y = i == 1 ? Y : t1; ln.ldy = i == 1 ? ldy : E; ln.w = m->embd_ln_w[i]; ln.b = m->embd_ln_b[i];
    ln.rows = rows; ln.C = E; ln.relu = 1;
    if (i == 1 && pe) { ln.pe = pe; ln.mask = mask; ln.T = T; }
    rc = launch_ln(ln, st);
  }
  return sc.end(rc);
}

}  // extern "C"
