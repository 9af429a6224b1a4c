// Internal to the engine's translation units (not installed): the model, its workspace and the functions that cross files.
// engine_model.hip: options, profiler, parameter table, finalize; engine_blocks.hip: workspace, plans, GEMM dispatch, block runners;
// engine.hip: forward(), graph capture, text_encode; engine_hybrid.hip: dcf_hybrid_phase*; ops_api.hip: post-processing, dcf_op_*.
#pragma once
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/decafnet_hip.h"
#include "attn.h"
#include "attn_grad.h"
#include "common.h"
#include "dec_chain.h"
#include "dropout.h"
#include "embd_chain.h"
#include "enc_chain.h"
#include "ffn_chain.h"
#include "gemm.h"
#include "head_chain.h"
#include "heads.h"
#include "postproc.h"
#include "rowops.h"
#include "score.h"

namespace dcf {

struct Bound {
  const float* p = nullptr;
  std::vector<int64_t> shape;
  int64_t numel() const {
    int64_t n = 1;
    for (auto s : shape) n *= s;
    return n;
  }
};

struct EncW {   // one TransformerEncoder of vid_net
  const float *ln_attn_w, *ln_attn_b, *dw_q, *dw_k, *dw_v, *qn_w, *qn_b, *kn_w, *kn_b, *vn_w, *vn_b;
  const float *wq, *bq, *wk, *bk, *wv, *bv, *wp, *bp, *ls_attn;
  const float *ln_ffn_w, *ln_ffn_b, *fc_w, *fc_b, *pj_w, *pj_b, *ls_ffn;
  const float *fc_wf, *fc_s, *fc_c;          // ffn.fc with ln_ffn folded in (k_fold_ln); nullptr where not built
  // enc_chain.hip: query / key / value with q / k / v_norm folded in, as chain images + the fold's s[n], c[n]; nullptr where not built
  const unsigned short* qkv_chain[3];
  const float *qkv_s[3], *qkv_c[3];
  const unsigned short* wp_chain;            // chain image of attn.proj (enc_chain.hip k_enc_attn) or nullptr
};
struct DecW {   // one TransformerDecoder of the fusion
  const float *ln_q_w, *ln_q_b, *ln_kv_w, *ln_kv_b, *dw, *qn_w, *qn_b;
  const float *wq, *bq, *wk, *bk, *wv, *bv, *wp, *bp;
  const float *wp_il, *bp_il;                // xattn.proj with its output rows in blocks of (32 scale rows, 32 shift rows of the same channels)
  const float *ln_ffn_w, *ln_ffn_b, *fc_w, *fc_b, *pj_w, *pj_b, *ls_ffn;
  const float *fc_wf, *fc_s, *fc_c;          // ffn.fc with ln_ffn folded in
  const unsigned short *wq_chain, *wp_chain; // chain images of xattn.query / the interleaved xattn.proj (dec_chain.hip) or nullptr
};
struct TextEncW {   // one TransformerEncoder of text_net (stride 0: no depthwise convs, global attention)
  const float *ln_attn_w, *ln_attn_b, *wq, *bq, *wk, *bk, *wv, *bv, *wp, *bp, *ls_attn;
  const float *ln_ffn_w, *ln_ffn_b, *fc_w, *fc_b, *pj_w, *pj_b, *ls_ffn;
};
struct HeadW {
  std::vector<const float*> conv;            // packed [N][3][Cin]
  std::vector<const float*> ln_w, ln_b;
  const float* out_w;                        // packed [NO][3][Cin]
  const float* out_b;
  const unsigned short* chain[2] = {nullptr, nullptr};   // chain images of the two trunk convolutions (head_chain.hip) or nullptr
  const unsigned short* out_chain = nullptr;             // ... and of the output convolution
};

// opt.model.vid_net.stride (video_net.py:39): the embedding convolutions divide the sequence by it; 0 (older callers) reads as 1
static inline int vid_stride_of(const dcf_config& c) { return c.vid_stride > 1 ? c.vid_stride : 1; }

struct Plan {    // geometry for one (T0, B, levels)
  int T0 = 0, B = 0, L = 0;
  LevelTable lt{};
  LevelTable* d_lt = nullptr;
};

struct HybridState;

}  // namespace dcf

struct dcf_model {
  dcf_config cfg{};
  std::unordered_map<std::string, dcf::Bound> bound;
  std::vector<float*> owned;                 // packed weights
  std::unordered_map<const float*, const unsigned short*> wsplit;   // fp32 weight -> [3][N][K] bf16 planes
  std::unordered_map<const float*, int64_t> wsplit_ldw;             // row pitch of the fp32 weight the planes were made from
  std::unordered_map<const float*, int> wsplit_terms;               // mode the image of a weight was made for (16 / 6)
  int gemm_terms = 16;                       // 16: f16x3 split MFMA GEMM (default); 6: bf16x6; 0: native fp32 MFMA
  bool force_x6 = false;                     // a weight did not fit the scaled fp16 range: the model runs bf16x6
  bool no_ln_carry = false;                  // dcf_model_set_ln_carry(m, 0): every LayerNorm as its own two-pass launch
  int option_epoch = 0;                      // option_epoch() the captured graphs were recorded under
  unsigned* status = nullptr;                // device words: [0] sticky numerics flag of the f16x3 GEMMs, [1] weight range flag
  bool finalized = false;
  const float* pe = nullptr;
  int64_t pe_T = 0;

  // resolved weights
  const float *vid_map_w = nullptr, *vid_map_b = nullptr;
  // column blocks of the (E, Din) vid_map weight: expert half, sidekick half, the scat column (model.py:543-551)
  const float *vid_w1 = nullptr, *vid_w2 = nullptr, *vid_w3 = nullptr;
  int64_t vid_ldw = 0;
  std::vector<dcf::DecW> dec;
  const float *fus_out_w = nullptr, *fus_out_b = nullptr;
  const float *embd_fc_w = nullptr, *embd_fc_b = nullptr;
  const float *embd_fc_wf = nullptr, *embd_fc_s = nullptr, *embd_fc_c = nullptr;   // vid_net.embd_fc with fusion.ln_out folded in
  std::vector<const float*> embd_conv, embd_ln_w, embd_ln_b;
  // the embedding stage as one kernel (embd_chain.h): embd_fc folded into embd_convs[0] as a chain image + the per-tap bias [3][E],
  // [0] for the raw stream (fusion.ln_out's affine folded in too, the kernel normalises), [1] for rows that come normalised; the
  // chain image of embd_convs[1].  nullptr where not built, or where a folded weight leaves the scaled fp16 range.
  const unsigned short* embd_chain_w1[2] = {nullptr, nullptr};
  const float* embd_chain_cb[2] = {nullptr, nullptr};
  const unsigned short* embd_chain_w2 = nullptr;
  std::vector<dcf::EncW> stem, branch;
  std::vector<const float*> pool_w;          // vid_net.pool_only: depthwise k3 weight [3][E] of every branch layer (video_net.py:107-109)
  dcf::HeadW cls1, cls2, reg;
  std::vector<float> reg_scales;             // host copy of reg_head.scales.{l}.scale
  const float *tcn_in_w = nullptr, *tcn_in_b = nullptr, *tcn_out_w = nullptr, *tcn_out_b = nullptr;
  std::vector<const float*> tcn_wd, tcn_bd, tcn_wp, tcn_bp, tcn_lnw, tcn_lnb;
  std::vector<const unsigned short*> tcn_frag;   // f16x3: MFMA fragment image of every TCN layer (launch_tcn_frag_image)
  // text_net (TextTransformer, text_net.py:92-188); empty when cfg.text_layers == 0
  const float *text_embd_w = nullptr, *text_embd_b = nullptr, *text_bkgd = nullptr;
  dcf::TextEncW text_pool{};                      // TextIdentity: attn_pool.attn.{query,key,value,proj} (text_net.py:50-53)
  std::vector<dcf::TextEncW> text_enc;
  const float* text_pe = nullptr;            // (text_pe_L, TE) token-major, borrowed
  int64_t text_pe_L = 0;
  char* text_ws = nullptr;
  size_t text_ws_bytes = 0;
  // half features (decafnet_hip_half.h) of a forward that cannot read them natively: their fp32 copies, vid then shallow of every video;
  // between forwards the scratch of dcf_select_videos (scores' partial sums, the masks side by side): stream order keeps the two apart
  char* half_ws = nullptr;
  size_t half_ws_bytes = 0;

  // workspace
  char* arena = nullptr;
  size_t arena_bytes = 0;
  std::vector<dcf::Plan> plans;
  // HIP graph of the last repeated forward (same pointers and sizes): one graph launch replaces ~135 kernel launches,
  // so a busy host cannot starve the GPU.  Captured on the second identical call, dropped whenever anything it bakes
  // in changes (weights, position encoding, workspace).
  std::vector<uint64_t> last_key, graph_key;
  hipGraph_t graph = nullptr;
  hipGraphExec_t graph_exec = nullptr;
  bool capturing = false;
  int graph_mode = 0;                        // dcf_model_set_graph_mode: 0 auto (by size), 1 always, 2 never
  std::vector<uint64_t> nocapture_key;       // argument set whose capture failed: run it eagerly, do not retry every call
  int last_launch = 0;                       // how the last forward was issued: 0 eager, 1 graph replay, 2 graph capture + launch
  // The legacy default stream (NULL: what torch's default stream is) cannot be captured.  A forward called on it hops to
  // this engine-owned non-blocking stream, ordered after / before the caller's stream by two events, so that the
  // reference's calling pattern (one stream, one video per call) replays a graph too.
  hipStream_t own = nullptr;
  hipEvent_t ev_in = nullptr, ev_out = nullptr;
  // last-forward bookkeeping for dcf_debug_copy
  struct {
    float *correl = nullptr, *gate = nullptr, *vidmap = nullptr, *fused = nullptr, *F = nullptr;
    int nq = 0, T0 = 0, B = 0, S = 0;
  } dbg;
  dcf::HybridState* hyb = nullptr;         // one long video sharded at pyramid level k (dcf_hybrid_phase1 / 2 / 3)
  int hyb_levels = 0;                        // > 0 while phase 1 runs: the forward builds levels 0 .. hyb_levels - 1 and stops behind the encoder
  size_t hyb_extra = 0;                      // bytes of workspace behind the forward's own buffers (the coarse pyramid)
  char* hyb_extra_ptr = nullptr;
  float* hyb_feat_out = nullptr;
  float* dbg_vidmap = nullptr;
  float* dbg_fused = nullptr;
  int64_t dbg_cap = 0;                        // capacity (floats) of the armed tap destinations
  bool keep_debug = false;
  // dcf_model_set_dropout: the training forward's dropout / drop-path (dropout.h).  `drop` points at `drop_state` only while
  // dcf_forward_train_videos runs with a rate above 0; every other entry point sees nullptr and its launch sequence of before.
  struct DropState {
    float p[5] = {0.f, 0.f, 0.f, 0.f, 0.f};     // vid proj, vid path, fusion proj, fusion path, refine (DROP_R_*)
    float scale[5] = {1.f, 1.f, 1.f, 1.f, 1.f}; // 1.0f / (1.0f - p), fp32
    uint64_t seed = 0;
    bool active = false;
    int b0 = 0;                                // first (video, query) row of the chunk being run
  } drop_state;
  DropState* drop = nullptr;
};

namespace dcf {

// ---- workspace ------------------------------------------------------------------------------
struct Arena {
  char* base;
  size_t off = 0, cap;
  bool dry;
  template <typename T>
  T* take(size_t n) {
    off = (off + 255) & ~(size_t)255;
    T* p = dry ? nullptr : reinterpret_cast<T*>(base + off);
    off += n * sizeof(T);
    return p;
  }
};

struct Buffers {
  float *P1, *P2, *tn, *partial, *correl, *gate;
  uint8_t *mask_all, *nbr_all, *kvmask, *maskv;
  uint8_t* tile_flags;                        // [B][(T0 + 63) / 64] 64-clip row tiles a query's gate keeps (GateArgs::tile_flags)
  uint8_t *mask_pre, *nbr_pre;                // vid_net.stride > 1: masks / neighbour flags of the input-resolution levels T0, T0/2, .. T0/stride
  float* col5;                                // vid_net.stride > 1: [B*T0/2][5E] rows of a k5 / stride-2 embedding convolution
  float *X, *R[7], *H2, *HID, *F, *HA, *HB, *HC, *HD, *logits1, *tcnA, *tcnB, *kvn, *Kt, *Vt;
  unsigned short* kvimg;                      // [B] K / V^T fragment images of the projected text (dec_chain.hip)
  float* kmadd;                               // [B][64] additive key mask
  float* stats;                               // [rows][E / 64] (sum, sum of squares): row statistics carried between GEMMs
  float* hstats[2];                           // the same for the k3 trunks (heads over the whole pyramid, embedding convolutions)
};

// The videos of one forward: all padded to the same T, video v with nq[v] queries; the queries of all videos are one flat
// list (text / outputs in video order).  One video is the reference's call (model.py:496 asserts bs == 1); several are
// the throughput extension dcf_forward_eval_videos: after vid_map every kernel works on rows [query][t] and does not
// care which video a query belongs to.
constexpr int DCF_MAX_VIDEOS = 16;
struct VideoSet {
  int nvid = 0;
  const float* vid[DCF_MAX_VIDEOS];
  const float* shallow[DCF_MAX_VIDEOS];
  const uint8_t* mask[DCF_MAX_VIDEOS];
  const float* text_cls[DCF_MAX_VIDEOS];      // (nq[v], D); with gate_override: the gate (nq, T)
  int nq[DCF_MAX_VIDEOS];
  float* logits1_out = nullptr;               // optional (nq, S): the logits of the first cls_head (fpn_logits1, model.py:445,471)
  bool half = false;                          // vid[] / shallow[] carry the addresses of IEEE binary16 values (decafnet_hip_half.h)
};

// what a forward reads besides the videos and where its results go: passed unchanged from the entry points down to forward()
struct ForwardCall {
  const float* const* text; const uint8_t* const* text_mask; const int32_t* text_len;
  const float* gate;                          // nullptr, or the externally selected gate (nq, T) of dcf_forward_eval_gated / dcf_hybrid_phase1
  float *logits, *offsets; uint8_t* masks;
  // dcf_forward_eval_selected (with `gate`): the expert features of the selected clips only, clip-major fp32 rows (sel_n, D), and
  // sel_pos (T) int32, the row of clip t among them or -1 (dcf_op_select_clips); the video's vid pointer is null
  const float* sel_rows = nullptr; const int32_t* sel_pos = nullptr; int sel_n = 0;
  // dcf_forward_eval_videos_selected: several videos, vs.nvid of them: sel_rows holds the rows of all of them, video v's from row
  // sel_first[v] on (sel_first[nvid] = sel_n), sel_pos is (nvid, T) and video-local; sel_first = nullptr is the one-video form.
  // sel_correl (nq, T): the sidekick scores a scat model needs, handed over by the caller (dcf_select_videos wrote them)
  const int32_t* sel_first = nullptr; const float* sel_correl = nullptr;
};

// the level-cut state of dcf_hybrid_phase1 / 2 / 3 (engine_hybrid.hip)
struct HybridState {
  bool valid = false;
  int k = 0, Tn = 0, Tc = 0, B = 0, Lk = 0;
  Buffers bn{};
  Plan pn{}, pc{}, pch{};                     // narrow pyramid; coarse pyramid (levels k .. L-1); its levels k+1 .. (what the heads see)
  float *Fc = nullptr, *logits1c = nullptr, *stacked = nullptr;
  uint8_t *maskc = nullptr, *nbrc = nullptr;
};

static inline GemmArgs gemm(const float* A, int64_t lda, const float* W, const float* bias, float* C, int64_t ldc, int M, int N,
                            int K) {
  GemmArgs g{};
  g.A = A; g.lda = lda; g.W = W; g.ldw = 0; g.bias = bias; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K;
  return g;
}

#define TRY(x) do { if ((x) != 0) return -1; } while (0)
constexpr int STATS_W = 64;                   // channels per slot of the row statistics carried between GEMMs
enum { DROP_R_VPROJ = 0, DROP_R_VPATH, DROP_R_FPROJ, DROP_R_FPATH, DROP_R_REFINE };

// ---- engine_model.hip
const char* last_error();
int debug_option(const char* name, int dflt);
int option_epoch();
bool profiling_on();
// A developer / test setting: the value dcf_debug_set_option gave `opt` (nullptr: no such option), else the environment variable
// `env` -- read once, when the Setting is made: keep it in a function-local static --, else `dflt`.
class Setting {
 public:
  enum Kind { VALUE, PRESENT };               // of the variable: its integer value / 1 where it is set at all (DCF_NO_...)
  Setting(const char* opt, const char* env, int dflt, Kind kind = VALUE);
  int get() const;
 private:
  const char* opt_; int base_;
};
void launch_permute3(const float* src, float* dst, int d0, int d1, int d2, int p0, int p1, int p2, hipStream_t st);
void launch_fold_ln(const float* W, const float* bias, const float* g, const float* beta, float* Wf, float* s, float* c, int N, int K,
                    hipStream_t st);
void drop_graph(dcf_model* m, bool keep_last_key = false);
void free_packed(dcf_model* m);
int init_gemm_mode(dcf_model* m, hipStream_t st);
int resolve_encoder(dcf_model* m, const std::string& p, int E, hipStream_t st, EncW& w);
int resolve_decoder(dcf_model* m, const std::string& p, int E, int TE, hipStream_t st, DecW& w);
int resolve_tcn(dcf_model* m, const std::string& pre, int n_in, int n_layers, hipStream_t st);

// ---- engine_blocks.hip
size_t carve_at(char* base, const dcf_config& c, int T0, int B, int nq, int S, int Lk, int nvid, Buffers& b, size_t extra = 0,
                char** extra_ptr = nullptr);
int get_plan(dcf_model* m, int T0, int B, int L, hipStream_t st, Plan** out);
int make_plan(dcf_model* m, Plan& p, const int* Tl, int n, int B, const float* scales, hipStream_t st);
int run_gemm(dcf_model* m, GemmArgs* g, int count, GemmAMode mode, hipStream_t st);
bool can_fuse_ln(dcf_model* m, const float* W, int M, int N, int K, GemmAMode mode);
bool can_norm_a(dcf_model* m, const float* W1, const float* W2, int M, int C, int* stats_w);
void norm_a(GemmArgs& g, const float* stats, int C, int stats_w, const float* ln_g, const float* ln_b);
EncPreArgs enc_pre_args(const EncW& w, const float* X, int64_t ldx, const uint8_t* mask_in, int B, int T_in, int E);
int run_encoder(dcf_model* m, const EncW& w, Buffers& b, const float* Xin, int64_t ldx, const uint8_t* mask_in,
                const uint8_t* mask_out, int B, int T_in, int stride, float* Xout, int64_t ldo, hipStream_t st);
int run_encoder_drop(dcf_model* m, const EncW& w, Buffers& b, const float* Xin, int64_t ldx, const uint8_t* mask_in,
                     const uint8_t* mask_out, int B, int T_in, int stride, float* Xout, int64_t ldo, uint32_t site0, hipStream_t st);
int run_head(dcf_model* m, const HeadW& h, Buffers& b, const Plan& pl, int Cin, int NO, int mode, int query_major, float* out,
             hipStream_t st, int row0 = 0, int rows = -1);
int run_head_pair(dcf_model* m, const HeadW& h1, const HeadW& h2, Buffers& b, const Plan& pl, int Cin, int NO1, int mode1,
                  float* out1, int NO2, int mode2, float* out2, hipStream_t st);
int run_fusion(dcf_model* m, Buffers& b, float* X, int64_t ldx, int B, int T, const LevelTable* lt, const uint8_t* mask,
               const uint8_t* nbr, const TextMeta* dm, int Lk, float* out, int64_t ld_out, hipStream_t st, bool* carry_out = nullptr);
int run_fusion_drop(dcf_model* m, Buffers& b, float* X, int64_t ldx, int B, int T, const uint8_t* mask, const TextMeta* dm, int Lk,
                    float* out, int64_t ld_out, hipStream_t st);
RefineArgs refine_args(dcf_model* m);
bool can_chain_embd(dcf_model* m, int rows0);
int run_embd_chain(dcf_model* m, const float* X, int64_t ldx, const uint8_t* nbr, int rows, int T, bool ln_in, const float* pe, float* Y,
                   int64_t ldy, hipStream_t st);

// ---- engine.hip
int forward(dcf_model* m, const VideoSet& vs, int T0, int nq, const ForwardCall& fc, hipStream_t st);
int launch_gather_masks(const uint8_t* const* masks, int nvid, uint8_t* dst, int T0, hipStream_t st);   // dst (nvid, T0)
int grow_half_ws(dcf_model* m, size_t need, hipStream_t st);     // m->half_ws holds at least `need` bytes afterwards
void launch_masks_out(const uint8_t* mask_all, uint8_t* out, const LevelTable* lt, const unsigned* status, float* logits, int rows,
                      hipStream_t st);

// ---- half.hip
int launch_half_to_f32(const uint16_t* src, float* dst, int64_t n, hipStream_t st);

// ---- engine_hybrid.hip
void free_hybrid(dcf_model* m);
int hybrid_take(dcf_model* m, const Buffers& b, const Plan& pl, int B, int Lk, hipStream_t st);

}  // namespace dcf
