// The model behind the C ABI: the thread's error string, the developer / test options, the per-launch profiler, the parameter
// table (bound by reference state_dict name) and finalize, which resolves it and repacks the weights.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <atomic>
#include <mutex>

#include "engine.h"

namespace dcf {

static thread_local std::string g_err;
void set_error(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
}
const char* last_error() { return g_err.c_str(); }

// ---- developer / test options (dcf_debug_set_option): named integers that override a built-in threshold, e.g. the row count from
// which a chain kernel replaces its launches, so that the operator tests can send small fixtures through the large-grid kernels
static std::unordered_map<std::string, int>& debug_options() {
  static std::unordered_map<std::string, int> o;
  return o;
}
static std::mutex& debug_options_mutex() {
  static std::mutex mu;
  return mu;
}
// bumped by every dcf_debug_set_option: a model whose captured graphs were recorded under another epoch drops them (the options
// choose kernels, a replay would keep running the old choice)
static std::atomic<int> g_option_epoch{0};
int option_epoch() { return g_option_epoch.load(); }
int debug_option(const char* name, int dflt) {
  std::lock_guard<std::mutex> lock(debug_options_mutex());
  auto& o = debug_options();
  auto it = o.find(name);
  return it == o.end() ? dflt : it->second;
}
Setting::Setting(const char* opt, const char* env, int dflt, Kind kind) : opt_(opt), base_(dflt) {
  const char* v = env ? getenv(env) : nullptr;
  if (v) base_ = kind == PRESENT ? 1 : atoi(v);
}
int Setting::get() const { return opt_ ? debug_option(opt_, base_) : base_; }

// ---- per-launch profiler (dcf_profile_*) --------------------------------------------------
struct ProfRec { std::string name; hipEvent_t a, b; double flops, bytes; };
static bool g_prof_on = false;
static std::vector<ProfRec> g_recs;
bool profiling_on() { return g_prof_on; }

ProfScope::ProfScope(const char* name, hipStream_t s, double flops, double bytes) : idx(-1), st(s) {
  if (!g_prof_on) return;
  ProfRec r{name, nullptr, nullptr, flops, bytes};
  if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) return;
  (void)hipEventRecord(r.a, st);
  g_recs.push_back(r);
  idx = (int)g_recs.size() - 1;
}
ProfScope::~ProfScope() {
  if (idx >= 0) (void)hipEventRecord(g_recs[idx].b, st);
}

// ---- tiny utility kernels ------------------------------------------------------------------
// dst[perm(i0,i1,i2)] = src[i0][i1][i2];  p0..p2 give the destination axis order
__global__ void k_permute3(const float* __restrict__ src, float* __restrict__ dst, int d0, int d1, int d2, int p0, int p1,
                           int p2) {
  const int n = d0 * d1 * d2;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int idx[3];
  idx[0] = i / (d1 * d2);
  idx[1] = (i / d2) % d1;
  idx[2] = i % d2;
  const int dims[3] = {d0, d1, d2};
  const int perm[3] = {p0, p1, p2};
  const int o = (idx[perm[0]] * dims[perm[1]] + idx[perm[1]]) * dims[perm[2]] + idx[perm[2]];
  dst[o] = src[i];
}
void launch_permute3(const float* src, float* dst, int d0, int d1, int d2, int p0, int p1, int p2, hipStream_t st) {
  const size_t n = (size_t)d0 * d1 * d2;
  hipLaunchKernelGGL(k_permute3, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, dst, d0, d1, d2, p0, p1, p2);
}

// LayerNorm folded into the 1x1 convolution that consumes it (GemmArgs::stats_in): Wf[n][k] = W[n][k] g[k],
// s[n] = sum_k Wf[n][k], c[n] = bias[n] + sum_k beta[k] W[n][k].  One wave per output channel.
__global__ __launch_bounds__(64) void k_fold_ln(const float* __restrict__ W, const float* __restrict__ bias, const float* __restrict__ g,
                                                const float* __restrict__ beta, float* __restrict__ Wf, float* __restrict__ s,
                                                float* __restrict__ c, int K) {
  const int n = blockIdx.x, lane = threadIdx.x;
  float a1 = 0.f, a2 = 0.f;
  for (int k = lane; k < K; k += 64) {
    const float w = W[(int64_t)n * K + k];
    const float wf = w * g[k];
    Wf[(int64_t)n * K + k] = wf;
    a1 += wf;
    a2 += beta[k] * w;
  }
  a1 = wave_sum(a1);
  a2 = wave_sum(a2);
  if (lane == 0) { s[n] = a1; c[n] = (bias ? bias[n] : 0.f) + a2; }
}
void launch_fold_ln(const float* W, const float* bias, const float* g, const float* beta, float* Wf, float* s, float* c, int N, int K,
                    hipStream_t st) {
  hipLaunchKernelGGL(k_fold_ln, dim3(N), dim3(64), 0, st, W, bias, g, beta, Wf, s, c, K);
}

// vid_net.embd_fc folded into the first embedding convolution (embd_chain.h), formed in fp64 and rounded once:
//   d[j] = sum_k Wfc[j][k] beta[k] + b_fc[j];   Wf[n][tap][k] = (sum_j Wc[n][tap][j] Wfc[j][k]) g[k];   cb[tap][n] = sum_j Wc[n][tap][j] d[j]
// Wc: the packed convolution [E][3][E]; g / beta: fusion.ln_out's affine, or nullptr (1 / 0).  One block per (n, tap), E threads.
__global__ void k_fold_embd_d(const float* __restrict__ Wfc, const float* __restrict__ bfc, const float* __restrict__ beta, double* __restrict__ d, int E) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= E) return;
  double a = bfc[j];
  if (beta)
    for (int k = 0; k < E; ++k) a += (double)Wfc[(int64_t)j * E + k] * (double)beta[k];
  d[j] = a;
}
__global__ void k_fold_embd(const float* __restrict__ Wc, const float* __restrict__ Wfc, const float* __restrict__ g, const double* __restrict__ d,
                            float* __restrict__ Wf, float* __restrict__ cb, int E) {
  const int n = blockIdx.x / 3, tap = blockIdx.x - 3 * n, k = threadIdx.x;
  const float* wc = Wc + ((int64_t)n * 3 + tap) * E;
  double a = 0.;
  for (int j = 0; j < E; ++j) a += (double)wc[j] * (double)Wfc[(int64_t)j * E + k];
  Wf[((int64_t)n * 3 + tap) * E + k] = (float)(g ? a * (double)g[k] : a);
  if (k == 0) {
    double c = 0.;
    for (int j = 0; j < E; ++j) c += (double)wc[j] * d[j];
    cb[(int64_t)tap * E + n] = (float)c;
  }
}

void drop_graph(dcf_model* m, bool keep_last_key) {
  if (m->graph_exec) (void)hipGraphExecDestroy(m->graph_exec);
  if (m->graph) (void)hipGraphDestroy(m->graph);
  m->graph_exec = nullptr;
  m->graph = nullptr;
  m->graph_key.clear();
  if (!keep_last_key) m->last_key.clear();
}

// the packed weights and images that finalize (or one dcf_op_* call on a scratch model) made
void free_packed(dcf_model* m) {
  for (float* p : m->owned) (void)hipFree(p);
  m->owned.clear();
  m->wsplit.clear();
  m->wsplit_ldw.clear();
  m->wsplit_terms.clear();
}

static int free_model(dcf_model* m) {
  drop_graph(m);
  if (m->status) (void)hipFree(m->status);
  m->status = nullptr;
  free_packed(m);
  for (auto& pl : m->plans) if (pl.d_lt) (void)hipFree(pl.d_lt);
  m->plans.clear();
  free_hybrid(m);                             // (the level-cut state of dcf_hybrid_phase1 / 2 / 3)
  if (m->arena) (void)hipFree(m->arena);
  if (m->text_ws) (void)hipFree(m->text_ws);
  if (m->half_ws) (void)hipFree(m->half_ws);
  if (m->ev_in) (void)hipEventDestroy(m->ev_in);
  if (m->ev_out) (void)hipEventDestroy(m->ev_out);
  if (m->own) (void)hipStreamDestroy(m->own);
  return 0;
}

static int get(dcf_model* m, const std::string& name, std::initializer_list<int64_t> shape, const float** out) {
  auto it = m->bound.find(name);
  DCF_CHECK(it != m->bound.end(), "parameter '%s' is not bound", name.c_str());
  const Bound& b = it->second;
  int64_t want = 1;
  for (auto s : shape) want *= s;
  DCF_CHECK(b.numel() == want, "parameter '%s' has %lld elements, expected %lld", name.c_str(), (long long)b.numel(),
            (long long)want);
  *out = b.p;
  return 0;
}

// repack a 3-d tensor [d0][d1][d2] with destination axis order (p0,p1,p2); result owned by the model
static int pack3(dcf_model* m, const float* src, int d0, int d1, int d2, int p0, int p1, int p2, hipStream_t st,
                 const float** out) {
  float* dst = nullptr;
  const size_t n = (size_t)d0 * d1 * d2;
  DCF_HIP(hipMalloc(&dst, n * sizeof(float)));
  m->owned.push_back(dst);
  launch_permute3(src, dst, d0, d1, d2, p0, p1, p2, st);
  DCF_HIP(hipGetLastError());
  *out = dst;
  return 0;
}

// bf16 planes of a GEMM weight [N][K] (row pitch K); owned by the model
static int split_weight(dcf_model* m, const float* W, int N, int K, hipStream_t st, int64_t ldw = 0, int terms = 0) {
  if (m->gemm_terms == 0 || m->wsplit.count(W)) return 0;
  if (!terms) terms = m->gemm_terms;
  unsigned short* planes = nullptr;
  DCF_HIP(hipMalloc(&planes, (size_t)3 * N * K * sizeof(unsigned short)));
  m->owned.push_back(reinterpret_cast<float*>(planes));
  if (launch_split_planes(W, planes, N, K, ldw ? ldw : K, st, terms, m->status ? m->status + 1 : nullptr)) return -1;
  m->wsplit[W] = planes;
  m->wsplit_ldw[W] = ldw ? ldw : K;
  m->wsplit_terms[W] = terms;
  return 0;
}
#define SPLIT(W, N, K) do { if (split_weight(m, (W), (N), (K), st)) return -1; } while (0)

// the (N, K) weight W / bias of a 1x1 convolution behind LayerNorm(g, beta): folded copies owned by the model (+ weight image)
static int fold_ln(dcf_model* m, const float* W, const float* bias, const float* g, const float* beta, int N, int K, hipStream_t st,
                   const float** wf, const float** s_out, const float** c_out) {
  float* buf = nullptr;
  DCF_HIP(hipMalloc(&buf, ((size_t)N * K + 2 * (size_t)N) * sizeof(float)));
  m->owned.push_back(buf);
  float* sv = buf + (size_t)N * K;
  launch_fold_ln(W, bias, g, beta, buf, sv, sv + N, N, K, st);
  DCF_HIP(hipGetLastError());
  *wf = buf; *s_out = sv; *c_out = sv + N;
  return split_weight(m, buf, N, K, st);
}

#define GET(name, shape, dst) do { if (get(m, (name), shape, &(dst))) return -1; } while (0)
#define SH(...) std::initializer_list<int64_t>{__VA_ARGS__}

int resolve_encoder(dcf_model* m, const std::string& p, int E, hipStream_t st, EncW& w) {
  const float* t;
  GET(p + ".ln_attn.weight", SH(E), w.ln_attn_w); GET(p + ".ln_attn.bias", SH(E), w.ln_attn_b);
  GET(p + ".attn.q_conv.conv.weight", SH(E, 3), t); if (pack3(m, t, 1, E, 3, 0, 2, 1, st, &w.dw_q)) return -1;
  GET(p + ".attn.k_conv.conv.weight", SH(E, 3), t); if (pack3(m, t, 1, E, 3, 0, 2, 1, st, &w.dw_k)) return -1;
  GET(p + ".attn.v_conv.conv.weight", SH(E, 3), t); if (pack3(m, t, 1, E, 3, 0, 2, 1, st, &w.dw_v)) return -1;
  GET(p + ".attn.q_norm.weight", SH(E), w.qn_w); GET(p + ".attn.q_norm.bias", SH(E), w.qn_b);
  GET(p + ".attn.k_norm.weight", SH(E), w.kn_w); GET(p + ".attn.k_norm.bias", SH(E), w.kn_b);
  GET(p + ".attn.v_norm.weight", SH(E), w.vn_w); GET(p + ".attn.v_norm.bias", SH(E), w.vn_b);
  GET(p + ".attn.attn.query.weight", SH(E, E), w.wq); GET(p + ".attn.attn.query.bias", SH(E), w.bq);
  GET(p + ".attn.attn.key.weight", SH(E, E), w.wk); GET(p + ".attn.attn.key.bias", SH(E), w.bk);
  GET(p + ".attn.attn.value.weight", SH(E, E), w.wv); GET(p + ".attn.attn.value.bias", SH(E), w.bv);
  GET(p + ".attn.attn.proj.weight", SH(E, E), w.wp); GET(p + ".attn.attn.proj.bias", SH(E), w.bp);
  GET(p + ".drop_path_attn.scale", SH(E), w.ls_attn);
  GET(p + ".ln_ffn.weight", SH(E), w.ln_ffn_w); GET(p + ".ln_ffn.bias", SH(E), w.ln_ffn_b);
  GET(p + ".ffn.fc.weight", SH(4 * E, E), w.fc_w); GET(p + ".ffn.fc.bias", SH(4 * E), w.fc_b);
  GET(p + ".ffn.proj.weight", SH(E, 4 * E), w.pj_w); GET(p + ".ffn.proj.bias", SH(E), w.pj_b);
  GET(p + ".drop_path_ffn.scale", SH(E), w.ls_ffn);
  SPLIT(w.wq, E, E); SPLIT(w.wk, E, E); SPLIT(w.wv, E, E); SPLIT(w.wp, E, E);
  SPLIT(w.fc_w, 4 * E, E); SPLIT(w.pj_w, E, 4 * E);
  w.fc_wf = w.fc_s = w.fc_c = nullptr;
  if (m->gemm_terms != 0 && E % 64 == 0 && fold_ln(m, w.fc_w, w.fc_b, w.ln_ffn_w, w.ln_ffn_b, 4 * E, E, st, &w.fc_wf, &w.fc_s, &w.fc_c)) return -1;
  for (int i = 0; i < 3; ++i) { w.qkv_chain[i] = nullptr; w.qkv_s[i] = w.qkv_c[i] = nullptr; }
  w.wp_chain = nullptr;
  if (m->gemm_terms == GEMM_F16X3 && enc_chain_supports(E, m->cfg.vid_heads, m->cfg.win > 0 ? m->cfg.win : 99)) {
    {
      unsigned short* img = nullptr;
      DCF_HIP(hipMalloc(&img, chain1_image_halfs(E, E) * sizeof(unsigned short)));
      m->owned.push_back(reinterpret_cast<float*>(img));
      if (launch_split_chain1(w.wp, img, E, E, st, nullptr)) return -1;          // (range: the same weights passed split_weight above)
      w.wp_chain = img;
    }
    const float* W3[3] = {w.wq, w.wk, w.wv};
    const float* B3[3] = {w.bq, w.bk, w.bv};
    const float* G3[3] = {w.qn_w, w.kn_w, w.vn_w};
    const float* H3[3] = {w.qn_b, w.kn_b, w.vn_b};
    for (int i = 0; i < 3; ++i) {
      const float* wf;
      if (fold_ln(m, W3[i], B3[i], G3[i], H3[i], E, E, st, &wf, &w.qkv_s[i], &w.qkv_c[i])) return -1;
      unsigned short* img = nullptr;
      DCF_HIP(hipMalloc(&img, chain1_image_halfs(E, E) * sizeof(unsigned short)));
      m->owned.push_back(reinterpret_cast<float*>(img));
      if (launch_split_chain1(wf, img, E, E, st, m->status ? m->status + 1 : nullptr)) return -1;     // (the gain widens the weight's range)
      w.qkv_chain[i] = img;
    }
  }
  return 0;
}

// TransformerDecoder parameters (blocks.py:594-630) under prefix p
int resolve_decoder(dcf_model* m, const std::string& p, int E, int TE, hipStream_t st, DecW& w) {
  const float* t;
  GET(p + ".ln_xattn_q.weight", SH(E), w.ln_q_w); GET(p + ".ln_xattn_q.bias", SH(E), w.ln_q_b);
  GET(p + ".ln_xattn_kv.weight", SH(TE), w.ln_kv_w); GET(p + ".ln_xattn_kv.bias", SH(TE), w.ln_kv_b);
  GET(p + ".xattn.q_conv.conv.weight", SH(E, 3), t); if (pack3(m, t, 1, E, 3, 0, 2, 1, st, &w.dw)) return -1;
  GET(p + ".xattn.q_norm.weight", SH(E), w.qn_w); GET(p + ".xattn.q_norm.bias", SH(E), w.qn_b);
  GET(p + ".xattn.xattn.query.weight", SH(E, E), w.wq); GET(p + ".xattn.xattn.query.bias", SH(E), w.bq);
  GET(p + ".xattn.xattn.key.weight", SH(E, TE), w.wk); GET(p + ".xattn.xattn.key.bias", SH(E), w.bk);
  GET(p + ".xattn.xattn.value.weight", SH(E, TE), w.wv); GET(p + ".xattn.xattn.value.bias", SH(E), w.bv);
  GET(p + ".xattn.xattn.proj.weight", SH(2 * E, E), w.wp); GET(p + ".xattn.xattn.proj.bias", SH(2 * E), w.bp);
  GET(p + ".ln_ffn.weight", SH(E), w.ln_ffn_w); GET(p + ".ln_ffn.bias", SH(E), w.ln_ffn_b);
  GET(p + ".ffn.fc.weight", SH(4 * E, E), w.fc_w); GET(p + ".ffn.fc.bias", SH(4 * E), w.fc_b);
  GET(p + ".ffn.proj.weight", SH(E, 4 * E), w.pj_w); GET(p + ".ffn.proj.bias", SH(E), w.pj_b);
  GET(p + ".drop_path_ffn.scale", SH(E), w.ls_ffn);
  SPLIT(w.wq, E, E); SPLIT(w.wk, E, TE); SPLIT(w.wv, E, TE); SPLIT(w.wp, 2 * E, E);
  SPLIT(w.fc_w, 4 * E, E); SPLIT(w.pj_w, E, 4 * E);
  w.fc_wf = w.fc_s = w.fc_c = nullptr;
  if (m->gemm_terms != 0 && E % 128 == 0 && fold_ln(m, w.fc_w, w.fc_b, w.ln_ffn_w, w.ln_ffn_b, 4 * E, E, st, &w.fc_wf, &w.fc_s, &w.fc_c)) return -1;
  // the same projection for the GEMM that applies the modulation in its epilogue (G_ADALN): rows (2, E / 32, 32) -> (E / 32, 2, 32)
  w.wp_il = w.bp_il = nullptr;
  if (E % 32 == 0) {
    if (pack3(m, w.wp, 2, E / 32, 32 * E, 1, 0, 2, st, &w.wp_il)) return -1;
    if (pack3(m, w.bp, 2, E / 32, 32, 1, 0, 2, st, &w.bp_il)) return -1;
    SPLIT(w.wp_il, 2 * E, E);
  }
  // the attention half of the layer as one kernel (dec_chain.hip): chain-order fragment images of the two projections
  w.wq_chain = w.wp_chain = nullptr;
  if (m->gemm_terms == GEMM_F16X3 && w.wp_il && dec_chain_supports(E, m->cfg.fusion_heads, 1)) {
    unsigned short *iq = nullptr, *ip = nullptr;
    DCF_HIP(hipMalloc(&iq, chain1_image_halfs(E, E) * sizeof(unsigned short)));
    m->owned.push_back(reinterpret_cast<float*>(iq));
    DCF_HIP(hipMalloc(&ip, chain1_image_halfs(2 * E, E) * sizeof(unsigned short)));
    m->owned.push_back(reinterpret_cast<float*>(ip));
    if (launch_split_chain1(w.wq, iq, E, E, st, nullptr)) return -1;          // (range: the same weights passed split_weight above)
    if (launch_split_chain1(w.wp_il, ip, 2 * E, E, st, nullptr)) return -1;
    w.wq_chain = iq; w.wp_chain = ip;
  }
  return 0;
}

// TCN parameters (tcn.py:40-64) under prefix p: in (32, n_in, 1) -> [n_in][32]; dilated (32,32,3) -> [3][ci][co];
// 1x1 (32,32,1) -> [ci][co]
int resolve_tcn(dcf_model* m, const std::string& pre, int n_in, int n_layers, hipStream_t st) {
  const float* t;
  m->tcn_wd.clear(); m->tcn_bd.clear(); m->tcn_wp.clear(); m->tcn_bp.clear(); m->tcn_lnw.clear(); m->tcn_lnb.clear();
  GET(pre + ".conv_1x1.weight", SH(TCN_HID, n_in), t); if (pack3(m, t, 1, TCN_HID, n_in, 0, 2, 1, st, &m->tcn_in_w)) return -1;
  GET(pre + ".conv_1x1.bias", SH(TCN_HID), m->tcn_in_b);
  for (int i = 0; i < n_layers; ++i) {
    const std::string p = pre + ".layers." + std::to_string(i);
    const float* pk;
    GET(p + ".conv_dilated.weight", SH(TCN_HID, TCN_HID, 3), t);
    if (pack3(m, t, TCN_HID, TCN_HID, 3, 2, 1, 0, st, &pk)) return -1;
    m->tcn_wd.push_back(pk);
    GET(p + ".conv_dilated.bias", SH(TCN_HID), t); m->tcn_bd.push_back(t);
    GET(p + ".conv_1x1.weight", SH(TCN_HID, TCN_HID), t);
    if (pack3(m, t, 1, TCN_HID, TCN_HID, 0, 2, 1, st, &pk)) return -1;
    m->tcn_wp.push_back(pk);
    if (m->gemm_terms == GEMM_F16X3) {                   // the layers run in f16x3 too: same weight range, same fallback
      if (launch_f16_weight_range(m->tcn_wd.back(), 3 * TCN_HID * TCN_HID, m->status ? m->status + 1 : nullptr, st)) return -1;
      if (launch_f16_weight_range(m->tcn_wp.back(), TCN_HID * TCN_HID, m->status ? m->status + 1 : nullptr, st)) return -1;
    }
    GET(p + ".conv_1x1.bias", SH(TCN_HID), t); m->tcn_bp.push_back(t);
    GET(p + ".norm.weight", SH(TCN_HID), t); m->tcn_lnw.push_back(t);
    GET(p + ".norm.bias", SH(TCN_HID), t); m->tcn_lnb.push_back(t);
  }
  GET(pre + ".conv_out.weight", SH(TCN_HID, TCN_HID), t);
  if (pack3(m, t, 1, TCN_HID, TCN_HID, 0, 2, 1, st, &m->tcn_out_w)) return -1;
  if (m->gemm_terms == GEMM_F16X3 && launch_f16_weight_range(m->tcn_out_w, TCN_HID * TCN_HID, m->status ? m->status + 1 : nullptr, st)) return -1;
  GET(pre + ".conv_out.bias", SH(TCN_HID), m->tcn_out_b);
  m->tcn_frag.clear();
  if (m->gemm_terms == GEMM_F16X3) {                     // the layers' weight fragments once per model, not once per workgroup
    for (int i = 0; i < n_layers; ++i) {
      unsigned short* img = nullptr;
      DCF_HIP(hipMalloc(&img, (size_t)TCN_FRAG_HALFS * sizeof(unsigned short)));
      m->owned.push_back(reinterpret_cast<float*>(img));
      if (launch_tcn_frag_image(m->tcn_wd[i], m->tcn_wp[i], i + 1 == n_layers ? m->tcn_out_w : nullptr, img, st)) return -1;
      m->tcn_frag.push_back(img);
    }
  }
  return 0;
}

// dense-conv arithmetic of the model (dcf_config.gemm_mode) and its status words
int init_gemm_mode(dcf_model* m, hipStream_t st) {
  const int gm = m->cfg.gemm_mode;
  DCF_CHECK(gm == 0 || gm == 1 || gm == 6 || gm == 16, "gemm_mode %d: use 0 / 16 (f16x3), 6 (bf16x6) or 1 (fp32); the bf16x3 mode was replaced by f16x3", gm);
  m->gemm_terms = gm == 1 ? 0 : (gm == 6 ? GEMM_BF16X6 : GEMM_F16X3);
  if (m->force_x6 && m->gemm_terms == GEMM_F16X3) m->gemm_terms = GEMM_BF16X6;
  if (!m->status) DCF_HIP(hipMalloc(&m->status, 2 * sizeof(unsigned)));
  DCF_HIP(hipMemsetAsync(m->status, 0, 2 * sizeof(unsigned), st));
  return 0;
}

static int resolve_head(dcf_model* m, const std::string& p, const std::string& out_name, int C, int NO, int layers,
                        hipStream_t st, HeadW& h) {
  const float* t;
  for (int i = 0; i < layers; ++i) {
    const std::string s = std::to_string(i);
    GET(p + ".convs." + s + ".conv.weight", SH(C, C, 3), t);
    const float* pk;
    if (pack3(m, t, C, C, 3, 0, 2, 1, st, &pk)) return -1;      // (N, Cin, 3) -> [N][3][Cin]
    SPLIT(pk, C, 3 * C);
    h.conv.push_back(pk);
    const float *lw, *lb;
    GET(p + ".norms." + s + ".weight", SH(C), lw); GET(p + ".norms." + s + ".bias", SH(C), lb);
    h.ln_w.push_back(lw); h.ln_b.push_back(lb);
  }
  GET(p + "." + out_name + ".conv.weight", SH(NO, C, 3), t);
  if (pack3(m, t, NO, C, 3, 0, 2, 1, st, &h.out_w)) return -1;
  GET(p + "." + out_name + ".conv.bias", SH(NO), h.out_b);
  h.chain[0] = h.chain[1] = h.out_chain = nullptr;
  if (m->gemm_terms == GEMM_F16X3 && layers == 2 && head_chain_supports(C, NO)) {      // the whole head as one kernel (head_chain.hip)
    for (int i = 0; i < 2; ++i) {
      unsigned short* img = nullptr;
      DCF_HIP(hipMalloc(&img, head_chain_image_halfs(C) * sizeof(unsigned short)));
      m->owned.push_back(reinterpret_cast<float*>(img));
      if (launch_split_chain3(h.conv[i], img, C, st, nullptr)) return -1;   // (range: the same weights passed split_weight above)
      h.chain[i] = img;
    }
    unsigned short* img = nullptr;                       // the output convolution runs in f16x3 too: same weight range, same fallback
    DCF_HIP(hipMalloc(&img, head_chain_out_image_halfs(C) * sizeof(unsigned short)));
    m->owned.push_back(reinterpret_cast<float*>(img));
    if (launch_split_chain_out(h.out_w, NO, img, C, st, m->status ? m->status + 1 : nullptr)) return -1;
    h.out_chain = img;
  }
  return 0;
}

// model.py:411-414 / :543-551: what vid_map (PtTransformer: vid_net.embd_fc) sees.  sfonly only exists in the iterative
// model and only on the msf branch (`elif`, model.py:546); its input is then the sidekick features alone.
static inline bool vidmap_sfonly(const dcf_config& c) { return c.model_kind == 0 && c.msf && c.sfonly; }
static inline int vidmap_in_dim(const dcf_config& c) {
  return ((c.msf && !vidmap_sfonly(c)) ? 2 * c.D : c.D) + (c.scat ? 1 : 0);
}

static int finalize(dcf_model* m, hipStream_t st) {
  const dcf_config& c = m->cfg;
  const int E = c.E, D = c.D, TE = c.TE, L = c.n_levels;
  const bool sfonly = vidmap_sfonly(c);
  const int Din = vidmap_in_dim(c);
  free_packed(m);
  if (init_gemm_mode(m, st)) return -1;
  m->dec.clear(); m->stem.clear(); m->branch.clear();
  m->embd_conv.clear(); m->embd_ln_w.clear(); m->embd_ln_b.clear();
  m->cls1 = HeadW(); m->cls2 = HeadW(); m->reg = HeadW();
  m->tcn_wd.clear(); m->tcn_bd.clear(); m->tcn_wp.clear(); m->tcn_bp.clear(); m->tcn_lnw.clear(); m->tcn_lnb.clear();
  const float* t;

  m->text_enc.clear();
  m->text_embd_w = m->text_embd_b = m->text_bkgd = nullptr;
  m->text_pool = TextEncW();
  if (c.text_kind == 1) {
    // TextIdentity (text_net.py:22-89): optional 1x1 embedding, optional AttNPool1D token (use_bkgd_token)
    DCF_CHECK(c.text_in > 0 && c.text_heads >= 1 && TE % c.text_heads == 0, "text_net (identity): in_dim=%d heads=%d do not fit TE=%d", c.text_in, c.text_heads, TE);
    if (m->bound.count("text_net.embd_fc.conv.weight")) {
      GET("text_net.embd_fc.conv.weight", SH(TE, c.text_in), m->text_embd_w); GET("text_net.embd_fc.conv.bias", SH(TE), m->text_embd_b);
    } else {
      DCF_CHECK(c.text_in == TE, "text_net (identity) without embd_fc needs in_dim == embd_dim (%d vs %d)", c.text_in, TE);
    }
    if (c.text_bkgd) {
      TextEncW& w = m->text_pool;
      const std::string p = "text_net.attn_pool.attn";
      GET(p + ".query.weight", SH(TE, TE), w.wq); GET(p + ".query.bias", SH(TE), w.bq);
      GET(p + ".key.weight", SH(TE, TE), w.wk); GET(p + ".key.bias", SH(TE), w.bk);
      GET(p + ".value.weight", SH(TE, TE), w.wv); GET(p + ".value.bias", SH(TE), w.bv);
      GET(p + ".proj.weight", SH(TE, TE), w.wp); GET(p + ".proj.bias", SH(TE), w.bp);
      SPLIT(w.wq, TE, TE); SPLIT(w.wk, TE, TE); SPLIT(w.wv, TE, TE); SPLIT(w.wp, TE, TE);
    }
  } else
  if (c.text_layers > 0 || c.text_in > 0) {
    DCF_CHECK(c.text_in > 0 && c.text_layers >= 0 && c.text_heads >= 1 && TE % c.text_heads == 0,
              "text_net: in_dim=%d layers=%d heads=%d do not fit TE=%d", c.text_in, c.text_layers, c.text_heads, TE);
    GET("text_net.embd_fc.conv.weight", SH(TE, c.text_in), m->text_embd_w); GET("text_net.embd_fc.conv.bias", SH(TE), m->text_embd_b);
    if (c.text_bkgd) GET("text_net.bkgd_token", SH(TE), m->text_bkgd);
    for (int i = 0; i < c.text_layers; ++i) {
      const std::string p = "text_net.transformer." + std::to_string(i);
      TextEncW w{};
      GET(p + ".ln_attn.weight", SH(TE), w.ln_attn_w); GET(p + ".ln_attn.bias", SH(TE), w.ln_attn_b);
      GET(p + ".attn.attn.query.weight", SH(TE, TE), w.wq); GET(p + ".attn.attn.query.bias", SH(TE), w.bq);
      GET(p + ".attn.attn.key.weight", SH(TE, TE), w.wk); GET(p + ".attn.attn.key.bias", SH(TE), w.bk);
      GET(p + ".attn.attn.value.weight", SH(TE, TE), w.wv); GET(p + ".attn.attn.value.bias", SH(TE), w.bv);
      GET(p + ".attn.attn.proj.weight", SH(TE, TE), w.wp); GET(p + ".attn.attn.proj.bias", SH(TE), w.bp);
      GET(p + ".drop_path_attn.scale", SH(TE), w.ls_attn);
      GET(p + ".ln_ffn.weight", SH(TE), w.ln_ffn_w); GET(p + ".ln_ffn.bias", SH(TE), w.ln_ffn_b);
      GET(p + ".ffn.fc.weight", SH(4 * TE, TE), w.fc_w); GET(p + ".ffn.fc.bias", SH(4 * TE), w.fc_b);
      GET(p + ".ffn.proj.weight", SH(TE, 4 * TE), w.pj_w); GET(p + ".ffn.proj.bias", SH(TE), w.pj_b);
      GET(p + ".drop_path_ffn.scale", SH(TE), w.ls_ffn);
      SPLIT(w.wq, TE, TE); SPLIT(w.wk, TE, TE); SPLIT(w.wv, TE, TE); SPLIT(w.wp, TE, TE);
      SPLIT(w.fc_w, 4 * TE, TE); SPLIT(w.pj_w, TE, 4 * TE);
      m->text_enc.push_back(w);
    }
  }

  if (c.model_kind == 1) {   // PtTransformer: vid_net.embd_fc takes the (2)D-wide gated input itself (model.py:43-48)
    GET("vid_net.embd_fc.conv.weight", SH(E, Din), m->vid_map_w); GET("vid_net.embd_fc.conv.bias", SH(E), m->vid_map_b);
  } else {
    GET("vid_map.conv.weight", SH(E, Din), m->vid_map_w); GET("vid_map.conv.bias", SH(E), m->vid_map_b);
  }
  // the deep / shallow column halves of the (E, [2]D[+1]) weight are separate GEMM operands with row pitch Din
  m->vid_w1 = (c.msf && sfonly) ? nullptr : m->vid_map_w;
  m->vid_w2 = c.msf ? (sfonly ? m->vid_map_w : m->vid_map_w + D) : nullptr;
  m->vid_w3 = nullptr;
  m->vid_ldw = Din;
  if (c.scat) {
    // the extra score column makes the row pitch odd: keep aligned copies of the column blocks (pitch D) and of the column
    float* blk[3] = {nullptr, nullptr, nullptr};
    const float* src[3] = {m->vid_w1, m->vid_w2, m->vid_map_w + (Din - 1)};
    const int wid[3] = {D, D, 1};
    for (int i = 0; i < 3; ++i) {
      if (!src[i]) continue;
      DCF_HIP(hipMalloc(&blk[i], (size_t)E * wid[i] * sizeof(float)));
      m->owned.push_back(blk[i]);
      DCF_HIP(hipMemcpy2DAsync(blk[i], (size_t)wid[i] * 4, src[i], (size_t)Din * 4, (size_t)wid[i] * 4, E, hipMemcpyDeviceToDevice, st));
    }
    m->vid_w1 = blk[0]; m->vid_w2 = blk[1]; m->vid_w3 = blk[2];
    m->vid_ldw = D;
  }
  // these two GEMMs read the raw feature files, whose range the model does not control; everything downstream is
  // bounded by LayerNorms.  In f16x3 mode they run without the activation pre-scale (|x| < 65504 instead of 4094; an
  // absolute representation floor of 2^-25 on the features).
  if (D % 32 == 0 && E % 32 == 0) {
    if (m->vid_w1 && split_weight(m, m->vid_w1, E, D, st, m->vid_ldw)) return -1;
    if (m->vid_w2 && split_weight(m, m->vid_w2, E, D, st, m->vid_ldw)) return -1;
  }
  for (int i = 0; i < c.fusion_layers; ++i) {
    DecW w{};
    if (resolve_decoder(m, "fusion.layers." + std::to_string(i), E, TE, st, w)) return -1;
    m->dec.push_back(w);
  }
  GET("fusion.ln_out.weight", SH(E), m->fus_out_w); GET("fusion.ln_out.bias", SH(E), m->fus_out_b);
  if (c.model_kind != 1) {
    GET("vid_net.embd_fc.conv.weight", SH(E, E), m->embd_fc_w); GET("vid_net.embd_fc.conv.bias", SH(E), m->embd_fc_b);
    SPLIT(m->embd_fc_w, E, E);
    m->embd_fc_wf = m->embd_fc_s = m->embd_fc_c = nullptr;
    if (m->gemm_terms != 0 && E % 64 == 0 && c.fusion_layers > 0 &&
        fold_ln(m, m->embd_fc_w, m->embd_fc_b, m->fus_out_w, m->fus_out_b, E, E, st, &m->embd_fc_wf, &m->embd_fc_s, &m->embd_fc_c)) return -1;
  }
  for (int i = 0, sv = vid_stride_of(c); i < c.n_embd_convs; ++i, sv = std::max(sv / 2, 1)) {
    const std::string s = std::to_string(i);
    const int taps = sv > 1 ? 5 : 3;                 // vid_net.stride > 1: k5 / stride 2 / padding 2 (video_net.py:62-70)
    GET("vid_net.embd_convs." + s + ".conv.weight", SH(E, E, taps), t);
    const float* pk;
    if (pack3(m, t, E, E, taps, 0, 2, 1, st, &pk)) return -1;
    SPLIT(pk, E, taps * E);
    m->embd_conv.push_back(pk);
    const float *lw, *lb;
    GET("vid_net.embd_norms." + s + ".weight", SH(E), lw); GET("vid_net.embd_norms." + s + ".bias", SH(E), lb);
    m->embd_ln_w.push_back(lw); m->embd_ln_b.push_back(lb);
  }
  // the embedding stage as one kernel: the folded first convolution for both kinds of input rows, the second as it is
  m->embd_chain_w1[0] = m->embd_chain_w1[1] = m->embd_chain_w2 = nullptr;
  m->embd_chain_cb[0] = m->embd_chain_cb[1] = nullptr;
  unsigned* embd_overflow = nullptr;
  if (m->gemm_terms == GEMM_F16X3 && c.model_kind != 1 && vid_stride_of(c) == 1 && c.n_embd_convs == 2 && embd_chain_supports(E)) {
    const size_t img = head_chain_image_halfs(E) * sizeof(unsigned short), wf = (size_t)E * 3 * E * sizeof(float);
    char* buf = nullptr;                               // 3 images, 2 bias sets, the overflow word; the fp32 / fp64 intermediates
    DCF_HIP(hipMalloc(&buf, 3 * img + 2 * 3 * E * sizeof(float) + 256 + wf + E * sizeof(double)));
    m->owned.push_back(reinterpret_cast<float*>(buf));
    unsigned short* imgs[3] = {reinterpret_cast<unsigned short*>(buf), reinterpret_cast<unsigned short*>(buf + img), reinterpret_cast<unsigned short*>(buf + 2 * img)};
    float* cb = reinterpret_cast<float*>(buf + 3 * img);
    embd_overflow = reinterpret_cast<unsigned*>(cb + 2 * 3 * E);
    float* Wf = reinterpret_cast<float*>(buf + 3 * img + 2 * 3 * E * sizeof(float) + 256);
    double* d = reinterpret_cast<double*>(reinterpret_cast<char*>(Wf) + wf);
    DCF_HIP(hipMemsetAsync(embd_overflow, 0, sizeof(unsigned), st));
    for (int v = 0; v < 2; ++v) {                      // (stream order: Wf and d are reused)
      const float *g = v == 0 ? m->fus_out_w : nullptr, *beta = v == 0 ? m->fus_out_b : nullptr;
      hipLaunchKernelGGL(k_fold_embd_d, dim3((E + 255) / 256), dim3(256), 0, st, m->embd_fc_w, m->embd_fc_b, beta, d, E);
      hipLaunchKernelGGL(k_fold_embd, dim3(3 * E), dim3(E), 0, st, m->embd_conv[0], m->embd_fc_w, g, (const double*)d, Wf, cb + v * 3 * E, E);
      DCF_HIP(hipGetLastError());
      // its own range word: a folded weight beyond the scaled fp16 range keeps the launch path, the model's arithmetic mode stays
      if (launch_split_chain3(Wf, imgs[v], E, st, embd_overflow)) return -1;
      m->embd_chain_w1[v] = imgs[v]; m->embd_chain_cb[v] = cb + v * 3 * E;
    }
    if (launch_split_chain3(m->embd_conv[1], imgs[2], E, st, nullptr)) return -1;      // (range: the same weights passed split_weight above)
    m->embd_chain_w2 = imgs[2];
  }
  for (int i = 0; i < c.n_stem; ++i) {
    EncW w{};
    if (resolve_encoder(m, "vid_net.stem." + std::to_string(i), E, st, w)) return -1;
    m->stem.push_back(w);
  }
  m->pool_w.clear();
  for (int i = 0; i < L; ++i) {
    if (c.pool_only) {
      const float* pk;
      GET("vid_net.branch." + std::to_string(i) + ".conv.weight", SH(E, 3), t);
      if (pack3(m, t, 1, E, 3, 0, 2, 1, st, &pk)) return -1;
      m->pool_w.push_back(pk);
      continue;
    }
    EncW w{};
    if (resolve_encoder(m, "vid_net.branch." + std::to_string(i), E, st, w)) return -1;
    m->branch.push_back(w);
  }
  if (resolve_head(m, "cls_head", "cls_head", E, 1, c.head_layers, st, m->cls1)) return -1;
  const int EH = c.model_kind == 0 ? E + TCN_HID : E;      // only the iterative model concatenates the refined logits (model.py:426-428)
  if (c.model_kind == 0 && resolve_head(m, "cls_head2", "cls_head", EH, 1, c.head_layers, st, m->cls2)) return -1;
  if (resolve_head(m, "reg_head", "reg_head", EH, 2, c.head_layers, st, m->reg)) return -1;
  m->reg_scales.assign(L, 1.f);
  for (int l = 0; l < L; ++l) {
    GET("reg_head.scales." + std::to_string(l) + ".scale", SH(1), t);
    DCF_HIP(hipMemcpyAsync(&m->reg_scales[l], t, sizeof(float), hipMemcpyDeviceToHost, st));
  }
  if (c.model_kind == 0 && resolve_tcn(m, "refine", L, L, st)) return -1;
  DCF_HIP(hipStreamSynchronize(st));
  if (embd_overflow) {
    unsigned over = 0u;
    DCF_HIP(hipMemcpy(&over, embd_overflow, sizeof(over), hipMemcpyDeviceToHost));
    if (over) m->embd_chain_w1[0] = m->embd_chain_w1[1] = m->embd_chain_w2 = nullptr;
  }
  for (auto& pl : m->plans) if (pl.d_lt) (void)hipFree(pl.d_lt);
  m->plans.clear();
  free_hybrid(m);                             // reg scales live in the level tables
  drop_graph(m);
  if (m->gemm_terms == GEMM_F16X3) {
    // did every weight fit the scaled fp16 range (|w| < 255.9)?  If not, rebuild the images for bf16x6.
    unsigned flags[2] = {0u, 0u};
    DCF_HIP(hipMemcpyAsync(flags, m->status, sizeof(flags), hipMemcpyDeviceToHost, st));
    DCF_HIP(hipStreamSynchronize(st));
    if (flags[1]) {
      m->force_x6 = true;
      return finalize(m, st);
    }
  }
  m->finalized = true;
  return 0;
}

}  // namespace dcf

extern "C" {

int dcf_model_create(const dcf_config* cfg, dcf_model** out) {
  DCF_CHECK(cfg && out, "dcf_model_create: null argument");
  DCF_CHECK(cfg->E > 0 && cfg->E % 32 == 0 && cfg->E <= 992, "E=%d must be a positive multiple of 32 (<= 992)", cfg->E);
  DCF_CHECK(cfg->attn_mode == 0 || cfg->attn_mode == 1, "attn_mode=%d: 0 (f16x3) or 1 (one fp16 product)", cfg->attn_mode);
  DCF_CHECK(cfg->D > 0 && cfg->D % 32 == 0, "D=%d must be a positive multiple of 32", cfg->D);
  DCF_CHECK(cfg->TE > 0 && cfg->TE % 32 == 0, "TE=%d must be a positive multiple of 32", cfg->TE);
  DCF_CHECK(cfg->n_levels >= 1 && cfg->n_levels <= dcf::DCF_MAX_LEVELS, "n_levels=%d out of range", cfg->n_levels);
  DCF_CHECK(cfg->win == 0 || (cfg->win > 0 && (cfg->win & 1)), "mha_win_size=%d must be odd, or 0 for global self-attention over the clips", cfg->win);
  DCF_CHECK(cfg->fusion_layers >= 0 && cfg->head_layers >= 0 && cfg->n_embd_convs >= 0 && cfg->n_stem >= 0, "negative layer count");
  DCF_CHECK(cfg->sn >= 1, "sn must be >= 1");
  DCF_CHECK(cfg->model_kind >= 0 && cfg->model_kind <= 2, "model_kind must be 0 (iterative early fusion), 1 (late fusion) or 2 (early fusion)");
  {
    const int sv = cfg->vid_stride > 1 ? cfg->vid_stride : 1;
    int lg = 0;
    while ((1 << lg) < sv) ++lg;
    DCF_CHECK((sv & (sv - 1)) == 0 && cfg->n_embd_convs >= lg, "vid_net.stride=%d must be a power of two with arch[0]=%d >= log2(stride) (video_net.py:52-53)",
              sv, cfg->n_embd_convs);
  }
  int ndev = 0;
  DCF_HIP(hipGetDeviceCount(&ndev));
  DCF_CHECK(ndev > 0, "no HIP device");
  dcf_model* m = new dcf_model();
  m->cfg = *cfg;
  *out = m;
  return 0;
}

void dcf_model_destroy(dcf_model* m) {
  if (!m) return;
  dcf::free_model(m);
  delete m;
}

int dcf_model_bind(dcf_model* m, const char* name, const float* data, const int64_t* shape, int32_t ndim) {
  DCF_CHECK(m && name && data, "dcf_model_bind: null argument");
  dcf::Bound b;
  b.p = data;
  for (int i = 0; i < ndim; ++i) b.shape.push_back(shape[i]);
  m->bound[name] = b;
  m->finalized = false;
  return 0;
}

int dcf_model_set_pe(dcf_model* m, const float* pe_tokens, int64_t T) {
  DCF_CHECK(m, "dcf_model_set_pe: null model");
  m->pe = pe_tokens;
  m->pe_T = T;
  return 0;
}

int dcf_model_set_text_pe(dcf_model* m, const float* pe_tokens, int64_t L) {
  DCF_CHECK(m, "dcf_model_set_text_pe: null model");
  m->text_pe = pe_tokens;
  m->text_pe_L = L;
  return 0;
}

int dcf_model_finalize(dcf_model* m, void* stream) {
  DCF_CHECK(m, "dcf_model_finalize: null model");
  return dcf::finalize(m, (hipStream_t)stream);
}

int dcf_numerics_status(dcf_model* m, int32_t reset, void* stream) {
  DCF_CHECK(m, "dcf_numerics_status: null model");
  int out = m->gemm_terms == dcf::GEMM_BF16X6 ? 4 : (m->gemm_terms == 0 ? 8 : 0);
  if (m->force_x6) out |= 2;
  if (m->status) {
    unsigned flag = 0u;
    hipStream_t st = (hipStream_t)stream;
    DCF_HIP(hipMemcpyAsync(&flag, m->status, sizeof(flag), hipMemcpyDeviceToHost, st));
    if (reset) DCF_HIP(hipMemsetAsync(m->status, 0, sizeof(unsigned), st));
    DCF_HIP(hipStreamSynchronize(st));
    if (flag & ~2u) out |= 1;
    if (flag & 2u) out |= 16;                  // one-pass LayerNorm statistics met an ill-conditioned row (common.h LN_ILL_RATIO)
  }
  return out;
}

int dcf_model_set_ln_carry(dcf_model* m, int32_t on) {
  DCF_CHECK(m, "dcf_model_set_ln_carry: null model");
  const bool off = on == 0;
  if (off != m->no_ln_carry) dcf::drop_graph(m);
  m->no_ln_carry = off;
  return 0;
}

int dcf_numerics_status_async(dcf_model* m, int32_t* host_dst, void* stream) {
  DCF_CHECK(m && host_dst, "dcf_numerics_status_async: null argument");
  if (!m->status) { *host_dst = 0; return 0; }
  DCF_HIP(hipMemcpyAsync(host_dst, m->status, sizeof(unsigned), hipMemcpyDeviceToHost, (hipStream_t)stream));
  return 0;
}

int dcf_model_set_dropout(dcf_model* m, float vid_proj_p, float vid_path_p, float fus_proj_p, float fus_path_p, float refine_p,
                          int64_t seed) {
  DCF_CHECK(m, "dcf_model_set_dropout: null model");
  const float p[5] = {vid_proj_p, vid_path_p, fus_proj_p, fus_path_p, refine_p};
  for (int i = 0; i < 5; ++i) DCF_CHECK(p[i] >= 0.f && p[i] < 1.f, "dcf_model_set_dropout: rate %d = %g outside [0, 1)", i, (double)p[i]);
  auto& d = m->drop_state;
  d.active = false;
  for (int i = 0; i < 5; ++i) {
    d.p[i] = p[i];
    d.scale[i] = 1.0f / (1.0f - p[i]);
    d.active = d.active || p[i] > 0.f;
  }
  d.seed = (uint64_t)seed;
  return 0;
}

int dcf_debug_set_option(const char* name, int32_t value) {
  DCF_CHECK(name && *name, "dcf_debug_set_option: empty name");
  static const char* known[] = {"dec_chain_min_rows", "enc_chain_min_rows", "enc_attn_min_rows", "fuse_scores", "tcn_frag", "gate_skip", "tcn_stack", "half_native", "embd_chain", "embd_chain_min_rows", "gemm_uniform"};
  bool ok = false;
  for (const char* k : known) ok = ok || strcmp(k, name) == 0;
  DCF_CHECK(ok, "dcf_debug_set_option: unknown option '%s'", name);
  {
    std::lock_guard<std::mutex> lock(dcf::debug_options_mutex());
    if (value < 0) dcf::debug_options().erase(name);           // back to the built-in value
    else dcf::debug_options()[name] = value;
  }
  dcf::g_option_epoch.fetch_add(1);                         // every model drops its captured graphs at its next forward
  return 0;
}

int dcf_model_set_graph_mode(dcf_model* m, int32_t mode) {
  DCF_CHECK(m && mode >= 0 && mode <= 2, "dcf_model_set_graph_mode: mode must be 0 (auto), 1 (always) or 2 (never)");
  if (mode != m->graph_mode) dcf::drop_graph(m);
  m->graph_mode = mode;
  return 0;
}

int dcf_debug_copy(dcf_model* m, int32_t what, float* dst, int64_t max_floats, void* stream) {
  DCF_CHECK(m && dst, "dcf_debug_copy: null argument");
  hipStream_t st = (hipStream_t)stream;
  const float* src = nullptr;
  int64_t n = 0;
  const int E = m->cfg.E;
  switch (what) {
    case 0: src = m->dbg.correl; n = (int64_t)m->dbg.nq * m->dbg.T0; break;
    case 1: src = m->dbg.gate; n = (int64_t)m->dbg.B * m->dbg.T0; break;
    case 4: src = m->dbg.F; n = (int64_t)m->dbg.B * m->dbg.S * (E + dcf::TCN_HID); break;
    case 2: case 3: {
      // these buffers are overwritten during the forward: arm the tap, the NEXT forward fills dst (rows0 * E floats of its
      // last query chunk) and disarms it again
      m->keep_debug = true;
      m->dbg_cap = max_floats;
      if (what == 2) m->dbg_vidmap = dst; else m->dbg_fused = dst;
      return 0;
    }
    default: DCF_CHECK(false, "dcf_debug_copy: unknown selector %d", what);
  }
  DCF_CHECK(src, "dcf_debug_copy: no forward has run yet");
  DCF_CHECK(n <= max_floats, "dcf_debug_copy: destination too small (%lld > %lld)", (long long)n, (long long)max_floats);
  DCF_HIP(hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, st));
  return 0;
}

// ---- profiling ---------------------------------------------------------------------------------
int dcf_profile_enable(int32_t on) {
  for (auto& r : dcf::g_recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
  dcf::g_recs.clear();
  dcf::g_prof_on = on != 0;
  return 0;
}

int64_t dcf_profile_report(char* buf, int64_t cap) {
  struct Agg { long count = 0; double ms = 0, flops = 0, bytes = 0; };
  std::vector<std::pair<std::string, Agg>> aggs;
  for (auto& r : dcf::g_recs) {
    if (hipEventSynchronize(r.b) != hipSuccess) continue;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) continue;
    Agg* a = nullptr;
    for (auto& kv : aggs) if (kv.first == r.name) a = &kv.second;
    if (!a) { aggs.emplace_back(r.name, Agg()); a = &aggs.back().second; }
    a->count++; a->ms += ms; a->flops += r.flops; a->bytes += r.bytes;
  }
  std::string out = "{";
  for (size_t i = 0; i < aggs.size(); ++i) {
    char line[512];
    snprintf(line, sizeof(line), "%s\"%s\": {\"count\": %ld, \"ms\": %.6f, \"flops\": %.6e, \"bytes\": %.6e}", i ? ", " : "",
             aggs[i].first.c_str(), aggs[i].second.count, aggs[i].second.ms, aggs[i].second.flops, aggs[i].second.bytes);
    out += line;
  }
  out += "}";
  if (buf && cap > 0) {
    size_t n = std::min((size_t)cap - 1, out.size());
    memcpy(buf, out.data(), n);
    buf[n] = 0;
  }
  return (int64_t)out.size() + 1;
}

}  // extern "C"
