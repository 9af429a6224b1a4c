// Attention-map dropout inside the attention cores, forward and backward -- the sliding-window core first, global self attention and
// cross attention in the section "dense attention" further down -- and channel dropout (include/decafnet_hip_attn_drop.h).  The map
// never exists in memory: the attention kernels hold it in registers, so the keep bits are drawn where the map element is formed.
//
// The sliding-window kernels are k_local_attn, k_attn_bwd_q and k_attn_bwd_kv of local_attn_kernels.h, instantiated here on
// LocalAttnDropArgs: one source with the dropout-free kernels of attn.hip and attn_grad.hip, the keep factor switched in at compile
// time.  That header has the arithmetic and the layout of the keep bits.
//
// p = 0 runs the dropout-free instantiations themselves (launch_local_attn, launch_local_attn_bwd; the dense forms call their
// exports): the bits of the dropout-free exports by construction.  A factor of 1.0f changes no bit either, but a second copy of an
// expression like D * corr + e * dP is contracted into an FMA per instantiation, and the compiler took the other product in one
// variant (the loop form of the query side: dQ off by an ulp at p = 0); equal bits must not rest on that.  The instantiations below
// therefore run with p > 0 only.
#include "attn_drop.h"

#include "attn.h"
#include "attn_grad.h"
#include "xattn_grad.h"
#include "../../include/decafnet_hip_attn.h"
#include "../../include/decafnet_hip_attn_drop.h"
#include "dropout.h"
#include "grad_common.h"
#include "local_attn_kernels.h"

namespace dcf {

// ------------------------------------------------------------------------------------------
// dense attention with dropout on its map: global self attention (keys = the T rows of the query's sequence) and cross attention
// (keys = the Lk rows of sequence b of K / V).  Every valid key of the sequence is visited, a masked key is excluded exactly (-inf).
// Plain kernels on the layout above (a wave per query row resp. per key row, a lane owns 4 channels, a head is LPH lanes): the
// dropout-free cores (k_global_attn, k_xattn_mfma and their backwards) are tuned per shape and are not copied; these serve p > 0.
// Keep bits: the Lk elements of a (row, head) in blocks of 32 through row_keep_bits; the query side of the backward leaves the words
// in scratch [rows][heads][ceil(Lk / 32)] for the key side.
// ------------------------------------------------------------------------------------------
struct DenseAttnDropArgs {
  const float* Q; const float* K; const float* V;   // [B*T][C], [B*Lk][C], [B*Lk][C]
  const uint8_t* kmask;                              // [B*Lk] or nullptr = every key valid
  float* O; const float* dO;
  float* dQ; float* dK; float* dV;
  float* stats;                                      // [B*T][heads][4]: m, 1 / l (0 without a valid key), delta, unused
  uint32_t* bits;                                    // [B*T][heads][nw]
  int B, T, Lk, C, heads, b0, nw;
  uint64_t seed; uint32_t site; float p, scale;
};

template <int NCH, int LPH>
__device__ __forceinline__ void dense_row_e0(const DenseAttnDropArgs& p, int64_t r, int lane, uint64_t* e0) {
  const int64_t bg = p.b0 + r / p.T;
  const int t = (int)(r % p.T);
#pragma unroll
  for (int j = 0; j < NCH; ++j) e0[j] = (uint64_t)(((bg * p.heads + (64 * j + lane) / LPH) * (int64_t)p.T + t) * (int64_t)p.Lk);
}

template <int NCH, int LPH, bool BWD>
__global__ __launch_bounds__(256) void k_dense_attn_drop_q(DenseAttnDropArgs p) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (r >= (int64_t)p.B * p.T) return;
  const int C = p.C;
  const int64_t kbase = (r / p.T) * p.Lk;
  const float scale = 1.0f / sqrtf(sqrtf((float)(C / p.heads)));
  uint64_t e0[NCH];
  dense_row_e0<NCH, LPH>(p, r, lane, e0);
  Row<NCH> q, g, k, v;
  q.load(p.Q + r * C, C, lane);
  scale_row(q, scale);
  if constexpr (BWD) g.load(p.dO + r * C, C, lane);
  f32x4 acc[NCH];
  float m[NCH], l[NCH], D[NCH];
#pragma unroll
  for (int j = 0; j < NCH; ++j) { acc[j] = zero4(); m[j] = -INFINITY; l[j] = 0.f; D[j] = 0.f; }
  if constexpr (BWD) {
    // The row maximum first, so that the sums below are formed of the very weights exp(s - m) that the second pass and the key side
    // form again: sum_j dS_tj = delta (1 - sum_j P_tj) then vanishes to the rounding of the sums alone.  (Carried online, each weight
    // differs from exp(s - m) by the roundings of the rescaling, and that difference times delta is what is left of a gradient that is
    // zero by symmetry -- key.bias, k_norm.bias -- : 1.2 of the rule's bound in the whole-step fixture with mha_win_size = 0.)
    for (int jk = 0; jk < p.Lk; ++jk) {
      if (p.kmask && p.kmask[kbase + jk] == 0) continue;
      k.load(p.K + (kbase + jk) * C, C, lane);
#pragma unroll
      for (int j = 0; j < NCH; ++j) m[j] = fmaxf(m[j], head_sum<LPH>(dotp(q.v[j], k.v[j] * scale)));
    }
  }
  for (int j0 = 0; j0 < p.Lk; j0 += 32) {
    const int nb = min(32, p.Lk - j0);
    uint32_t bits[NCH];
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      bits[j] = row_keep_bits<LPH>(p.seed, p.site, p.p, e0[j] + (uint64_t)j0, nb, lane);
      if (BWD && p.bits && lane % LPH == 0 && 256 * j + 4 * lane < C) p.bits[(r * p.heads + (64 * j + lane) / LPH) * p.nw + (j0 >> 5)] = bits[j];
    }
    for (int jj = 0; jj < nb; ++jj) {
      if (p.kmask && p.kmask[kbase + j0 + jj] == 0) continue;
      k.load(p.K + (kbase + j0 + jj) * C, C, lane);
      v.load(p.V + (kbase + j0 + jj) * C, C, lane);
#pragma unroll
      for (int j = 0; j < NCH; ++j) {
        const float s = head_sum<LPH>(dotp(q.v[j], k.v[j] * scale));
        if constexpr (BWD) {
          const float e = exp_res(s - m[j]);
          const float ek = ((bits[j] >> jj) & 1u) ? e * p.scale : 0.f;
          l[j] += e;
          D[j] += ek * head_sum<LPH>(dotp(g.v[j], v.v[j]));
        } else {
          const float mn = fmaxf(m[j], s);
          const float corr = m[j] == -INFINITY ? 0.f : exp_res(m[j] - mn);
          const float e = exp_res(s - mn);
          const float ek = ((bits[j] >> jj) & 1u) ? e * p.scale : 0.f;
          l[j] = l[j] * corr + e;
          acc[j] = acc[j] * corr + ek * v.v[j];
          m[j] = mn;
        }
      }
    }
  }
  if constexpr (!BWD) {
    Row<NCH> o;
#pragma unroll
    for (int j = 0; j < NCH; ++j) o.v[j] = l[j] > 0.f ? acc[j] / l[j] + 0.0f : zero4();     // no valid key: zeros; a zero leaves as +0
    o.store(p.O + r * C, C, lane);
    return;
  }
  float il[NCH], delta[NCH];
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    il[j] = l[j] > 0.f ? 1.0f / l[j] : 0.f;
    delta[j] = D[j] * il[j];
    if (p.stats && lane % LPH == 0 && 256 * j + 4 * lane < C)
      *reinterpret_cast<f32x4*>(p.stats + (r * p.heads + (64 * j + lane) / LPH) * 4) = f32x4{m[j], il[j], delta[j], 0.f};
  }
  if (!p.dQ) return;
  Row<NCH> dq;
  dq.zero();
  for (int j0 = 0; j0 < p.Lk; j0 += 32) {
    const int nb = min(32, p.Lk - j0);
    uint32_t bits[NCH];
#pragma unroll
    for (int j = 0; j < NCH; ++j) bits[j] = row_keep_bits<LPH>(p.seed, p.site, p.p, e0[j] + (uint64_t)j0, nb, lane);
    for (int jj = 0; jj < nb; ++jj) {
      if (p.kmask && p.kmask[kbase + j0 + jj] == 0) continue;
      k.load(p.K + (kbase + j0 + jj) * C, C, lane);
      v.load(p.V + (kbase + j0 + jj) * C, C, lane);
#pragma unroll
      for (int j = 0; j < NCH; ++j) {
        const float s = head_sum<LPH>(dotp(q.v[j], k.v[j] * scale));
        const float dp = head_sum<LPH>(dotp(g.v[j], v.v[j]));
        const float pj = exp_res(s - m[j]) * il[j];
        const float dpk = ((bits[j] >> jj) & 1u) ? dp * p.scale : 0.f;
        dq.v[j] += (pj * (dpk - delta[j])) * (k.v[j] * scale);
      }
    }
  }
  scale_row(dq, scale);
  dq.store(p.dQ + r * C, C, lane);
}

// key side: a wave per key row, a gather over the T queries of its sequence in ascending order
template <int NCH, int LPH>
__global__ __launch_bounds__(256) void k_dense_attn_drop_kv(DenseAttnDropArgs p) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (r >= (int64_t)p.B * p.Lk) return;
  const int C = p.C;
  const int jk = (int)(r % p.Lk);
  const int64_t qbase = (r / p.Lk) * p.T;
  const float scale = 1.0f / sqrtf(sqrtf((float)(C / p.heads)));
  Row<NCH> k, v, dk, dv, q, g;
  dk.zero();
  dv.zero();
  if (!p.kmask || p.kmask[r] != 0) {                     // a masked key: exactly 0, whatever dO holds
    k.load(p.K + r * C, C, lane);
    v.load(p.V + r * C, C, lane);
    scale_row(k, scale);
    const bool want_dk = p.dK != nullptr;
    for (int t = 0; t < p.T; ++t) {
      q.load(p.Q + (qbase + t) * C, C, lane);
      g.load(p.dO + (qbase + t) * C, C, lane);
#pragma unroll
      for (int j = 0; j < NCH; ++j) {
        const bool act = 256 * j + 4 * lane < C;           // (a head's lanes are all inside C or all outside)
        const int64_t rh = (qbase + t) * p.heads + (64 * j + lane) / LPH;
        const f32x4 st = act ? *reinterpret_cast<const f32x4*>(p.stats + rh * 4) : zero4();
        const bool kept = act && ((p.bits[rh * p.nw + (jk >> 5)] >> (jk & 31)) & 1u) != 0;
        const f32x4 qs = q.v[j] * scale;
        const float s = head_sum<LPH>(dotp(qs, k.v[j]));
        const float pj = exp_res(s - st.x) * st.y;
        const float pk = kept ? pj * p.scale : 0.f;
        dv.v[j] += pk * g.v[j];
        if (want_dk) {
          const float dp = head_sum<LPH>(dotp(g.v[j], v.v[j]));
          const float dpk = kept ? dp * p.scale : 0.f;
          dk.v[j] += (pj * (dpk - st.z)) * qs;
        }
      }
    }
  }
  if (p.dK) {
    scale_row(dk, scale);
    dk.store(p.dK + r * C, C, lane);
  }
  if (p.dV) dv.store(p.dV + r * C, C, lane);
}

// ------------------------------------------------------------------------------------------
// channel dropout: one decision per (sample, channel) of a (B', Cin, T) tensor, e = (b0 + b) Cin + c
// ------------------------------------------------------------------------------------------
constexpr int CD_ROWS = 16;            // rows of one sequence a thread walks with the keep bits of its four channels

__global__ __launch_bounds__(256) void k_channel_dropout(const float* __restrict__ X, float* __restrict__ Y, int B, int T, int C, int b0,
                                                         uint64_t seed, uint32_t site, float p, float scale) {
  const int c4n = C / 4, tcn = (T + CD_ROWS - 1) / CD_ROWS;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)B * tcn * c4n) return;
  const int c = (int)(i % c4n) * 4;
  const int tc = (int)((i / c4n) % tcn);
  const int b = (int)(i / ((int64_t)c4n * tcn));
  // C is a multiple of 4: the four channels are the four words of one counter block
  const Philox4 v = drop_block(seed, site, (uint64_t)((int64_t)(b0 + b) * C + c) >> 2);
  f32x4 kf;
  kf.x = drop_keep_word(v.x, p) ? scale : 0.f; kf.y = drop_keep_word(v.y, p) ? scale : 0.f;
  kf.z = drop_keep_word(v.z, p) ? scale : 0.f; kf.w = drop_keep_word(v.w, p) ? scale : 0.f;
  const int t1 = min(T, (tc + 1) * CD_ROWS);
  for (int t = tc * CD_ROWS; t < t1; ++t) {
    const int64_t o = ((int64_t)b * T + t) * C + c;
    const f32x4 x = ld4(X + o);
    st4(Y + o, f32x4{kf.x != 0.f ? x.x * kf.x : 0.f, kf.y != 0.f ? x.y * kf.y : 0.f, kf.z != 0.f ? x.z * kf.z : 0.f,
                    kf.w != 0.f ? x.w * kf.w : 0.f});              // a dropped element is +0, whatever X holds
  }
}

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------
static int ad_check(const char* who, const LocalAttnDropArgs& a) {
  if (local_attn_geometry_check(who, a.B, a.T, a.C, a.heads, a.window, "has its backward in dcf_op_global_attn_drop_bwd")) return -1;
  DCF_CHECK(a.b0 >= 0, "%s: b0 = %d must not be negative", who, a.b0);
  DCF_CHECK(a.p >= 0.f && a.p < 1.f, "%s: p = %g outside [0, 1)", who, (double)a.p);
  return 0;
}

template <int NCH, int LPH, int WMAX>
static void ad_launch_fwd(const LocalAttnDropArgs& a, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL((k_local_attn<NCH, LPH, false, WMAX, false, LocalAttnDropArgs>), grid, dim3(256), 0, st, a);
}
template <int NCH, int LPH, int WMAX>
static void ad_launch_bwd(const LocalAttnDropArgs& a, dim3 grid, bool kv, hipStream_t st) {
  hipLaunchKernelGGL((k_attn_bwd_q<NCH, LPH, WMAX, LocalAttnDropArgs>), grid, dim3(256), 0, st, a);
  if (kv) hipLaunchKernelGGL((k_attn_bwd_kv<NCH, LPH, WMAX, LocalAttnDropArgs>), grid, dim3(256), 0, st, a);
}
// the variants of the dropout-free launchers: the forward unrolls windows of at most 9 / 19 keys at every width, the backward at
// rows of one chunk
#define AD_FWD(NCH_, LPH_) do {                                                           \
    if (a.window <= 9) ad_launch_fwd<NCH_, LPH_, 9>(a, grid, st);                         \
    else if (a.window <= 19) ad_launch_fwd<NCH_, LPH_, 19>(a, grid, st);                  \
    else ad_launch_fwd<NCH_, LPH_, 0>(a, grid, st); } while (0)
#define AD_BWD(NCH_, LPH_) do {                                                           \
    if (NCH_ == 1 && a.window <= 9) ad_launch_bwd<1, LPH_, 9>(a, grid, kv, st);           \
    else if (NCH_ == 1 && a.window <= 19) ad_launch_bwd<1, LPH_, 19>(a, grid, kv, st);    \
    else ad_launch_bwd<NCH_, LPH_, 0>(a, grid, kv, st); } while (0)
static DenseAttnDropArgs dense_args(const float* Q, const float* K, const float* V, const uint8_t* kmask, float* O, const float* dO, float* dQ,
                                    float* dK, float* dV, int B, int T, int Lk, int C, int heads, int b0, int64_t seed, int32_t site, float p) {
  DenseAttnDropArgs a{};
  a.Q = Q; a.K = K; a.V = V; a.kmask = kmask; a.O = O; a.dO = dO; a.dQ = dQ; a.dK = dK; a.dV = dV;
  a.B = B; a.T = T; a.Lk = Lk; a.C = C; a.heads = heads; a.b0 = b0; a.nw = (Lk + 31) / 32;
  a.seed = (uint64_t)seed; a.site = (uint32_t)site; a.p = p; a.scale = 1.0f / (1.0f - p);
  return a;
}

template <int NCH, int LPH>
static void ad_dense_fwd(const DenseAttnDropArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((k_dense_attn_drop_q<NCH, LPH, false>), dim3((unsigned)(((int64_t)a.B * a.T + 3) / 4)), dim3(256), 0, st, a);
}
template <int NCH, int LPH>
static void ad_dense_bwd(const DenseAttnDropArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((k_dense_attn_drop_q<NCH, LPH, true>), dim3((unsigned)(((int64_t)a.B * a.T + 3) / 4)), dim3(256), 0, st, a);
  if (a.dK || a.dV) hipLaunchKernelGGL((k_dense_attn_drop_kv<NCH, LPH>), dim3((unsigned)(((int64_t)a.B * a.Lk + 3) / 4)), dim3(256), 0, st, a);
}
#define AD_DENSE_FWD(NCH_, LPH_) ad_dense_fwd<NCH_, LPH_>(a, st)
#define AD_DENSE_BWD(NCH_, LPH_) ad_dense_bwd<NCH_, LPH_>(a, st)

// the checks every p takes; `dims`: the head dimensions of the dropout-free export
static int dense_check(const char* who, const DenseAttnDropArgs& a, int dmin, int dmax, int lk_max) {
  DCF_CHECK(a.B > 0 && a.T > 0 && a.heads > 0, "%s: empty batch (B=%d T=%d heads=%d)", who, a.B, a.T, a.heads);
  DCF_CHECK(a.Lk >= 1 && a.Lk <= lk_max, "%s: %d keys per sequence (1 to %d)", who, a.Lk, lk_max);
  DCF_CHECK(a.C > 0 && a.C % 4 == 0 && a.C <= 1024 && a.C % a.heads == 0, "%s: C=%d must be a multiple of 4 and of heads=%d, up to 1024", who, a.C,
            a.heads);
  const int d = a.C / a.heads;
  DCF_CHECK(d >= dmin && d <= dmax && (d & (d - 1)) == 0, "%s: head dimension %d (a power of two from %d to %d, the dropout-free export's)", who, d,
            dmin, dmax);
  DCF_CHECK((int64_t)a.B * a.T < (1ll << 31) - 64 && (int64_t)a.B * a.Lk < (1ll << 31) - 64 && a.B <= 65535,
            "%s: %lld rows in %d sequences (< 2^31 rows, <= 65535 sequences)", who, (long long)a.B * a.T, a.B);
  DCF_CHECK(a.b0 >= 0, "%s: b0 = %d must not be negative", who, a.b0);
  DCF_CHECK(a.p >= 0.f && a.p < 1.f, "%s: p = %g outside [0, 1)", who, (double)a.p);
  return 0;
}

static int launch_dense_attn_drop(const char* who, const DenseAttnDropArgs& a, bool bwd, hipStream_t st) {
  const int nch = (a.C + 255) / 256, lph = a.C / a.heads / 4;
  bool ok = true;
  if (bwd) DCF_ATTN_ROW_SHAPES(nch, lph, ok, AD_DENSE_BWD);
  else DCF_ATTN_ROW_SHAPES(nch, lph, ok, AD_DENSE_FWD);
  DCF_CHECK(ok, "%s: no kernel for C=%d heads=%d", who, a.C, a.heads);
  DCF_HIP(hipGetLastError());
  return 0;
}

// the backward of either dense form at p > 0: statistics and keep words in stream-ordered scratch when dK or dV is wanted
static int dense_attn_drop_bwd(const char* who, DenseAttnDropArgs a, hipStream_t st) {
  if (!a.dQ && !a.dK && !a.dV) return 0;
  a.nw = (a.Lk + 31) / 32;
  StreamScratch sc(st);
  if (a.dK || a.dV) {
    if (sc.take(&a.stats, (size_t)a.B * a.T * a.heads * 4) || sc.take(&a.bits, (size_t)a.B * a.T * a.heads * a.nw)) return -1;
  }
  return sc.end(launch_dense_attn_drop(who, a, true, st));
}

int launch_local_attn_drop(const LocalAttnDropArgs& a, hipStream_t st) {
  const char* who = "local attention with map dropout";
  DCF_CHECK(a.Q && a.K && a.V && a.mask && a.O, "%s: null operand", who);
  if (ad_check(who, a)) return -1;
  if (a.p == 0.f) return launch_local_attn(LocalAttnArgs{a.Q, a.K, a.V, a.mask, a.O, a.B, a.T, a.C, a.heads, a.window}, st);
  const int nch = (a.C + 255) / 256, lph = a.C / a.heads / 4;
  const int qpw = a.window <= 19 ? LA_QPW : 1;
  const dim3 grid((unsigned)(((int64_t)a.B * ((a.T + qpw - 1) / qpw) + 3) / 4));
  bool ok = true;
  DCF_ATTN_ROW_SHAPES(nch, lph, ok, AD_FWD);
  DCF_CHECK(ok, "%s: no kernel for C=%d heads=%d", who, a.C, a.heads);
  DCF_HIP(hipGetLastError());
  return 0;
}

int launch_local_attn_drop_bwd(const LocalAttnDropArgs& a, hipStream_t st) {
  const char* who = "local attention backward with map dropout";
  DCF_CHECK(a.Q && a.K && a.V && a.dO, "%s: null operand", who);
  if (ad_check(who, a)) return -1;
  if (a.p == 0.f)     // (the statistics scratch has the dropout-free backward's size)
    return launch_local_attn_bwd(LocalAttnGradArgs{a.Q, a.K, a.V, a.mask, a.dO, a.dQ, a.dK, a.dV, a.stats, a.B, a.T, a.C, a.heads, a.window}, st);
  const int nch = (a.C + 255) / 256, lph = a.C / a.heads / 4;
  const bool kv = a.dK || a.dV;
  DCF_CHECK(!kv || a.stats, "%s: dK / dV need the row statistics scratch", who);
  if (!a.dQ && !kv) return 0;
  const dim3 grid((unsigned)(((int64_t)a.B * a.T + 3) / 4));       // four waves per workgroup, a wave per row
  bool ok = true;
  DCF_ATTN_ROW_SHAPES(nch, lph, ok, AD_BWD);
  DCF_CHECK(ok, "%s: no kernel for C=%d heads=%d", who, a.C, a.heads);
  DCF_HIP(hipGetLastError());
  return 0;
}

}  // namespace dcf

using namespace dcf;

extern "C" {

int dcf_attn_drop_ext_version(void) { return DCF_ATTN_DROP_EXT_VERSION; }

int dcf_op_local_attn_drop(const float* Q, const float* K, const float* V, const uint8_t* mask, float* O, int32_t B, int32_t T, int32_t C,
                           int32_t heads, int32_t window, int32_t b0, int64_t seed, int32_t site, float p, void* stream) {
  LocalAttnDropArgs a{Q, K, V, mask, O, nullptr, nullptr, nullptr, nullptr, nullptr, B, T, C, heads, window, b0, (uint64_t)seed, (uint32_t)site,
                      p, 1.0f / (1.0f - p)};
  DCF_CHECK(aligned16(Q) && aligned16(K) && aligned16(V) && aligned16(O), "dcf_op_local_attn_drop: pointers must be 16-byte aligned");
  if (window == 0) {                                     // global self attention, as dcf_op_local_attn defines it
    const char* who = "dcf_op_local_attn_drop (window = 0)";
    DCF_CHECK(Q && K && V && mask && O, "%s: null operand", who);
    const DenseAttnDropArgs g = dense_args(Q, K, V, mask, O, nullptr, nullptr, nullptr, nullptr, B, T, T, C, heads, b0, seed, site, p);
    if (dense_check(who, g, 32, 64, (1 << 30))) return -1;
    if (p == 0.f) return dcf_op_local_attn(Q, K, V, mask, O, B, T, C, heads, 0, stream);
    return launch_dense_attn_drop(who, g, false, (hipStream_t)stream);
  }
  return launch_local_attn_drop(a, (hipStream_t)stream);
}

int dcf_op_local_attn_drop_bwd(const float* Q, const float* K, const float* V, const uint8_t* mask, const float* dO, float* dQ, float* dK,
                               float* dV, int32_t B, int32_t T, int32_t C, int32_t heads, int32_t window, int32_t b0, int64_t seed,
                               int32_t site, float p, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  LocalAttnDropArgs a{Q, K, V, mask, nullptr, dO, dQ, dK, dV, nullptr, B, T, C, heads, window, b0, (uint64_t)seed, (uint32_t)site,
                      p, 1.0f / (1.0f - p)};
  DCF_CHECK(aligned16(Q) && aligned16(K) && aligned16(V) && aligned16(dO) && aligned16(dQ) && aligned16(dK) && aligned16(dV),
            "dcf_op_local_attn_drop_bwd: pointers must be 16-byte aligned");
  if (!dK && !dV) return launch_local_attn_drop_bwd(a, st);
  // every check comes before the scratch: an unsupported shape allocates and launches nothing
  DCF_CHECK(Q && K && V && dO, "dcf_op_local_attn_drop_bwd: null operand");
  if (ad_check("dcf_op_local_attn_drop_bwd", a)) return -1;
  // the row statistics (and keep bits) the key-side gather reads: stream-ordered scratch, no host wait
  StreamScratch sc(st);
  if (sc.take(&a.stats, (size_t)B * T * heads * 4)) return -1;
  return sc.end(launch_local_attn_drop_bwd(a, st));
}

int dcf_op_global_attn_drop_bwd(const float* Q, const float* K, const float* V, const uint8_t* mask, const float* dO, float* dQ, float* dK,
                                float* dV, int32_t B, int32_t T, int32_t C, int32_t heads, int32_t b0, int64_t seed, int32_t site, float p,
                                void* stream) {
  const char* who = "dcf_op_global_attn_drop_bwd";
  DCF_CHECK(Q && K && V && dO, "%s: null operand", who);
  const DenseAttnDropArgs a = dense_args(Q, K, V, mask, nullptr, dO, dQ, dK, dV, B, T, T, C, heads, b0, seed, site, p);
  if (dense_check(who, a, 32, 64, (1 << 30))) return -1;
  DCF_CHECK(aligned16(Q) && aligned16(K) && aligned16(V) && aligned16(dO) && aligned16(dQ) && aligned16(dK) && aligned16(dV),
            "%s: pointers must be 16-byte aligned", who);
  if (p == 0.f) return dcf_op_global_attn_bwd(Q, K, V, mask, dO, dQ, dK, dV, B, T, C, heads, stream);
  return dense_attn_drop_bwd(who, a, (hipStream_t)stream);
}

int dcf_op_xattn_drop(const float* Q, const float* K, const float* V, const uint8_t* kvmask, float* O, int32_t B, int32_t T, int32_t Lk, int32_t C,
                      int32_t heads, int32_t b0, int64_t seed, int32_t site, float p, void* stream) {
  const char* who = "dcf_op_xattn_drop";
  DCF_CHECK(Q && K && V && kvmask && O, "%s: null operand", who);
  const DenseAttnDropArgs a = dense_args(Q, K, V, kvmask, O, nullptr, nullptr, nullptr, nullptr, B, T, Lk, C, heads, b0, seed, site, p);
  if (dense_check(who, a, 16, 128, XG_MAX_LK)) return -1;
  DCF_CHECK(aligned16(Q) && aligned16(K) && aligned16(V) && aligned16(O), "%s: pointers must be 16-byte aligned", who);
  if (p == 0.f) return dcf_op_xattn(Q, K, V, kvmask, O, B, T, Lk, C, heads, stream);
  return launch_dense_attn_drop(who, a, false, (hipStream_t)stream);
}

int dcf_op_xattn_drop_bwd(const float* Q, const float* K, const float* V, const uint8_t* kvmask, const float* dO, float* dQ, float* dK, float* dV,
                          int32_t B, int32_t T, int32_t Lk, int32_t C, int32_t heads, int32_t b0, int64_t seed, int32_t site, float p,
                          void* stream) {
  const char* who = "dcf_op_xattn_drop_bwd";
  DCF_CHECK(Q && K && V && dO, "%s: null operand", who);
  const DenseAttnDropArgs a = dense_args(Q, K, V, kvmask, nullptr, dO, dQ, dK, dV, B, T, Lk, C, heads, b0, seed, site, p);
  if (dense_check(who, a, 16, 128, XG_MAX_LK)) return -1;
  DCF_CHECK(aligned16(Q) && aligned16(K) && aligned16(V) && aligned16(dO) && aligned16(dQ) && aligned16(dK) && aligned16(dV),
            "%s: pointers must be 16-byte aligned", who);
  if (p == 0.f) return dcf_op_xattn_bwd(Q, K, V, kvmask, dO, dQ, dK, dV, B, T, Lk, C, heads, stream);
  return dense_attn_drop_bwd(who, a, (hipStream_t)stream);
}

int dcf_op_channel_dropout(const float* X, float* Y, int32_t B, int32_t T, int32_t C, int32_t b0, int64_t seed, int32_t site, float p,
                           void* stream) {
  const char* who = "dcf_op_channel_dropout";
  DCF_CHECK(X && Y, "%s: null argument", who);
  DCF_CHECK(B > 0 && T > 0, "%s: empty batch (B = %d, T = %d)", who, B, T);
  DCF_CHECK(C > 0 && C % 4 == 0, "%s: C = %d must be a positive multiple of 4", who, C);
  DCF_CHECK((int64_t)B * T < (1ll << 31) - 64, "%s: %lld rows (< 2^31)", who, (long long)B * T);
  DCF_CHECK(b0 >= 0, "%s: b0 = %d must not be negative", who, b0);
  DCF_CHECK(p >= 0.f && p < 1.f, "%s: p = %g outside [0, 1)", who, (double)p);
  DCF_CHECK(aligned16(X) && aligned16(Y), "%s: pointers must be 16-byte aligned", who);
  if (p == 0.f && X == Y) return 0;
  const int64_t n = (int64_t)B * ((T + CD_ROWS - 1) / CD_ROWS) * (C / 4);
  DCF_CHECK((n + 255) / 256 < (1ll << 31), "%s: %lld thread blocks (< 2^31)", who, (long long)((n + 255) / 256));
  hipLaunchKernelGGL(k_channel_dropout, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, X, Y, B, T, C, b0, (uint64_t)seed,
                     (uint32_t)site, p, 1.0f / (1.0f - p));
  DCF_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
