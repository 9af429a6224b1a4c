// Attention-map dropout inside the attention cores, forward and backward -- the sliding-window core first, global self attention and
// cross attention in the section "dense attention" further down -- and channel dropout (include/decafnet_hip_attn_drop.h).  The map
// never exists in memory: k_local_attn (attn.hip) and its backward (attn_grad.hip) hold it in registers, so the keep bits are drawn
// where the map element is formed.
//
// The kernels are those two files' kernels with one more factor, written again here so that the released exports keep their compiled
// code: the same data layout (a wave owns a query row -- two in the unrolled forward --, a lane owns 4 consecutive channels of each
// 256-channel chunk, a head is a group of LPH = d / 4 adjacent lanes), the same expressions in the same order.  With P the softmax
// map, k the keep factor (scale = 1 / (1 - p) or 0) and Pd = k o P:
//   O_t = sum_j Pd_tj v_j            dV_j = sum_t Pd_tj dO_t          dPd_tj = dO_t . v_j        dP = k o dPd
//   delta_t = sum_j Pd_tj dPd_tj     dS = P o (dP - delta)            dQ, dK from dS as in attn_grad.hip
// The forward carries the softmax online, so the factor multiplies the un-normalised weight e = exp(s - m) on its way into the
// accumulator, not on its way into the running sum: O = (sum_j k e_j v_j) / (sum_j e_j).
//
// p = 0 runs the dropout-free kernels themselves (launch_local_attn, launch_local_attn_bwd; the dense forms call their exports):
// the bits of the dropout-free exports by construction.  A factor of 1.0f changes no bit either, but a second copy of an expression like D * corr + e * dP is contracted into
// an FMA per instantiation, and the compiler took the other product in one variant here (the loop form of the query side: dQ off by
// an ulp at p = 0); equal bits must not rest on that.  The kernels below therefore run with p > 0 only.
//
// Keep bits.  Element (b, h, t, slot) of the reference's (bs, H, T, W) map has index e = (((b0 + b) H + h) T + t) W + slot; slot is
// key t - W / 2 + slot.  The W elements of a (row, head) are consecutive, so they lie in at most (W + 6) / 4 counter blocks of the
// Philox stream.  For W <= 32 the lanes of a head's group draw different blocks of the row and OR their words together with lane
// permutes: one 32-bit word per (row, head) and chunk, bit `slot` = kept, one Philox block per lane and row at W = 9 / 19 with d >= 24
// instead of one per lane and key.  The backward's query-side kernel leaves that word in the fourth slot of the row statistics, where
// the key-side gather -- which meets every (query, key) pair from the key's side, a different row per pair -- picks it up with the
// statistics it loads anyway.  Wider windows draw per element, on both sides.
#include "attn_drop.h"

#include "attn.h"
#include "attn_grad.h"
#include "xattn_grad.h"
#include "../../include/decafnet_hip_attn.h"
#include "../../include/decafnet_hip_attn_drop.h"
#include "dropout.h"
#include "grad_common.h"

namespace dcf {

constexpr int AD_PACK_MAX = 32;        // widest window whose keep bits are packed into one word per (row, head)

template <int LPH>
__device__ __forceinline__ float ad_head_sum(float v) {
  if constexpr (LPH == 1) return v;
  else return group_sum<LPH>(v);
}

// the forward's exp and 4-channel partial (attn.hip)
__device__ __forceinline__ float ad_fast_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896340736f); }
__device__ __forceinline__ float ad_dot4(const f32x4& a, const f32x4& b) {
  return (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w);
}

template <int NCH>
__device__ __forceinline__ void ad_scale_row(Row<NCH>& r, float s) {
#pragma unroll
  for (int j = 0; j < NCH; ++j) r.v[j] *= s;
}

// keep bits of the W (<= 32) elements e0 .. e0 + W - 1 of one (row, head): bit slot <-> element e0 + slot.  The LPH lanes of the head
// take the row's counter blocks in turn (the row starts at word e0 & 3 of its first block) and OR their parts over the group; every
// lane of the wave must call it (the exchange is a lane permute).
template <int LPH>
__device__ __forceinline__ uint32_t row_keep_bits(uint64_t seed, uint32_t site, float p, uint64_t e0, int W, int lane) {
  const uint64_t blk0 = e0 >> 2;
  const int off = (int)(e0 & 3), nblk = (off + W + 3) >> 2, nmax = (W + 6) >> 2;   // nmax: the wave-uniform bound of nblk
  uint32_t bits = 0;
  for (int i0 = 0; i0 < nmax; i0 += LPH) {
    const int i = i0 + (lane & (LPH - 1));
    if (i < nblk) {
      const Philox4 v = drop_block(seed, site, blk0 + (uint64_t)i);
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const int slot = 4 * i + w - off;
        if (slot >= 0 && slot < W) bits |= (uint32_t)drop_keep_word(philox_word(v, w), p) << slot;
      }
    }
  }
#pragma unroll
  for (int s = 1; s < LPH; s <<= 1) bits |= (uint32_t)__shfl_xor((int)bits, s);
  return bits;
}

// the keep decisions of one query row as a lane sees them: per 256-channel chunk the lane's head, hence its own word / first element
template <int NCH, int LPH>
struct RowKeep {
  uint32_t bits[NCH];
  uint64_t e0[NCH];
  // row t of sequence bg = b0 + b of the reference's batch
  __device__ __forceinline__ void init(const LocalAttnDropArgs& p, int64_t bg, int t, int lane, bool packed) {
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      const int hd = (64 * j + lane) / LPH;
      e0[j] = (uint64_t)(((bg * p.heads + hd) * (int64_t)p.T + t) * (int64_t)p.window);
      bits[j] = packed ? row_keep_bits<LPH>(p.seed, p.site, p.p, e0[j], p.window, lane) : 0u;
    }
  }
  __device__ __forceinline__ bool kept(const LocalAttnDropArgs& p, int j, int slot, bool packed) const {
    if (packed) return ((bits[j] >> slot) & 1u) != 0;
    return drop_keep(p.seed, p.site, e0[j] + (uint64_t)slot, p.p);
  }
};

// ------------------------------------------------------------------------------------------
// forward: k_local_attn (attn.hip) with the keep factor on the weight that enters the accumulator
// ------------------------------------------------------------------------------------------
constexpr int AD_QPW = 2;              // query rows per wave of the unrolled variants (LA_QPW, attn.hip)

template <int NCH, int LPH, int WMAX>
__global__ __launch_bounds__(256) void k_local_attn_drop(LocalAttnDropArgs p) {
  constexpr int QPW = WMAX > 0 ? AD_QPW : 1;
  const int lane = threadIdx.x & 63;
  const int wps = (p.T + QPW - 1) / QPW;               // waves per sequence
  const int64_t w = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (w >= (int64_t)p.B * wps) return;
  const int C = p.C;
  const int t = (int)(w % wps) * QPW;
  const int64_t base = (w / wps) * p.T, r = base + t;
  const int half = p.window / 2;
  const float scale = 1.0f / sqrtf(sqrtf((float)(C / p.heads)));
  const bool packed = WMAX > 0 || p.window <= AD_PACK_MAX;
  const int nq = min(QPW, p.T - t);
  const int lo = max(t - half, 0), hi = min(t + (nq - 1) + half, p.T - 1);
  unsigned long long km = 0ull;
  if constexpr (WMAX > 0) km = __ballot(lane <= hi - lo && p.mask[base + lo + lane] != 0);
  bool live[QPW];
  RowKeep<NCH, LPH> keep[QPW];
#pragma unroll
  for (int z = 0; z < QPW; ++z) {
    live[z] = z < nq && p.mask[r + (z < nq ? z : 0)] != 0;       // padded query rows are forced to 0 (blocks.py:293)
    keep[z].init(p, p.b0 + w / wps, t + z, lane, packed);
  }
  auto fetch = [&](int u, Row<NCH>& k, Row<NCH>& v) __attribute__((always_inline)) {
    k.load(p.K + (base + u) * C, C, lane);
    v.load(p.V + (base + u) * C, C, lane);
  };
  Row<NCH> kb[2], vb[2];
  if constexpr (WMAX > 0) {
    fetch(lo, kb[0], vb[0]);
    fetch(lo + 1 <= hi ? lo + 1 : hi, kb[1], vb[1]);
  }
  Row<NCH> q[QPW];
  f32x4 acc[QPW][NCH];
  float m[QPW][NCH], l[QPW][NCH];
#pragma unroll
  for (int z = 0; z < QPW; ++z) {
    q[z].load(p.Q + (r + (z < nq ? z : 0)) * C, C, lane);
#pragma unroll
    for (int j = 0; j < NCH; ++j) { q[z].v[j] *= scale; acc[z][j] = f32x4{0.f, 0.f, 0.f, 0.f}; m[z][j] = -INFINITY; l[z][j] = 0.f; }
  }
  // key u of query z is slot u - (t + z - half) of that row of the map
  auto key = [&](int z, bool valid, int u, const Row<NCH>& k, const Row<NCH>& v) __attribute__((always_inline)) {
    const float pen = valid ? 0.f : -1e4f;             // padded keys get a finite -1e4 (blocks.py:279)
    const int slot = u - (t + z - half);
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      float s = ad_head_sum<LPH>(ad_dot4(q[z].v[j], k.v[j] * scale)) + pen;
      float mn = fmaxf(m[z][j], s);
      float corr = ad_fast_exp(m[z][j] - mn);          // exp(-inf) = 0 on the first key
      float e = ad_fast_exp(s - mn);
      const float ek = keep[z].kept(p, j, slot, packed) ? e * p.scale : 0.f;   // a dropped element is +0
      acc[z][j] = acc[z][j] * corr + ek * v.v[j];
      l[z][j] = l[z][j] * corr + e;                    // the softmax is the dropout-free one
      m[z][j] = mn;
    }
  };
  if constexpr (WMAX > 0) {
#pragma unroll
    for (int i = 0; i < WMAX + QPW - 1; ++i) {
      const int u = lo + i;
      if (u > hi) break;
      const bool valid = ((km >> i) & 1ull) != 0;
#pragma unroll
      for (int z = 0; z < QPW; ++z)
        if (live[z] && u >= t + z - half && u <= t + z + half) key(z, valid, u, kb[i & 1], vb[i & 1]);
      if (i + 2 < WMAX + QPW - 1 && u + 2 <= hi) fetch(u + 2, kb[i & 1], vb[i & 1]);   // this register set is free again
    }
  } else {
    if (live[0]) {
      for (int u = lo; u <= hi; ++u) {
        fetch(u, kb[0], vb[0]);
        key(0, p.mask[base + u] != 0, u, kb[0], vb[0]);
      }
    }
  }
#pragma unroll
  for (int z = 0; z < QPW; ++z) {
    if (z >= nq) break;
    Row<NCH> o;
#pragma unroll
    // (+ 0.0f: a zero leaves as +0.  A window that opens with kept padded keys carries their values until the first valid key rescales
    // them by exp(-1e4) = 0, which leaves the sign of what was there: -0 where every valid key is dropped afterwards.)
    for (int j = 0; j < NCH; ++j) o.v[j] = live[z] ? acc[z][j] / l[z][j] + 0.0f : f32x4{0.f, 0.f, 0.f, 0.f};
    o.store(p.O + (r + z) * C, C, lane);
  }
}

// ------------------------------------------------------------------------------------------
// backward, query side (k_attn_bwd_q, attn_grad.hip): statistics, the row's keep bits, dQ
// ------------------------------------------------------------------------------------------
template <int NCH, int LPH, int WMAX>
__global__ __launch_bounds__(256) void k_attn_drop_bwd_q(LocalAttnDropArgs p) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (r >= (int64_t)p.B * p.T) return;
  const int C = p.C;
  const int t = (int)(r % p.T);
  const int64_t base = r - t;
  if (p.mask && p.mask[r] == 0) {                        // a padded query: P_t. = 0, so dQ_t = 0 and it feeds no key
    if (p.dQ) { Row<NCH> z; z.zero(); z.store(p.dQ + r * C, C, lane); }
    return;
  }
  const int half = p.window / 2;
  const int lo = max(t - half, 0), hi = min(t + half, p.T - 1), n = hi - lo + 1;
  const int slot0 = lo - (t - half);                     // slot of key lo
  const float scale = 1.0f / sqrtf(sqrtf((float)(C / p.heads)));
  const bool packed = WMAX > 0 || p.window <= AD_PACK_MAX;
  unsigned long long km = ~0ull;
  if constexpr (WMAX > 0) {
    if (p.mask) km = __ballot(lane < n && p.mask[base + lo + lane] != 0);
  }
  RowKeep<NCH, LPH> keep;
  keep.init(p, p.b0 + base / p.T, t, lane, packed);
  Row<NCH> q, g, dq;
  q.load(p.Q + r * C, C, lane);
  g.load(p.dO + r * C, C, lane);
  ad_scale_row(q, scale);
  dq.zero();
  float m[NCH], l[NCH], D[NCH];
#pragma unroll
  for (int j = 0; j < NCH; ++j) { m[j] = -INFINITY; l[j] = 0.f; D[j] = 0.f; }

  auto score = [&](const Row<NCH>& k, const Row<NCH>& v, bool valid, float* s, float* dp) __attribute__((always_inline)) {
    const float pen = valid ? 0.f : -1e4f;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      s[j] = ad_head_sum<LPH>(dotp(q.v[j], k.v[j] * scale)) + pen;
      dp[j] = ad_head_sum<LPH>(dotp(g.v[j], v.v[j]));    // dPd: the gradient at the dropped map
    }
  };
  auto online = [&](const float* s, const float* dp, int slot) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      const float mn = fmaxf(m[j], s[j]);
      const float corr = m[j] == -INFINITY ? 0.f : exp_res(m[j] - mn);
      const float e = exp_res(s[j] - mn);
      const float ek = keep.kept(p, j, slot, packed) ? e * p.scale : 0.f;
      l[j] = l[j] * corr + e;
      D[j] = D[j] * corr + ek * dp[j];                   // delta = sum_j Pd dPd
      m[j] = mn;
    }
  };
  float il[NCH], delta[NCH];
  auto finish = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      il[j] = 1.0f / l[j];                               // the query sees itself: l >= 1
      delta[j] = D[j] * il[j];
      if (p.stats && lane % LPH == 0 && 256 * j + 4 * lane < C)
        *reinterpret_cast<f32x4*>(p.stats + (r * p.heads + (64 * j + lane) / LPH) * 4) =
            f32x4{m[j], il[j], delta[j], __uint_as_float(keep.bits[j])};     // (the word is moved, never computed with)
    }
  };
  auto accum = [&](const float* s, const float* dp, int slot, const Row<NCH>& k) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      const float pj = exp_res(s[j] - m[j]) * il[j];
      const float dpk = keep.kept(p, j, slot, packed) ? dp[j] * p.scale : 0.f;   // dP = k o dPd
      const float ds = pj * (dpk - delta[j]);
      dq.v[j] += ds * (k.v[j] * scale);
    }
  };

  if constexpr (WMAX > 0) {
    float s[WMAX][NCH], dp[WMAX][NCH];
    Row<NCH> kb[2], vb[2];
    kb[0].load(p.K + (base + lo) * C, C, lane);
    vb[0].load(p.V + (base + lo) * C, C, lane);
    kb[1].load(p.K + (base + min(lo + 1, hi)) * C, C, lane);
    vb[1].load(p.V + (base + min(lo + 1, hi)) * C, C, lane);
#pragma unroll
    for (int i = 0; i < WMAX; ++i) {
      if (i < n) {
        score(kb[i & 1], vb[i & 1], ((km >> i) & 1ull) != 0, s[i], dp[i]);
        online(s[i], dp[i], slot0 + i);
      }
      if (i + 2 < WMAX && i + 2 < n) {
        kb[i & 1].load(p.K + (base + lo + i + 2) * C, C, lane);
        vb[i & 1].load(p.V + (base + lo + i + 2) * C, C, lane);
      }
    }
    finish();
    if (p.dQ) {
      kb[0].load(p.K + (base + lo) * C, C, lane);
      kb[1].load(p.K + (base + min(lo + 1, hi)) * C, C, lane);
#pragma unroll
      for (int i = 0; i < WMAX; ++i) {
        if (i < n) accum(s[i], dp[i], slot0 + i, kb[i & 1]);
        if (i + 2 < WMAX && i + 2 < n) kb[i & 1].load(p.K + (base + lo + i + 2) * C, C, lane);
      }
    }
  } else {
    float s[NCH], dp[NCH];
    Row<NCH> k, v;
    for (int u = lo; u <= hi; ++u) {
      k.load(p.K + (base + u) * C, C, lane);
      v.load(p.V + (base + u) * C, C, lane);
      score(k, v, !p.mask || p.mask[base + u] != 0, s, dp);
      online(s, dp, slot0 + u - lo);
    }
    finish();
    if (p.dQ) {
      for (int u = lo; u <= hi; ++u) {                   // the same expressions on the same operands: the same s and dPd
        k.load(p.K + (base + u) * C, C, lane);
        v.load(p.V + (base + u) * C, C, lane);
        score(k, v, !p.mask || p.mask[base + u] != 0, s, dp);
        accum(s, dp, slot0 + u - lo, k);
      }
    }
  }
  if (p.dQ) {
    ad_scale_row(dq, scale);
    dq.store(p.dQ + r * C, C, lane);
  }
}

// ------------------------------------------------------------------------------------------
// backward, key side (k_attn_bwd_kv, attn_grad.hip): dK and dV as a gather over the queries whose band holds the key
// ------------------------------------------------------------------------------------------
template <int NCH, int LPH, int WMAX>
__global__ __launch_bounds__(256) void k_attn_drop_bwd_kv(LocalAttnDropArgs p) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (r >= (int64_t)p.B * p.T) return;
  const int C = p.C;
  const int t = (int)(r % p.T);
  const int64_t base = r - t;
  const int half = p.window / 2;
  const int lo = max(t - half, 0), hi = min(t + half, p.T - 1), n = hi - lo + 1;
  const float scale = 1.0f / sqrtf(sqrtf((float)(C / p.heads)));
  const float pen = (p.mask && p.mask[r] == 0) ? -1e4f : 0.f;
  const bool packed = WMAX > 0 || p.window <= AD_PACK_MAX;
  const int64_t bg = p.b0 + base / p.T;
  unsigned long long qm = ~0ull;
  if constexpr (WMAX > 0) {
    if (p.mask) qm = __ballot(lane < n && p.mask[base + lo + lane] != 0);
  }
  Row<NCH> k, v, dk, dv;
  k.load(p.K + r * C, C, lane);
  v.load(p.V + r * C, C, lane);
  ad_scale_row(k, scale);
  dk.zero();
  dv.zero();
  const bool want_dk = p.dK != nullptr;

  auto fetch = [&](int u, Row<NCH>& q, Row<NCH>& g, f32x4* st) __attribute__((always_inline)) {
    q.load(p.Q + (base + u) * C, C, lane);
    g.load(p.dO + (base + u) * C, C, lane);
#pragma unroll
    for (int j = 0; j < NCH; ++j)
      st[j] = 256 * j + 4 * lane < C ? *reinterpret_cast<const f32x4*>(p.stats + ((base + u) * p.heads + (64 * j + lane) / LPH) * 4)
                                     : f32x4{0.f, 0.f, 0.f, 0.f};
  };
  // key t is slot t - (u - half) of query u's row of the map
  auto query = [&](int u, const Row<NCH>& q, const Row<NCH>& g, const f32x4* st) __attribute__((always_inline)) {
    const int slot = t - u + half;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      bool kept;
      if (packed) kept = ((__float_as_uint(st[j].w) >> slot) & 1u) != 0;
      else {
        const int hd = (64 * j + lane) / LPH;
        kept = drop_keep(p.seed, p.site, (uint64_t)(((bg * p.heads + hd) * (int64_t)p.T + u) * (int64_t)p.window + slot), p.p);
      }
      const f32x4 qs = q.v[j] * scale;
      const float s = ad_head_sum<LPH>(dotp(qs, k.v[j])) + pen;
      const float pj = exp_res(s - st[j].x) * st[j].y;
      const float pk = kept ? pj * p.scale : 0.f;
      dv.v[j] += pk * g.v[j];
      if (want_dk) {
        const float dp = ad_head_sum<LPH>(dotp(g.v[j], v.v[j]));
        const float dpk = kept ? dp * p.scale : 0.f;
        const float ds = pj * (dpk - st[j].z);
        dk.v[j] += ds * qs;
      }
    }
  };

  if constexpr (WMAX > 0) {
    Row<NCH> qb[2], gb[2];
    f32x4 sb[2][NCH];
    fetch(lo, qb[0], gb[0], sb[0]);
    fetch(min(lo + 1, hi), qb[1], gb[1], sb[1]);
#pragma unroll
    for (int i = 0; i < WMAX; ++i) {
      if (i < n && ((qm >> i) & 1ull)) query(lo + i, qb[i & 1], gb[i & 1], sb[i & 1]);   // a padded query attends to nothing
      if (i + 2 < WMAX && i + 2 < n) fetch(lo + i + 2, qb[i & 1], gb[i & 1], sb[i & 1]);
    }
  } else {
    Row<NCH> q, g;
    f32x4 st[NCH];
    for (int u = lo; u <= hi; ++u) {
      if (p.mask && p.mask[base + u] == 0) continue;
      fetch(u, q, g, st);
      query(u, q, g, st);
    }
  }
  if (p.dK) {
    ad_scale_row(dk, scale);
    dk.store(p.dK + r * C, C, lane);
  }
  if (p.dV) dv.store(p.dV + r * C, C, lane);
}

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
  ad_scale_row(q, scale);
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
      for (int j = 0; j < NCH; ++j) m[j] = fmaxf(m[j], ad_head_sum<LPH>(dotp(q.v[j], k.v[j] * scale)));
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
        const float s = ad_head_sum<LPH>(dotp(q.v[j], k.v[j] * scale));
        if constexpr (BWD) {
          const float e = exp_res(s - m[j]);
          const float ek = ((bits[j] >> jj) & 1u) ? e * p.scale : 0.f;
          l[j] += e;
          D[j] += ek * ad_head_sum<LPH>(dotp(g.v[j], v.v[j]));
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
        const float s = ad_head_sum<LPH>(dotp(q.v[j], k.v[j] * scale));
        const float dp = ad_head_sum<LPH>(dotp(g.v[j], v.v[j]));
        const float pj = exp_res(s - m[j]) * il[j];
        const float dpk = ((bits[j] >> jj) & 1u) ? dp * p.scale : 0.f;
        dq.v[j] += (pj * (dpk - delta[j])) * (k.v[j] * scale);
      }
    }
  }
  ad_scale_row(dq, scale);
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
    ad_scale_row(k, scale);
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
        const float s = ad_head_sum<LPH>(dotp(qs, k.v[j]));
        const float pj = exp_res(s - st.x) * st.y;
        const float pk = kept ? pj * p.scale : 0.f;
        dv.v[j] += pk * g.v[j];
        if (want_dk) {
          const float dp = ad_head_sum<LPH>(dotp(g.v[j], v.v[j]));
          const float dpk = kept ? dp * p.scale : 0.f;
          dk.v[j] += (pj * (dpk - st.z)) * qs;
        }
      }
    }
  }
  if (p.dK) {
    ad_scale_row(dk, scale);
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
  DCF_CHECK(a.B > 0 && a.T > 0 && a.heads > 0, "%s: empty batch (B=%d T=%d heads=%d)", who, a.B, a.T, a.heads);
  DCF_CHECK(a.window != 0, "%s: window = 0 (global attention) has its backward in dcf_op_global_attn_drop_bwd", who);
  DCF_CHECK(a.window >= 1 && a.window % 2 == 1, "%s: window = %d must be odd and >= 1", who, a.window);
  DCF_CHECK(a.C > 0 && a.C % a.heads == 0, "%s: C=%d not divisible by heads=%d", who, a.C, a.heads);
  const int d = a.C / a.heads, nch = (a.C + 255) / 256;
  DCF_CHECK(a.C % 4 == 0 && nch <= 4 && d >= 4 && d <= 256 && (d & (d - 1)) == 0,
            "%s: unsupported C=%d / head dim=%d (need power-of-two head dim in [4,256], C<=1024)", who, a.C, d);
  DCF_CHECK((int64_t)a.B * a.T < (1ll << 31) - 64, "%s: %lld rows (< 2^31)", who, (long long)a.B * a.T);
  DCF_CHECK(a.b0 >= 0, "%s: b0 = %d must not be negative", who, a.b0);
  DCF_CHECK(a.p >= 0.f && a.p < 1.f, "%s: p = %g outside [0, 1)", who, (double)a.p);
  return 0;
}

template <int NCH, int LPH, int WMAX>
static void ad_launch_fwd(const LocalAttnDropArgs& a, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL((k_local_attn_drop<NCH, LPH, WMAX>), grid, dim3(256), 0, st, a);
}
template <int NCH, int LPH, int WMAX>
static void ad_launch_bwd(const LocalAttnDropArgs& a, dim3 grid, bool kv, hipStream_t st) {
  hipLaunchKernelGGL((k_attn_drop_bwd_q<NCH, LPH, WMAX>), grid, dim3(256), 0, st, a);
  if (kv) hipLaunchKernelGGL((k_attn_drop_bwd_kv<NCH, LPH, WMAX>), grid, dim3(256), 0, st, a);
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
#define AD_DISPATCH(WHAT) do {                                                            \
    switch (nch * 100 + lph) {                           /* the forward's table (DISPATCH_ATTN, attn.hip) */ \
      case 101: WHAT(1, 1); break;   case 102: WHAT(1, 2); break;   case 104: WHAT(1, 4); break;   case 108: WHAT(1, 8); break; \
      case 116: WHAT(1, 16); break;  case 132: WHAT(1, 32); break;  case 164: WHAT(1, 64); break;  \
      case 208: WHAT(2, 8); break;   case 216: WHAT(2, 16); break;  case 232: WHAT(2, 32); break;  case 264: WHAT(2, 64); break; \
      case 316: WHAT(3, 16); break;  case 332: WHAT(3, 32); break;  case 364: WHAT(3, 64); break;  \
      case 416: WHAT(4, 16); break;  case 432: WHAT(4, 32); break;  case 464: WHAT(4, 64); break;  \
      default: ok = false;                                                                \
    } } while (0)

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
  if (bwd) AD_DISPATCH(AD_DENSE_BWD);
  else AD_DISPATCH(AD_DENSE_FWD);
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
  const int qpw = a.window <= 19 ? AD_QPW : 1;
  const dim3 grid((unsigned)(((int64_t)a.B * ((a.T + qpw - 1) / qpw) + 3) / 4));
  bool ok = true;
  AD_DISPATCH(AD_FWD);
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
  AD_DISPATCH(AD_BWD);
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
