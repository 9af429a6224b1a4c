// The sliding-window attention kernels -- forward (instantiated in attn.hip), backward query side and key side (attn_grad.hip) --
// each written once, with and without dropout on the attention map (instantiated in attn_drop.hip), and what the row-per-wave
// attention kernels share: the head sum, the forward's exp and 4-channel partial, the keep bits of a row of the map and the table of
// compiled row shapes.
//
// A kernel is templated on its argument struct.  With LocalAttnArgs / LocalAttnGradArgs it is the dropout-free kernel; with
// LocalAttnDropArgs (map_drop<Args>) every map element passes through its keep factor on the way into a sum.  The switch is made at
// compile time: every dropout expression sits behind `if constexpr (DROP)` -- mostly inside a kernel's small kf(), which returns its
// operand without dropout -- so the dropout-free instantiations compile to the instruction streams they had before the kernels were
// templates (no factor of 1.0f that a contraction could treat differently in one variant), and their kernel arguments keep their
// layout.  Written any other way that still folds to the same arithmetic (an empty helper object, a helper that takes `p`), the
// compiler ordered or allocated a few of them differently: compare the device assembly of every instantiation after a change here
// (tools/isa_diff.py; profiles/attn_drop.md, "One source").
//
// With P the softmax map, k the keep factor (scale = 1 / (1 - p) or 0) and Pd = k o P:
//   O_t = sum_j Pd_tj v_j            dV_j = sum_t Pd_tj dO_t          dPd_tj = dO_t . v_j        dP = k o dPd
//   delta_t = sum_j Pd_tj dPd_tj     dS = P o (dP - delta)            dQ, dK from dS (attn_grad.hip)
// The forward carries the softmax online, so the factor multiplies the un-normalised weight e = exp(s - m) on its way into the
// accumulator, not on its way into the running sum: O = (sum_j k e_j v_j) / (sum_j e_j).
//
// Keep bits.  Element (b, h, t, slot) of the reference's (bs, H, T, W) map has index e = (((b0 + b) H + h) T + t) W + slot; slot is
// key t - W / 2 + slot.  The W elements of a (row, head) are consecutive, so they lie in at most (W + 6) / 4 counter blocks of the
// Philox stream.  For W <= 32 the lanes of a head's group draw different blocks of the row and OR their words together with lane
// permutes: one 32-bit word per (row, head) and chunk, bit `slot` = kept, one Philox block per lane and row at W = 9 / 19 with d >= 24
// instead of one per lane and key.  The backward's query-side kernel leaves that word in the fourth slot of the row statistics, where
// the key-side gather -- which meets every (query, key) pair from the key's side, a different row per pair -- picks it up with the
// statistics it loads anyway.  Wider windows draw per element, on both sides.
#pragma once
#include <type_traits>

#include "attn.h"
#include "attn_drop.h"
#include "attn_grad.h"
#include "dropout.h"
#include "grad_common.h"

namespace dcf {

// The (256-channel chunks per row, lanes per head) pairs the row-per-wave attention kernels are compiled for:
// WHAT(NCH, LPH, ...) of the pair nch * 100 + lph, or ok = false where there is none.
#define DCF_ATTN_ROW_SHAPES(nch, lph, ok, WHAT, ...)                                                 \
  do {                                                                                               \
    switch ((nch) * 100 + (lph)) {                                                                   \
      case 101: WHAT(1, 1, ##__VA_ARGS__); break;                                                    \
      case 102: WHAT(1, 2, ##__VA_ARGS__); break;                                                    \
      case 104: WHAT(1, 4, ##__VA_ARGS__); break;                                                    \
      case 108: WHAT(1, 8, ##__VA_ARGS__); break;                                                    \
      case 116: WHAT(1, 16, ##__VA_ARGS__); break;                                                   \
      case 132: WHAT(1, 32, ##__VA_ARGS__); break;                                                   \
      case 164: WHAT(1, 64, ##__VA_ARGS__); break;                                                   \
      case 208: WHAT(2, 8, ##__VA_ARGS__); break;                                                    \
      case 216: WHAT(2, 16, ##__VA_ARGS__); break;                                                   \
      case 232: WHAT(2, 32, ##__VA_ARGS__); break;                                                   \
      case 264: WHAT(2, 64, ##__VA_ARGS__); break;                                                   \
      case 316: WHAT(3, 16, ##__VA_ARGS__); break;                                                   \
      case 332: WHAT(3, 32, ##__VA_ARGS__); break;                                                   \
      case 364: WHAT(3, 64, ##__VA_ARGS__); break;                                                   \
      case 416: WHAT(4, 16, ##__VA_ARGS__); break;                                                   \
      case 432: WHAT(4, 32, ##__VA_ARGS__); break;                                                   \
      case 464: WHAT(4, 64, ##__VA_ARGS__); break;                                                   \
      default: (ok) = false;                                                                         \
    }                                                                                                \
  } while (0)

template <int LPH>
__device__ __forceinline__ float head_sum(float v) {
  if constexpr (LPH == 1) return v;
  else return group_sum<LPH>(v);
}

// exp(x) for x <= 0 (softmax after max subtraction) as one v_exp_f32: exp2(x * log2(e)).  Relative error
// ~ (1 + |x|) * 2^-23; arguments below -126/log2(e) flush to 0 exactly like the tail of expf would round.
__device__ __forceinline__ float fast_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896340736f); }

__device__ __forceinline__ float dot4(const f32x4& a, const f32x4& b) {
  return (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w);
}

template <int NCH>
__device__ __forceinline__ void scale_row(Row<NCH>& r, float s) {
#pragma unroll
  for (int j = 0; j < NCH; ++j) r.v[j] *= s;
}

// ------------------------------------------------------------------------------------------
// the keep decisions of the map
// ------------------------------------------------------------------------------------------
template <class Args>
inline constexpr bool map_drop = std::is_same_v<Args, LocalAttnDropArgs>;

constexpr int LA_PACK_MAX = 32;        // widest window whose keep bits are packed into one word per (row, head)

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

// The keep decisions of one query row as a lane sees them: per 256-channel chunk the lane's head, hence its own word / first
// element.  Empty without dropout.
template <int NCH, int LPH, bool DROP>
struct RowKeep {};
template <int NCH, int LPH>
struct RowKeep<NCH, LPH, true> {
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
// forward.  One wave per query row, 8 waves per SIMD.  Measured alternatives (level 0, 26 us):
// all K/V rows of the window requested up front (4 waves/SIMD) 0.107 -> 0.120 ms per step; K/V of a 16-row strip staged
// once through LDS (3 workgroups per CU) 0.157; a strip of queries per wave with the window in a register ring 0.275 ->
// 0.314 ms per five-video forward (profiles/r02_gemm_operand_stream.md).
// ------------------------------------------------------------------------------------------
constexpr int LA_QPW = 2;      // (four rows per wave at 6 waves per SIMD: 0.251 ms per five-video forward against 0.231; one row: 0.256)
// WMAX > 0: windows of at most WMAX keys.  A wave takes LA_QPW = two consecutive query rows: their windows overlap in all but one key,
// so the 2 * (WMAX + 1) K / V row loads serve both (10 KiB instead of 18 KiB per query through the vector-memory path at
// w = 9, which is what bounds this kernel).  The key loop is fully unrolled (no loop-carried registers: the rows of the
// next keys stay in flight across the score -> exp -> accumulate chain of the current one with counted waits) and capped at
// 64 registers = 8 waves per SIMD so that the scheduler cannot hoist the whole window's loads.
// WMAX = 0: any window, one query per wave, one round trip per key.
// EAGER (WMAX > 0; small grids: the upper pyramid levels of one video): every K / V row of the wave's window requested at once.  With a
// few hundred waves on the chip nothing hides a round trip (1 - 2 us from the Infinity Cache, where the projections' output lies), and the
// two-row ring above makes a wave pay five of them in a row: 6.5 -> 3.6 us per launch at <= 4 096 rows.  Same operations, same bits.
// With dropout: no register cap and neither FULL nor EAGER variants (attn_drop.hip instantiates <NCH, LPH, false, WMAX, false>).
template <int NCH, int LPH, bool FULL, int WMAX, bool EAGER = false, class Args = LocalAttnArgs>
__global__ __launch_bounds__(256, map_drop<Args> ? 1 : (EAGER ? 2 : (WMAX > 0 && NCH == 1 ? 8 : 4))) void k_local_attn(Args p) {
  constexpr bool DROP = map_drop<Args>;
  constexpr int QPW = WMAX > 0 ? LA_QPW : 1;           // query rows per wave
  const int lane = threadIdx.x & 63;
  const int wps = (p.T + QPW - 1) / QPW;               // waves per sequence
  const int64_t w = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // scalar: the key loop is uniform
  if (w >= (int64_t)p.B * wps) return;
  const int C = FULL ? 256 * NCH : p.C;                 // FULL: every lane chunk exists, no per-lane channel predicate
  const int t = (int)(w % wps) * QPW;
  const int64_t base = (w / wps) * p.T, r = base + t;
  const int half = p.window / 2;
  const float scale = 1.0f / sqrtf(sqrtf((float)(C / p.heads)));
  const bool packed = DROP && (WMAX > 0 || p.window <= LA_PACK_MAX);
  // query z of the wave is row t + z (T may be odd: the second one may not exist); out-of-range keys are -inf (blocks.py:260-261)
  const int nq = min(QPW, p.T - t);
  const int lo = max(t - half, 0), hi = min(t + (nq - 1) + half, p.T - 1);
  // validity of the window's keys: one mask byte per lane (lane l <-> key lo + l), one ballot
  unsigned long long km = 0ull;
  if constexpr (WMAX > 0) km = __ballot(lane <= hi - lo && p.mask[base + lo + lane] != 0);
  bool live[QPW];
  RowKeep<NCH, LPH, DROP> keep[QPW];
#pragma unroll
  for (int z = 0; z < QPW; ++z) {
    live[z] = z < nq && p.mask[r + (z < nq ? z : 0)] != 0;       // padded query rows are forced to 0 (blocks.py:293)
    if constexpr (DROP) keep[z].init(p, p.b0 + w / wps, t + z, lane, packed);
  }
  auto fetch = [&](int u, Row<NCH>& k, Row<NCH>& v) __attribute__((always_inline)) {
    k.load(p.K + (base + u) * C, C, lane);
    v.load(p.V + (base + u) * C, C, lane);
  };
  constexpr int NKB = EAGER ? WMAX + QPW - 1 : 2;
  static_assert(!EAGER || WMAX > 0, "EAGER needs a bounded window");
  static_assert(!DROP || (!FULL && !EAGER), "the kernels with map dropout have no FULL / EAGER variants");
  Row<NCH> kb[NKB], vb[NKB];
  if constexpr (EAGER) {
#pragma unroll
    for (int i = 0; i < NKB; ++i) fetch(lo + i <= hi ? lo + i : hi, kb[i], vb[i]);
  } else if constexpr (WMAX > 0) {
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
  // x through the keep factor of the map at (query z, key u), which is slot u - (t + z - half) of that row of the map: k x with
  // dropout (a dropped element is +0), x itself without
  auto kf = [&](int z, int j, int u, float x) __attribute__((always_inline)) {
    if constexpr (DROP) return keep[z].kept(p, j, u - (t + z - half), packed) ? x * p.scale : 0.f;
    else return x;
  };
  auto key = [&](int z, bool valid, int u, const Row<NCH>& k, const Row<NCH>& v) __attribute__((always_inline)) {
    const float pen = valid ? 0.f : -1e4f;             // padded keys get a finite -1e4 (blocks.py:279)
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      float s = head_sum<LPH>(dot4(q[z].v[j], k.v[j] * scale)) + pen;
      float mn = fmaxf(m[z][j], s);
      float corr = fast_exp(m[z][j] - mn);             // exp(-inf) = 0 on the first key; v_exp_f32 instead of ~12-instruction expf
      float e = fast_exp(s - mn);
      acc[z][j] = acc[z][j] * corr + kf(z, j, u, e) * v.v[j];
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
        if (live[z] && u >= t + z - half && u <= t + z + half) key(z, valid, u, kb[EAGER ? i : (i & 1)], vb[EAGER ? i : (i & 1)]);
      if constexpr (!EAGER) {
        if (i + 2 < WMAX + QPW - 1 && u + 2 <= hi) fetch(u + 2, kb[i & 1], vb[i & 1]);   // this register set is free again
      }
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
    for (int j = 0; j < NCH; ++j) {
      // With dropout a zero leaves as +0.  A window that opens with kept padded keys carries their values until the first valid key
      // rescales them by exp(-1e4) = 0, which leaves the sign of what was there: -0 where every valid key is dropped afterwards.
      if constexpr (DROP) o.v[j] = live[z] ? acc[z][j] / l[z][j] + 0.0f : f32x4{0.f, 0.f, 0.f, 0.f};
      else o.v[j] = live[z] ? acc[z][j] / l[z][j] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    o.store(p.O + (r + z) * C, C, lane);
  }
}

// ------------------------------------------------------------------------------------------
// backward, query side: statistics, with dropout the row's keep bits, and dQ
// ------------------------------------------------------------------------------------------
template <int NCH, int LPH, int WMAX, class Args = LocalAttnGradArgs>
__global__ __launch_bounds__(256) void k_attn_bwd_q(Args p) {
  constexpr bool DROP = map_drop<Args>;
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // scalar: the key loop is uniform
  if (r >= (int64_t)p.B * p.T) return;
  const int C = p.C;
  const int t = (int)(r % p.T);
  const int64_t base = r - t;
  if (p.mask && p.mask[r] == 0) {                        // a padded query: p_t. = 0 (blocks.py:293), so dQ_t = 0 and it feeds no key
    if (p.dQ) { Row<NCH> z; z.zero(); z.store(p.dQ + r * C, C, lane); }
    return;
  }
  const int half = p.window / 2;
  const int lo = max(t - half, 0), hi = min(t + half, p.T - 1), n = hi - lo + 1;
  const int slot0 = lo - (t - half);                     // slot of key lo in the row of the map
  const float scale = 1.0f / sqrtf(sqrtf((float)(C / p.heads)));
  const bool packed = DROP && (WMAX > 0 || p.window <= LA_PACK_MAX);
  unsigned long long km = ~0ull;                         // validity of the window's keys: lane l <-> key lo + l, one ballot
  if constexpr (WMAX > 0) {
    if (p.mask) km = __ballot(lane < n && p.mask[base + lo + lane] != 0);
  }
  RowKeep<NCH, LPH, DROP> keep;
  if constexpr (DROP) keep.init(p, p.b0 + base / p.T, t, lane, packed);
  Row<NCH> q, g, dq;
  q.load(p.Q + r * C, C, lane);
  g.load(p.dO + r * C, C, lane);
  scale_row(q, scale);
  dq.zero();
  float m[NCH], l[NCH], D[NCH];
#pragma unroll
  for (int j = 0; j < NCH; ++j) { m[j] = -INFINITY; l[j] = 0.f; D[j] = 0.f; }

  // x through the keep factor of the map at `slot` of the row: k x with dropout (a dropped element is +0), x itself without
  auto kf = [&](int j, int slot, float x) __attribute__((always_inline)) {
    if constexpr (DROP) return keep.kept(p, j, slot, packed) ? x * p.scale : 0.f;
    else return x;
  };
  auto score = [&](const Row<NCH>& k, const Row<NCH>& v, bool valid, float* s, float* dp) __attribute__((always_inline)) {
    const float pen = valid ? 0.f : -1e4f;               // padded keys get a finite -1e4 (blocks.py:279)
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      s[j] = head_sum<LPH>(dotp(q.v[j], k.v[j] * scale)) + pen;
      dp[j] = head_sum<LPH>(dotp(g.v[j], v.v[j]));       // dPd: the gradient at the (dropped) map
    }
  };
  auto online = [&](const float* s, const float* dp, int slot) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      const float mn = fmaxf(m[j], s[j]);
      const float corr = m[j] == -INFINITY ? 0.f : exp_res(m[j] - mn);
      const float e = exp_res(s[j] - mn);
      const float ek = kf(j, slot, e);
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
      float word = 0.f;                                  // with dropout the row's keep bits (moved, never computed with)
      if constexpr (DROP) word = __uint_as_float(keep.bits[j]);
      if (p.stats && lane % LPH == 0 && 256 * j + 4 * lane < C)
        *reinterpret_cast<f32x4*>(p.stats + (r * p.heads + (64 * j + lane) / LPH) * 4) = f32x4{m[j], il[j], delta[j], word};
    }
  };
  auto accum = [&](const float* s, const float* dp, int slot, const Row<NCH>& k) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      const float pj = exp_res(s[j] - m[j]) * il[j];
      const float dpk = kf(j, slot, dp[j]);              // dP = k o dPd
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
      if (i < n) {                                       // (no break: a single-exit loop of known length unrolls fully)
        score(kb[i & 1], vb[i & 1], ((km >> i) & 1ull) != 0, s[i], dp[i]);
        online(s[i], dp[i], slot0 + i);
      }
      if (i + 2 < WMAX && i + 2 < n) {                   // this register set is free again
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
      for (int u = lo; u <= hi; ++u) {                   // the same expressions on the same operands: the same s and dP
        k.load(p.K + (base + u) * C, C, lane);
        v.load(p.V + (base + u) * C, C, lane);
        score(k, v, !p.mask || p.mask[base + u] != 0, s, dp);
        accum(s, dp, slot0 + u - lo, k);
      }
    }
  }
  if (p.dQ) {
    scale_row(dq, scale);
    dq.store(p.dQ + r * C, C, lane);
  }
}

// ------------------------------------------------------------------------------------------
// backward, key side: dK and dV as a gather over the queries whose band holds the key
// ------------------------------------------------------------------------------------------
template <int NCH, int LPH, int WMAX, class Args = LocalAttnGradArgs>
__global__ __launch_bounds__(256) void k_attn_bwd_kv(Args p) {
  constexpr bool DROP = map_drop<Args>;
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (r >= (int64_t)p.B * p.T) return;
  const int C = p.C;
  const int t = (int)(r % p.T);
  const int64_t base = r - t;
  const int half = p.window / 2;
  const int lo = max(t - half, 0), hi = min(t + half, p.T - 1), n = hi - lo + 1;    // |u - t| <= half is symmetric: the queries that see key t
  const float scale = 1.0f / sqrtf(sqrtf((float)(C / p.heads)));
  const float pen = (p.mask && p.mask[r] == 0) ? -1e4f : 0.f;
  const bool packed = DROP && (WMAX > 0 || p.window <= LA_PACK_MAX);
  [[maybe_unused]] int64_t bg = 0;                       // with dropout: the sequence's index in the reference's batch
  if constexpr (DROP) bg = p.b0 + base / p.T;
  unsigned long long qm = ~0ull;                         // liveness of those queries: lane l <-> query lo + l
  if constexpr (WMAX > 0) {
    if (p.mask) qm = __ballot(lane < n && p.mask[base + lo + lane] != 0);
  }
  Row<NCH> k, v, dk, dv;
  k.load(p.K + r * C, C, lane);
  v.load(p.V + r * C, C, lane);
  scale_row(k, scale);
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
  // key t is slot t - (u - half) of query u's row of the map, whose packed keep bits came with its statistics
  auto query = [&](int u, const Row<NCH>& q, const Row<NCH>& g, const f32x4* st) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      [[maybe_unused]] bool kept = true;
      if constexpr (DROP) {
        const int slot = t - u + half;
        if (packed) kept = ((__float_as_uint(st[j].w) >> slot) & 1u) != 0;
        else {
          const int hd = (64 * j + lane) / LPH;
          kept = drop_keep(p.seed, p.site, (uint64_t)(((bg * p.heads + hd) * (int64_t)p.T + u) * (int64_t)p.window + slot), p.p);
        }
      }
      const f32x4 qs = q.v[j] * scale;
      const float s = head_sum<LPH>(dotp(qs, k.v[j])) + pen;
      const float pj = exp_res(s - st[j].x) * st[j].y;
      float pk = pj;                                     // Pd = k o P (a dropped element is +0)
      if constexpr (DROP) pk = kept ? pj * p.scale : 0.f;
      dv.v[j] += pk * g.v[j];
      if (want_dk) {
        float dp = head_sum<LPH>(dotp(g.v[j], v.v[j]));
        if constexpr (DROP) dp = kept ? dp * p.scale : 0.f;      // dP = k o dPd
        const float ds = pj * (dp - st[j].z);
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
    scale_row(dk, scale);
    dk.store(p.dK + r * C, C, lane);
  }
  if (p.dV) dv.store(p.dV + r * C, C, lane);
}

}  // namespace dcf
