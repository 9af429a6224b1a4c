// Backward of the sliding-window attention core (k_local_attn, attn.hip; MaskedMHA local branch, blocks.py:204-325, 357-373).
//
// Per sequence b, head h, query row t, half = window / 2, scale = d^-1/4 on q and on k:
//   s_tj = (scale q_t) . (scale k_j) + pen_j   for |j - t| <= half, 0 <= j < T;   pen_j = -1e4 at a padded key, else 0
//   p_t. = softmax_j s_tj,  O_t = sum_j p_tj v_j;   a padded QUERY row has p_t. = 0, O_t = 0
//   dP_tj = dO_t . v_j,  delta_t = sum_j p_tj dP_tj,  dS_tj = p_tj (dP_tj - delta_t)
//   dV_j = sum_t p_tj dO_t,  dQ_t = scale^2 sum_j dS_tj k_j,  dK_j = scale^2 sum_t dS_tj q_t     (t over the live queries whose band holds j)
//
// Two kernels, both with the forward's data layout (a wave owns a row, a lane owns 4 consecutive channels of each 256-channel
// chunk, a head is a group of d / 4 adjacent lanes, dot products are a 4-term partial + DPP adds inside the group):
//   k_attn_bwd_q  : a wave per QUERY row.  Pass 1 walks the window's K / V rows: scores and dP, the softmax statistics carried online
//                   (running maximum m, running sum l, running sum of e * dP); it leaves (m, 1 / l, delta) per (row, head) in scratch.
//                   Pass 2 walks the K rows again: p = exp(s - m) / l, dS, dQ.  Windows of at most 9 / 19 keys are unrolled with the
//                   scores and dP kept in registers and the rows requested two keys ahead; wider windows loop and recompute.
//   k_attn_bwd_kv : a wave per KEY row j: a gather over the at most `window` queries whose band holds j -- q_t, dO_t and the three
//                   statistics of row t, the same score and dP expressions (bit for bit: dotp of grad_common.h pins the contraction), dK and dV
//                   accumulated in registers in ascending t and written once.  No atomics, one fixed summation order.
// delta is formed from p and dP (not from a stored O): with one key in the window p = 1 and delta = dP exactly, hence dS = 0 exactly.
// m and 1 / l are kept apart (not as one log-sum-exp): exp(s - m) / l is the forward's own p, without the rounding of m + log l.
//
// Arithmetic: fp32 on the vector ALU.  The kernels move 2 (query side: 2 w + 2, re-read from L1) rows of C floats per key through the
// vector-memory path and do ~10 flops per loaded float: like the forward they are bound by that path, not by the ALU.
#include "attn_grad.h"

#include "grad_common.h"

namespace dcf {

template <int LPH>
__device__ __forceinline__ float ag_head_sum(float v) {
  if constexpr (LPH == 1) return v;
  else return group_sum<LPH>(v);
}

template <int NCH>
__device__ __forceinline__ void scale_row(Row<NCH>& r, float s) {
#pragma unroll
  for (int j = 0; j < NCH; ++j) r.v[j] *= s;
}

// ------------------------------------------------------------------------------------------
// query side: statistics and dQ
// ------------------------------------------------------------------------------------------
template <int NCH, int LPH, int WMAX>
__global__ __launch_bounds__(256) void k_attn_bwd_q(LocalAttnGradArgs p) {
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
  const float scale = 1.0f / sqrtf(sqrtf((float)(C / p.heads)));
  unsigned long long km = ~0ull;                         // validity of the window's keys: lane l <-> key lo + l, one ballot
  if constexpr (WMAX > 0) {
    if (p.mask) km = __ballot(lane < n && p.mask[base + lo + lane] != 0);
  }
  Row<NCH> q, g, dq;
  q.load(p.Q + r * C, C, lane);
  g.load(p.dO + r * C, C, lane);
  scale_row(q, scale);
  dq.zero();
  float m[NCH], l[NCH], D[NCH];
#pragma unroll
  for (int j = 0; j < NCH; ++j) { m[j] = -INFINITY; l[j] = 0.f; D[j] = 0.f; }

  auto score = [&](const Row<NCH>& k, const Row<NCH>& v, bool valid, float* s, float* dp) __attribute__((always_inline)) {
    const float pen = valid ? 0.f : -1e4f;               // padded keys get a finite -1e4 (blocks.py:279)
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      s[j] = ag_head_sum<LPH>(dotp(q.v[j], k.v[j] * scale)) + pen;
      dp[j] = ag_head_sum<LPH>(dotp(g.v[j], v.v[j]));
    }
  };
  auto online = [&](const float* s, const float* dp) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      const float mn = fmaxf(m[j], s[j]);
      const float corr = m[j] == -INFINITY ? 0.f : exp_res(m[j] - mn);
      const float e = exp_res(s[j] - mn);
      l[j] = l[j] * corr + e;
      D[j] = D[j] * corr + e * dp[j];
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
        *reinterpret_cast<f32x4*>(p.stats + (r * p.heads + (64 * j + lane) / LPH) * 4) = f32x4{m[j], il[j], delta[j], 0.f};
    }
  };
  auto accum = [&](const float* s, const float* dp, const Row<NCH>& k) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      const float pj = exp_res(s[j] - m[j]) * il[j];
      const float ds = pj * (dp[j] - delta[j]);
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
        online(s[i], dp[i]);
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
        if (i < n) accum(s[i], dp[i], kb[i & 1]);
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
      online(s, dp);
    }
    finish();
    if (p.dQ) {
      for (int u = lo; u <= hi; ++u) {                   // the same expressions on the same operands: the same s and dP
        k.load(p.K + (base + u) * C, C, lane);
        v.load(p.V + (base + u) * C, C, lane);
        score(k, v, !p.mask || p.mask[base + u] != 0, s, dp);
        accum(s, dp, k);
      }
    }
  }
  if (p.dQ) {
    scale_row(dq, scale);
    dq.store(p.dQ + r * C, C, lane);
  }
}

// ------------------------------------------------------------------------------------------
// key side: dK and dV as a gather over the queries whose band holds the key
// ------------------------------------------------------------------------------------------
template <int NCH, int LPH, int WMAX>
__global__ __launch_bounds__(256) void k_attn_bwd_kv(LocalAttnGradArgs p) {
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
  auto query = [&](const Row<NCH>& q, const Row<NCH>& g, const f32x4* st) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      const f32x4 qs = q.v[j] * scale;
      const float s = ag_head_sum<LPH>(dotp(qs, k.v[j])) + pen;
      const float pj = exp_res(s - st[j].x) * st[j].y;
      dv.v[j] += pj * g.v[j];
      if (want_dk) {
        const float dp = ag_head_sum<LPH>(dotp(g.v[j], v.v[j]));
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
      if (i < n && ((qm >> i) & 1ull)) query(qb[i & 1], gb[i & 1], sb[i & 1]);        // a padded query attends to nothing
      if (i + 2 < WMAX && i + 2 < n) fetch(lo + i + 2, qb[i & 1], gb[i & 1], sb[i & 1]);
    }
  } else {
    Row<NCH> q, g;
    f32x4 st[NCH];
    for (int u = lo; u <= hi; ++u) {
      if (p.mask && p.mask[base + u] == 0) continue;
      fetch(u, q, g, st);
      query(q, g, st);
    }
  }
  if (p.dK) {
    scale_row(dk, scale);
    dk.store(p.dK + r * C, C, lane);
  }
  if (p.dV) dv.store(p.dV + r * C, C, lane);
}

// ------------------------------------------------------------------------------------------
// launcher
// ------------------------------------------------------------------------------------------
// the unrolled variants serve rows of one chunk (C <= 256: every published configuration); wider rows take the loop, whose two to
// four loads per row and lane are in flight together anyway (unrolled, their score registers would not fit beside the rows)
template <int NCH, int LPH, int WMAX>
static void ag_launch(const LocalAttnGradArgs& a, dim3 grid, bool kv, hipStream_t st) {
  hipLaunchKernelGGL((k_attn_bwd_q<NCH, LPH, WMAX>), grid, dim3(256), 0, st, a);
  if (kv) hipLaunchKernelGGL((k_attn_bwd_kv<NCH, LPH, WMAX>), grid, dim3(256), 0, st, a);
}
#define AG_LAUNCH(NCH_, LPH_) do {                                                        \
    if (NCH_ == 1 && a.window <= 9) ag_launch<1, LPH_, 9>(a, grid, kv, st);               \
    else if (NCH_ == 1 && a.window <= 19) ag_launch<1, LPH_, 19>(a, grid, kv, st);        \
    else ag_launch<NCH_, LPH_, 0>(a, grid, kv, st); } while (0)

int launch_local_attn_bwd(const LocalAttnGradArgs& a, hipStream_t st) {
  DCF_CHECK(a.Q && a.K && a.V && a.dO, "local attention backward: null operand");
  DCF_CHECK(a.B > 0 && a.T > 0 && a.heads > 0, "local attention backward: empty batch (B=%d T=%d heads=%d)", a.B, a.T, a.heads);
  DCF_CHECK(a.window != 0, "local attention backward: window = 0 (global attention) has no backward");
  DCF_CHECK(a.window >= 1 && a.window % 2 == 1, "local attention backward: window = %d must be odd and >= 1", a.window);
  DCF_CHECK(a.C > 0 && a.C % a.heads == 0, "local attention backward: C=%d not divisible by heads=%d", a.C, a.heads);
  const int d = a.C / a.heads, nch = (a.C + 255) / 256, lph = d / 4;
  DCF_CHECK(a.C % 4 == 0 && nch <= 4 && d >= 4 && d <= 256 && (d & (d - 1)) == 0,
            "local attention backward: unsupported C=%d / head dim=%d (need power-of-two head dim in [4,256], C<=1024)", a.C, d);
  const int64_t rows = (int64_t)a.B * a.T;
  DCF_CHECK(rows < (1ll << 31) - 64, "local attention backward: %lld rows (< 2^31)", (long long)rows);
  const bool kv = a.dK || a.dV;
  DCF_CHECK(!kv || a.stats, "local attention backward: dK / dV need the row statistics scratch");
  if (!a.dQ && !kv) return 0;
  const dim3 grid((unsigned)((rows + 3) / 4));           // four waves per workgroup, a wave per row
  bool ok = true;
  switch (nch * 100 + lph) {                             // the forward's table (DISPATCH_ATTN, attn.hip)
    case 101: AG_LAUNCH(1, 1); break;
    case 102: AG_LAUNCH(1, 2); break;
    case 104: AG_LAUNCH(1, 4); break;
    case 108: AG_LAUNCH(1, 8); break;
    case 116: AG_LAUNCH(1, 16); break;
    case 132: AG_LAUNCH(1, 32); break;
    case 164: AG_LAUNCH(1, 64); break;
    case 208: AG_LAUNCH(2, 8); break;
    case 216: AG_LAUNCH(2, 16); break;
    case 232: AG_LAUNCH(2, 32); break;
    case 264: AG_LAUNCH(2, 64); break;
    case 316: AG_LAUNCH(3, 16); break;
    case 332: AG_LAUNCH(3, 32); break;
    case 364: AG_LAUNCH(3, 64); break;
    case 416: AG_LAUNCH(4, 16); break;
    case 432: AG_LAUNCH(4, 32); break;
    case 464: AG_LAUNCH(4, 64); break;
    default: ok = false;
  }
  DCF_CHECK(ok, "local attention backward: no kernel for C=%d heads=%d", a.C, a.heads);
  DCF_HIP(hipGetLastError());
  return 0;
}

}  // namespace dcf
