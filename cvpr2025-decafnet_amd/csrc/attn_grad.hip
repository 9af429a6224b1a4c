// Backward of the sliding-window attention core (k_local_attn, attn.hip; MaskedMHA local branch, blocks.py:204-325, 357-373).
//
// Per sequence b, head h, query row t, half = window / 2, scale = d^-1/4 on q and on k:
//   s_tj = (scale q_t) . (scale k_j) + pen_j   for |j - t| <= half, 0 <= j < T;   pen_j = -1e4 at a padded key, else 0
//   p_t. = softmax_j s_tj,  O_t = sum_j p_tj v_j;   a padded QUERY row has p_t. = 0, O_t = 0
//   dP_tj = dO_t . v_j,  delta_t = sum_j p_tj dP_tj,  dS_tj = p_tj (dP_tj - delta_t)
//   dV_j = sum_t p_tj dO_t,  dQ_t = scale^2 sum_j dS_tj k_j,  dK_j = scale^2 sum_t dS_tj q_t     (t over the live queries whose band holds j)
//
// Two kernels (local_attn_kernels.h, instantiated here), both with the forward's data layout (a wave owns a row, a lane owns 4 consecutive channels of each 256-channel
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
#include "local_attn_kernels.h"        // k_attn_bwd_q, k_attn_bwd_kv, the table of row shapes

namespace dcf {

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

int local_attn_geometry_check(const char* who, int B, int T, int C, int heads, int window, const char* window0) {
  DCF_CHECK(B > 0 && T > 0 && heads > 0, "%s: empty batch (B=%d T=%d heads=%d)", who, B, T, heads);
  DCF_CHECK(window != 0, "%s: window = 0 (global attention) %s", who, window0);
  DCF_CHECK(window >= 1 && window % 2 == 1, "%s: window = %d must be odd and >= 1", who, window);
  DCF_CHECK(C > 0 && C % heads == 0, "%s: C=%d not divisible by heads=%d", who, C, heads);
  const int d = C / heads, nch = (C + 255) / 256;
  DCF_CHECK(C % 4 == 0 && nch <= 4 && d >= 4 && d <= 256 && (d & (d - 1)) == 0,
            "%s: unsupported C=%d / head dim=%d (need power-of-two head dim in [4,256], C<=1024)", who, C, d);
  DCF_CHECK((int64_t)B * T < (1ll << 31) - 64, "%s: %lld rows (< 2^31)", who, (long long)B * T);
  return 0;
}

int launch_local_attn_bwd(const LocalAttnGradArgs& a, hipStream_t st) {
  const char* who = "local attention backward";
  DCF_CHECK(a.Q && a.K && a.V && a.dO, "%s: null operand", who);
  if (local_attn_geometry_check(who, a.B, a.T, a.C, a.heads, a.window, "has no backward")) return -1;
  const int nch = (a.C + 255) / 256, lph = a.C / a.heads / 4;
  const bool kv = a.dK || a.dV;
  DCF_CHECK(!kv || a.stats, "%s: dK / dV need the row statistics scratch", who);
  if (!a.dQ && !kv) return 0;
  const dim3 grid((unsigned)(((int64_t)a.B * a.T + 3) / 4));       // four waves per workgroup, a wave per row
  bool ok = true;
  DCF_ATTN_ROW_SHAPES(nch, lph, ok, AG_LAUNCH);
  DCF_CHECK(ok, "%s: no kernel for C=%d heads=%d", who, a.C, a.heads);
  DCF_HIP(hipGetLastError());
  return 0;
}

}  // namespace dcf
