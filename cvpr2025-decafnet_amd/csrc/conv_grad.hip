// Backward of MaskedConv1D (dense, k = 1 / 3, libs/modeling/blocks.py:87-106) and of the channel LayerNorm (blocks.py:125-131) on
// token-major (B*T, C) fp32 rows -- the two operators every differentiable block of the network is built from.
//
//   forward      Y[b,t,n]  = bias[n] + sum_j sum_c W[n,c,j] m[b,t+j-p] X[b,t+j-p,c]       (taps stay inside sequence b; Y is not masked)
//   weight grad  dW[n,c,j] = sum_{b,t} dY[b,t,n] m X[b,t+j-p,c],   db[n] = sum dY[b,t,n]
//   data grad    dX[b,t,c] = m[b,t] sum_j sum_n dY[b,t-j+p,n] W[n,c,j]
//
// Weight gradient (k_wgrad): a GEMM whose reduction dimension is the ROWS (tens of thousands) and whose output is only N x kC, on
// v_mfma_f32_32x32x16_f16 with both operands split into two fp16 planes (hi + lo, three products: the f16x3 arithmetic of
// gemm_bf16s.hip).  Neither operand is a weight, so neither has a pre-split image: a thread reads 8 consecutive rows of ONE column
// (a wave reads 64 adjacent columns of a row: 256 B per request), splits them and writes them to LDS as one 16-byte vector per
// plane -- the k-contiguous layout an MFMA operand wants, i.e. the transposition happens in the registers.  The three taps are the
// same X rows shifted by +-1: the thread reads its 8 rows and a one-row rim (10 loads, converted once) and writes the three
// shifted, seam-gated vectors; X is read from memory once.  A workgroup owns a 64 (n) x 64 (c) x k tile of the output and one
// slice of the rows; its fp32 partial goes to scratch and k_cg_reduce adds the slices in a fixed order (blocked_sum, grad_common.h; no
// floating-point atomics: bit-identical from run to run).  db rides along: the threads that staged dY add up what they staged.
//
// Range of dY.  The forward pre-scales activations by a fixed 2^4 because their range is structural; a gradient has no such bound
// (after 1 / loss_norm it is routinely 1e-6 and below, where fp16 planes lose bits or flush).  k_absmax reduces max |dY| into a
// device word (an integer max of the bit patterns: order independent), every kernel derives the power of two of conv_grad.h from
// that word on the device -- no host wait -- and k_cg_reduce / k_dx_finish undo it.  Powers of two commute with every rounding
// here, so dY, 2^-30 dY and 2^10 dY give the same bits up to that factor.  A non-finite sum raises the sticky word of this file,
// which the NEXT call of one of the three exports reports (a -1 return with a message); the values themselves stay non-finite.
//
// Data gradient: the forward's tap-3 row GEMM (launch_gemm_split, A_ROWS_TAP3) on dY with the weight image permuted to
// Wp[c][tap][n] = W[n][c][k-1-tap]; neighbour flags from the sequence ends alone (dY at a padded row is a legitimate operand);
// dY is scaled into a scratch copy first and k_dx_finish multiplies the result by the row mask and the inverse scale.
// N = 1, 2 (the heads' output convolutions) is vector-ALU work in both directions (k_wgrad_small, k_dgrad_small).
//
// LayerNorm backward (k_ln_bwd): a wave owns a run of rows, keeps x and dOut of a row in registers (one read of each, one write of
// dX), recomputes mean / rstd two-pass exactly like row_layernorm, masks by the recomputed output (out > 0) and accumulates
// dw = sum dy xhat, db = sum dy per lane; workgroup partials, fixed-order final sum.
//
// k = 5 / stride 2 / padding 2 (the embedding convolutions of vid_net.stride > 1, video_net.py:62-70; T even, To = T / 2, no bias):
//
//   forward      Y[b,u,n]  = sum_{j<5} sum_c W[n,c,j] m[b,2u+j-2] X[b,2u+j-2,c]
//   weight grad  dW[n,c,j] = sum_{b,u} dY[b,u,n] m X[b,2u+j-2,c]
//   data grad    dX[b,t,c] = m[b,t] sum_{j = t (mod 2), 0 <= (t+2-j)/2 < To} sum_n dY[b,(t+2-j)/2,n] W[n,c,j]
//
// dcf_op_conv5s2_split is the forward's own path (launch_im2col5s2 into a scratch, then the split GEMM on K = 5 Cin).  The weight
// gradient (k_wgrad5) is k_wgrad's scheme with the reduction over the OUTPUT rows: because T = 2 To, output row r of the flattened
// batch reads input rows 2 r - 2 .. 2 r + 2, so a thread that stages output rows r .. r + 7 reads input rows 2 r - 2 .. 2 r + 16 of its
// column once (19 loads, converted once) and writes five seam- and mask-gated vectors per plane.  LDS per workgroup: dY 2 planes x 64
// columns x WG_PITCH halfs = 10 240 B, X 5 taps x 2 planes x 64 x WG_PITCH halfs = 51 200 B, 61 440 B in all (k = 3: 41 984 B with
// the bias sums): LDS alone admits two workgroups per CU of 160 KiB where k = 3 has three, but the five accumulators and the 19-row
// staging take 276 registers (no spills), one wave per SIMD: one workgroup per CU is resident; every 16-byte vector stays aligned
// because the tap and plane strides are multiples of 64 * WG_PITCH halfs = 5 120 B and a row run starts at a multiple of 8 halfs.
// The data gradient splits the input rows by parity: even rows 2 u take taps 4, 2, 0 of the output rows u - 1, u, u + 1 and odd rows
// 2 u + 1 take taps 3, 1 of u, u + 1 -- two tap-3 row GEMMs on dY itself (one launch, count = 2), each writing every other row of dX
// (row pitch 2 Cin); the odd one carries a zero image for its first tap, because the row GEMM has three taps: 6 taps of work for 5.
#include <mutex>
#include "../../include/decafnet_hip.h"
#include "conv_grad.h"
#include "grad_common.h"
#include "gemm.h"
#include "rowops.h"

namespace dcf {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

__global__ __launch_bounds__(256) void k_absmax(const float* __restrict__ x, int64_t n, unsigned* __restrict__ word) {
  unsigned m = 0u;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const unsigned b = __float_as_uint(x[i]) & 0x7fffffffu;
    m = b > m ? b : m;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned t = (unsigned)__shfl_xor((int)m, o);
    m = t > m ? t : m;
  }
  if ((threadIdx.x & 63) == 0 && m) atomicMax(word, m);       // integer max: the result does not depend on the order
}

// bit0 = row valid (mask; all rows when mask is null or self_always), bit1 / bit2 = a left / right neighbour exists in the sequence
__global__ void k_seqflags(const uint8_t* __restrict__ mask, uint8_t* __restrict__ out, int T, int rows, int self_always) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const int t = r % T;
  unsigned f = (self_always || !mask || mask[r]) ? 1u : 0u;
  if (t > 0) f |= 2u;
  if (t < T - 1) f |= 4u;
  out[r] = (uint8_t)f;
}

// ------------------------------------------------------------------------------------------
// weight gradient on the matrix cores
// ------------------------------------------------------------------------------------------
constexpr int WG_ROWS = 32;      // reduction rows per LDS chunk (two k-steps of 16)
constexpr int WG_PITCH = 40;     // halfs per (plane, column): 32 rows + 8 pad = 80 B, keeps every 16-byte vector aligned
constexpr float WG_SX = 16.f;    // activation pre-scale of the forward (gemm_bf16s.hip F16_SA)

template <int KT>
__global__ __launch_bounds__(256) void k_wgrad(ConvGradArgs p) {
  constexpr int XN = KT == 3 ? 10 : 8;       // rows a thread reads of its X column per chunk (8 + the rim)
  constexpr int RIM = KT == 3 ? 1 : 0;
  __shared__ __attribute__((aligned(16))) _Float16 s_dy[2 * 64 * WG_PITCH];
  __shared__ __attribute__((aligned(16))) _Float16 s_x[KT * 2 * 64 * WG_PITCH];
  __shared__ float s_db[4 * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tiles_c = (p.Cin + 63) / 64;
  const int tn = blockIdx.x / tiles_c, tc = blockIdx.x - tn * tiles_c;
  const int slice = blockIdx.y;
  const int r_begin = slice * p.slice_rows;
  const int r_end = r_begin + p.slice_rows < p.rows ? r_begin + p.slice_rows : p.rows;
  float inv;
  const float s = cg_scale(*p.absmax, inv);
  const int n_g = tn * 64 + lane, c_g = tc * 64 + lane;
  const bool n_ok = n_g < p.N, c_ok = c_g < p.Cin;
  const float* __restrict__ dyp = p.dY + n_g;
  const float* __restrict__ xp = p.X + c_g;
  const uint8_t* __restrict__ flags = p.flags;
  const int N = p.N, Cin = p.Cin, rows = p.rows;

  float dyv[8], xv[XN];
  unsigned fl[XN];
  auto load = [&](int r0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int r = r0 + i;
      dyv[i] = (n_ok && r < r_end) ? dyp[(int64_t)r * N] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < XN; ++i) {
      const int q = r0 + i - RIM;
      const unsigned f = (q >= 0 && q < rows) ? (unsigned)flags[q] : 0u;
      fl[i] = f;
      xv[i] = (c_ok && (f & 1u)) ? xp[(int64_t)q * Cin] : 0.f;
    }
  };

  const int h = lane >> 5, r32 = lane & 31;
  const int wn = wave & 1, wc = wave >> 1;
  const bool active = tn * 64 + wn * 32 < N && tc * 64 + wc * 32 < Cin;      // (N, Cin are multiples of 32: a 32-block is whole or absent)
  f32x16 acc[KT];
#pragma unroll
  for (int j = 0; j < KT; ++j)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
  float dbacc = 0.f;

  load(r_begin + wave * 8);
  for (int r0 = r_begin; r0 < r_end; r0 += WG_ROWS) {
    {  // registers -> LDS: split into (hi, lo) fp16 planes, 8 consecutive rows of this thread's column = one 16-byte vector
      f16x8 dh, dl;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float v = dyv[i] * s;
        dbacc += v;
        const _Float16 hi = (_Float16)v;
        dh[i] = hi;
        dl[i] = (_Float16)(v - (float)hi);
      }
      *reinterpret_cast<f16x8*>(&s_dy[(0 * 64 + lane) * WG_PITCH + wave * 8]) = dh;
      *reinterpret_cast<f16x8*>(&s_dy[(1 * 64 + lane) * WG_PITCH + wave * 8]) = dl;
      _Float16 xh[XN], xl[XN];
#pragma unroll
      for (int i = 0; i < XN; ++i) {
        const _Float16 hi = (_Float16)(xv[i] * WG_SX);
        xh[i] = hi;
        xl[i] = (_Float16)__builtin_fmaf(xv[i], WG_SX, -(float)hi);
      }
#pragma unroll
      for (int j = 0; j < KT; ++j) {
        f16x8 th, tl;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          // tap j of row r0 + i reads row r0 + i + j - p: usable if that neighbour lies in the same sequence (its mask is in xv)
          bool ok = true;
          if (KT == 3 && j == 0) ok = (fl[i + RIM] & 2u) != 0u;
          if (KT == 3 && j == 2) ok = (fl[i + RIM] & 4u) != 0u;
          th[i] = ok ? xh[i + j] : (_Float16)0.f;
          tl[i] = ok ? xl[i + j] : (_Float16)0.f;
        }
        *reinterpret_cast<f16x8*>(&s_x[((j * 2 + 0) * 64 + lane) * WG_PITCH + wave * 8]) = th;
        *reinterpret_cast<f16x8*>(&s_x[((j * 2 + 1) * 64 + lane) * WG_PITCH + wave * 8]) = tl;
      }
    }
    __syncthreads();
    if (r0 + WG_ROWS < r_end) load(r0 + WG_ROWS + wave * 8);      // the next chunk travels while this one is multiplied
    if (active) {
#pragma unroll
      for (int ks = 0; ks < WG_ROWS / 16; ++ks) {
        const int ko = ks * 16 + h * 8;
        const f16x8 a_hi = *reinterpret_cast<const f16x8*>(&s_dy[(0 * 64 + wn * 32 + r32) * WG_PITCH + ko]);
        const f16x8 a_lo = *reinterpret_cast<const f16x8*>(&s_dy[(1 * 64 + wn * 32 + r32) * WG_PITCH + ko]);
#pragma unroll
        for (int j = 0; j < KT; ++j) {
          const f16x8 b_hi = *reinterpret_cast<const f16x8*>(&s_x[((j * 2 + 0) * 64 + wc * 32 + r32) * WG_PITCH + ko]);
          const f16x8 b_lo = *reinterpret_cast<const f16x8*>(&s_x[((j * 2 + 1) * 64 + wc * 32 + r32) * WG_PITCH + ko]);
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_lo, b_hi, acc[j], 0, 0, 0);
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, b_lo, acc[j], 0, 0, 0);
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, b_hi, acc[j], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }

  if (active) {
    // accumulator element e of lane (h, r32): n = 4 h + (e & 3) + 8 (e >> 2), c = r32 of this wave's 32 x 32 block
    const int c = tc * 64 + wc * 32 + r32;
#pragma unroll
    for (int j = 0; j < KT; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int n = tn * 64 + wn * 32 + 4 * h + (e & 3) + 8 * (e >> 2);
        p.part[(((int64_t)slice * N + n) * KT + j) * Cin + c] = acc[j][e];
      }
  }
  if (p.dbpart && tc == 0) {         // (uniform per workgroup)
    s_db[wave * 64 + lane] = dbacc;
    __syncthreads();
    if (tid < 64 && n_ok) p.dbpart[(int64_t)slice * N + n_g] = (s_db[lane] + s_db[64 + lane]) + (s_db[128 + lane] + s_db[192 + lane]);
  }
}

// k = 5 / stride 2: the reduction runs over the output rows of the flattened batch (rows = B * To); output row r reads input rows
// 2 r + j - 2 (T = 2 To).  flags (per OUTPUT row): bit1 = an output row to the left exists in the sequence (taps 0, 1 stay inside),
// bit2 = one to the right (tap 4 stays inside).  mask (per INPUT row) may be null.
__global__ __launch_bounds__(256) void k_wgrad5(ConvGradArgs p, const uint8_t* __restrict__ mask) {
  constexpr int KT = 5, XN = 19;             // input rows 2 r0 - 2 .. 2 r0 + 16 for output rows r0 .. r0 + 7
  __shared__ __attribute__((aligned(16))) _Float16 s_dy[2 * 64 * WG_PITCH];
  __shared__ __attribute__((aligned(16))) _Float16 s_x[KT * 2 * 64 * WG_PITCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tiles_c = (p.Cin + 63) / 64;
  const int tn = blockIdx.x / tiles_c, tc = blockIdx.x - tn * tiles_c;
  const int slice = blockIdx.y;
  const int r_begin = slice * p.slice_rows;
  const int r_end = r_begin + p.slice_rows < p.rows ? r_begin + p.slice_rows : p.rows;
  float inv;
  const float s = cg_scale(*p.absmax, inv);
  const int n_g = tn * 64 + lane, c_g = tc * 64 + lane;
  const bool n_ok = n_g < p.N, c_ok = c_g < p.Cin;
  const float* __restrict__ dyp = p.dY + n_g;
  const float* __restrict__ xp = p.X + c_g;
  const uint8_t* __restrict__ flags = p.flags;
  const int N = p.N, Cin = p.Cin, rows = p.rows;
  const int64_t rows_in = 2 * (int64_t)rows;

  float dyv[8], xv[XN];
  unsigned fl[8];
  auto load = [&](int r0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int r = r0 + i;
      const bool ok = r < r_end;
      dyv[i] = (n_ok && ok) ? dyp[(int64_t)r * N] : 0.f;
      fl[i] = ok ? (unsigned)flags[r] : 0u;
    }
#pragma unroll
    for (int i = 0; i < XN; ++i) {
      const int64_t q = 2 * (int64_t)r0 - 2 + i;
      const bool ok = c_ok && q >= 0 && q < rows_in && (!mask || mask[q]);
      xv[i] = ok ? xp[q * Cin] : 0.f;
    }
  };

  const int h = lane >> 5, r32 = lane & 31;
  const int wn = wave & 1, wc = wave >> 1;
  const bool active = tn * 64 + wn * 32 < N && tc * 64 + wc * 32 < Cin;
  f32x16 acc[KT];
#pragma unroll
  for (int j = 0; j < KT; ++j)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;

  load(r_begin + wave * 8);
  for (int r0 = r_begin; r0 < r_end; r0 += WG_ROWS) {
    {
      f16x8 dh, dl;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float v = dyv[i] * s;
        const _Float16 hi = (_Float16)v;
        dh[i] = hi;
        dl[i] = (_Float16)(v - (float)hi);
      }
      *reinterpret_cast<f16x8*>(&s_dy[(0 * 64 + lane) * WG_PITCH + wave * 8]) = dh;
      *reinterpret_cast<f16x8*>(&s_dy[(1 * 64 + lane) * WG_PITCH + wave * 8]) = dl;
      _Float16 xh[XN], xl[XN];
#pragma unroll
      for (int i = 0; i < XN; ++i) {
        const _Float16 hi = (_Float16)(xv[i] * WG_SX);
        xh[i] = hi;
        xl[i] = (_Float16)__builtin_fmaf(xv[i], WG_SX, -(float)hi);
      }
#pragma unroll
      for (int j = 0; j < KT; ++j) {
        f16x8 th, tl;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          // tap j of output row r0 + i reads input row 2 (r0 + i) + j - 2 = xv[2 i + j]: inside the sequence for j = 2, 3 always,
          // for j = 0, 1 if an output row to the left exists, for j = 4 if one to the right does (the mask is in xv)
          bool ok = true;
          if (j < 2) ok = (fl[i] & 2u) != 0u;
          if (j == 4) ok = (fl[i] & 4u) != 0u;
          th[i] = ok ? xh[2 * i + j] : (_Float16)0.f;
          tl[i] = ok ? xl[2 * i + j] : (_Float16)0.f;
        }
        *reinterpret_cast<f16x8*>(&s_x[((j * 2 + 0) * 64 + lane) * WG_PITCH + wave * 8]) = th;
        *reinterpret_cast<f16x8*>(&s_x[((j * 2 + 1) * 64 + lane) * WG_PITCH + wave * 8]) = tl;
      }
    }
    __syncthreads();
    if (r0 + WG_ROWS < r_end) load(r0 + WG_ROWS + wave * 8);
    if (active) {
#pragma unroll
      for (int ks = 0; ks < WG_ROWS / 16; ++ks) {
        const int ko = ks * 16 + h * 8;
        const f16x8 a_hi = *reinterpret_cast<const f16x8*>(&s_dy[(0 * 64 + wn * 32 + r32) * WG_PITCH + ko]);
        const f16x8 a_lo = *reinterpret_cast<const f16x8*>(&s_dy[(1 * 64 + wn * 32 + r32) * WG_PITCH + ko]);
#pragma unroll
        for (int j = 0; j < KT; ++j) {
          const f16x8 b_hi = *reinterpret_cast<const f16x8*>(&s_x[((j * 2 + 0) * 64 + wc * 32 + r32) * WG_PITCH + ko]);
          const f16x8 b_lo = *reinterpret_cast<const f16x8*>(&s_x[((j * 2 + 1) * 64 + wc * 32 + r32) * WG_PITCH + ko]);
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_lo, b_hi, acc[j], 0, 0, 0);
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, b_lo, acc[j], 0, 0, 0);
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, b_hi, acc[j], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }

  if (active) {
    const int c = tc * 64 + wc * 32 + r32;
#pragma unroll
    for (int j = 0; j < KT; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int n = tn * 64 + wn * 32 + 4 * h + (e & 3) + 8 * (e >> 2);
        p.part[(((int64_t)slice * N + n) * KT + j) * Cin + c] = acc[j][e];
      }
  }
}

// N = 1, 2: one wave per (64 channels, row slice); a lane owns a channel and slides a 3-row window of its column through registers
template <int KT, int NO>
__global__ __launch_bounds__(64) void k_wgrad_small(ConvGradArgs p) {
  const int lane = threadIdx.x, c = blockIdx.x * 64 + lane, slice = blockIdx.y;
  const bool c_ok = c < p.Cin;
  const int r_begin = slice * p.slice_rows;
  const int r_end = r_begin + p.slice_rows < p.rows ? r_begin + p.slice_rows : p.rows;
  float inv;
  const float s = cg_scale(*p.absmax, inv);
  const float* __restrict__ xp = p.X + (c_ok ? c : 0);
  const int Cin = p.Cin, rows = p.rows;
  auto xrow = [&](int q) -> float {
    if (q < 0 || q >= rows) return 0.f;
    return (p.flags[q] & 1u) ? xp[(int64_t)q * Cin] : 0.f;
  };
  float acc[NO][KT], db[NO];
#pragma unroll
  for (int n = 0; n < NO; ++n) {
    db[n] = 0.f;
#pragma unroll
    for (int j = 0; j < KT; ++j) acc[n][j] = 0.f;
  }
  float xl = KT == 3 ? xrow(r_begin - 1) : 0.f, xc = xrow(r_begin);
  for (int r = r_begin; r < r_end; ++r) {
    const float xr = KT == 3 ? xrow(r + 1) : 0.f;
    const unsigned f = p.flags[r];
#pragma unroll
    for (int n = 0; n < NO; ++n) {
      const float d = p.dY[(int64_t)r * NO + n] * s;
      db[n] += d;
      if (KT == 3) {
        acc[n][0] = __builtin_fmaf(d, (f & 2u) ? xl : 0.f, acc[n][0]);
        acc[n][1] = __builtin_fmaf(d, xc, acc[n][1]);
        acc[n][2] = __builtin_fmaf(d, (f & 4u) ? xr : 0.f, acc[n][2]);
      } else {
        acc[n][0] = __builtin_fmaf(d, xc, acc[n][0]);
      }
    }
    xl = xc; xc = xr;
    if (KT == 1 && r + 1 < r_end) xc = xrow(r + 1);
  }
  if (c_ok) {
#pragma unroll
    for (int n = 0; n < NO; ++n)
#pragma unroll
      for (int j = 0; j < KT; ++j) p.part[(((int64_t)slice * NO + n) * KT + j) * Cin + c] = acc[n][j];
  }
  if (p.dbpart && blockIdx.x == 0 && lane < NO) {
    float v = db[0];
#pragma unroll
    for (int n = 1; n < NO; ++n) v = lane == n ? db[n] : v;
    p.dbpart[(int64_t)slice * NO + lane] = v;
  }
}

// out[o(i)] (+)= extra * inv_scale * sum_s part[s][i], s in order.  KT > 1: part is laid out [n][j][c], out is PyTorch's [n][c][j].
__global__ __launch_bounds__(256) void k_cg_reduce(const float* __restrict__ part, int nparts, int64_t stride, int count,
                                                   const unsigned* __restrict__ absmax, float extra, float* __restrict__ out, int KT, int C,
                                                   int accumulate, unsigned* __restrict__ status) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  float sum = 0.f;
  DCF_BLOCKED_SUM(sum, part, nparts, stride, i);
  float inv = 1.f;
  if (absmax) (void)cg_scale(*absmax, inv);
  const float v = (sum * extra) * inv;
  if (!(__builtin_fabsf(v) <= 3.4028234664e38f)) atomicOr(status, 1u);
  int o = i;
  if (KT > 1) {
    const int n = i / (KT * C), rem = i - n * KT * C, j = rem / C, c = rem - j * C;
    o = (n * C + c) * KT + j;
  }
  out[o] = accumulate ? out[o] + v : v;
}

// ------------------------------------------------------------------------------------------
// data gradient
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_scale_copy(const float* __restrict__ x, float* __restrict__ y, int64_t n, const unsigned* __restrict__ absmax) {
  float inv;
  const float s = cg_scale(*absmax, inv);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) y[i] = x[i] * s;
}

// Wp[c][tap][n] = W[n][c][k - 1 - tap]: the forward GEMM's [N_out][tap][cin] weight with the roles of the channels exchanged
__global__ void k_permute_wT(const float* __restrict__ W, float* __restrict__ Wp, int N, int Cin, int k) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * Cin * k) return;
  const int c = i / (k * N), rem = i - c * k * N, tap = rem / N, n = rem - tap * N;
  Wp[i] = W[((int64_t)n * Cin + c) * k + (k - 1 - tap)];
}

// k = 5 / stride 2, data gradient: the weight images of the two row GEMMs, Wp[c][tap][n] (tap 0, 1, 2 = output rows u - 1, u, u + 1).
// parity 0 (input rows 2 u): W[n][c][4 - 2 tap]; parity 1 (rows 2 u + 1): W[n][c][5 - 2 tap], tap 0 has no weight and holds zeros.
__global__ void k_permute_w5T(const float* __restrict__ W, float* __restrict__ Wp, int N, int Cin, int parity) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * Cin * 3) return;
  const int c = i / (3 * N), rem = i - c * 3 * N, tap = rem / N, n = rem - tap * N;
  const int j = 4 + parity - 2 * tap;
  Wp[i] = j < 5 ? W[((int64_t)n * Cin + c) * 5 + j] : 0.f;
}

// forward: Wf[n][j][c] = W[n][c][j], the [N][tap][cin] rows of the forward GEMM
__global__ void k_permute_w5(const float* __restrict__ W, float* __restrict__ Wf, int N, int Cin) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * Cin * 5) return;
  const int n = i / (5 * Cin), rem = i - n * 5 * Cin, j = rem / Cin, c = rem - j * Cin;
  Wf[i] = W[((int64_t)n * Cin + c) * 5 + j];
}

__global__ __launch_bounds__(256) void k_dx_finish(float* __restrict__ dX, const uint8_t* __restrict__ mask, const unsigned* __restrict__ absmax,
                                                   int64_t rows, int C4, unsigned* __restrict__ status) {
  float inv;
  (void)cg_scale(*absmax, inv);
  const int64_t n4 = rows * C4;
  bool bad = false;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / C4;
    const float f = (!mask || mask[r]) ? inv : 0.f;
    f32x4 v = reinterpret_cast<f32x4*>(dX)[i];
    bad |= !(__builtin_fabsf(v.x) <= 3.4028234664e38f) || !(__builtin_fabsf(v.y) <= 3.4028234664e38f) ||
           !(__builtin_fabsf(v.z) <= 3.4028234664e38f) || !(__builtin_fabsf(v.w) <= 3.4028234664e38f);
    v.x *= f; v.y *= f; v.z *= f; v.w *= f;
    reinterpret_cast<f32x4*>(dX)[i] = v;
  }
  if (bad) atomicOr(status, 1u);
}

// N = 1, 2: dX[r][c] = m[r] sum_j sum_n dY[r - j + p][n] W[n][c][j], one thread per element
template <int KT, int NO>
__global__ __launch_bounds__(256) void k_dgrad_small(const float* __restrict__ dY, const uint8_t* __restrict__ flags, const float* __restrict__ W,
                                                     float* __restrict__ dX, int64_t rows, int Cin) {
  const int64_t total = rows * Cin;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / Cin;
    const int c = (int)(i - r * Cin);
    const unsigned f = flags[r];
    float v = 0.f;
    if (f & 1u) {
#pragma unroll
      for (int n = 0; n < NO; ++n) {
        const float* w = W + ((int64_t)n * Cin + c) * KT;
        if (KT == 3) {
          if (f & 4u) v = __builtin_fmaf(dY[(r + 1) * NO + n], w[0], v);
          v = __builtin_fmaf(dY[r * NO + n], w[1], v);
          if (f & 2u) v = __builtin_fmaf(dY[(r - 1) * NO + n], w[2], v);
        } else {
          v = __builtin_fmaf(dY[r * NO + n], w[0], v);
        }
      }
    }
    dX[i] = v;
  }
}

// ------------------------------------------------------------------------------------------
// LayerNorm backward
// ------------------------------------------------------------------------------------------
template <int NCH>
__global__ __launch_bounds__(256) void k_ln_bwd(LnBwdArgs p) {
  extern __shared__ float s_ln[];              // [4 waves][2][C]
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int C = p.C;
  const int64_t r_begin = ((int64_t)blockIdx.x * 4 + wave) * p.rows_per_wave;
  const int64_t r_end = r_begin + p.rows_per_wave < p.rows ? r_begin + p.rows_per_wave : p.rows;
  const float inv_c = 1.0f / (float)C;
  Row<NCH> dw, db;
  dw.zero(); db.zero();
  Row<NCH> xn, gn;
  if (r_begin < r_end) { xn.load(p.X + r_begin * C, C, lane); gn.load(p.dOut + r_begin * C, C, lane); }
  for (int64_t r = r_begin; r < r_end; ++r) {
    Row<NCH> x = xn, g = gn;
    if (r + 1 < r_end) { xn.load(p.X + (r + 1) * C, C, lane); gn.load(p.dOut + (r + 1) * C, C, lane); }
    // mean / rstd exactly as row_layernorm (common.h) computes them
    const float mean = x.sum() * inv_c;
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      if (256 * j + 4 * lane < C) {
        x.v[j].x -= mean; x.v[j].y -= mean; x.v[j].z -= mean; x.v[j].w -= mean;
        sq += (x.v[j].x * x.v[j].x + x.v[j].y * x.v[j].y) + (x.v[j].z * x.v[j].z + x.v[j].w * x.v[j].w);
      }
    }
    const float var = wave_sum(sq) * inv_c;
    const float rs = 1.0f / sqrtf(var + 1e-5f);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      const int c = 256 * j + 4 * lane;
      if (c < C) {
        f32x4 xh = x.v[j];
        xh.x *= rs; xh.y *= rs; xh.z *= rs; xh.w *= rs;
        f32x4 ww = f32x4{1.f, 1.f, 1.f, 1.f}, bb = f32x4{0.f, 0.f, 0.f, 0.f};
        if (p.w) { ww = *reinterpret_cast<const f32x4*>(p.w + c); bb = *reinterpret_cast<const f32x4*>(p.b + c); }
        f32x4 dy = g.v[j];
        if (p.relu) {                       // the forward's output, recomputed: the gradient passes where out > 0
          f32x4 y;
          y.x = xh.x * ww.x + bb.x; y.y = xh.y * ww.y + bb.y; y.z = xh.z * ww.z + bb.z; y.w = xh.w * ww.w + bb.w;
          dy.x = y.x > 0.f ? dy.x : 0.f; dy.y = y.y > 0.f ? dy.y : 0.f; dy.z = y.z > 0.f ? dy.z : 0.f; dy.w = y.w > 0.f ? dy.w : 0.f;
        }
        db.v[j] += dy;
        dw.v[j] += dy * xh;
        const f32x4 dh = dy * ww;           // d / d xhat
        s1 += (dh.x + dh.y) + (dh.z + dh.w);
        s2 += (dh.x * xh.x + dh.y * xh.y) + (dh.z * xh.z + dh.w * xh.w);
        x.v[j] = xh; g.v[j] = dh;
      }
    }
    s1 = wave_sum(s1) * inv_c;
    s2 = wave_sum(s2) * inv_c;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      if (256 * j + 4 * lane < C) {
        const f32x4 xh = x.v[j], dh = g.v[j];
        f32x4 o;
        o.x = rs * ((dh.x - s1) - xh.x * s2); o.y = rs * ((dh.y - s1) - xh.y * s2);
        o.z = rs * ((dh.z - s1) - xh.z * s2); o.w = rs * ((dh.w - s1) - xh.w * s2);
        x.v[j] = o;
      }
    }
    x.store(p.dX + r * C, C, lane);
  }
  if (!p.part) return;
  dw.store(s_ln + (wave * 2 + 0) * C, C, lane);
  db.store(s_ln + (wave * 2 + 1) * C, C, lane);
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * C; i += 256)
    p.part[(int64_t)blockIdx.x * 2 * C + i] = (s_ln[i] + s_ln[2 * C + i]) + (s_ln[4 * C + i] + s_ln[6 * C + i]);
}

// ------------------------------------------------------------------------------------------
// launches
// ------------------------------------------------------------------------------------------
static inline unsigned grid_for(int64_t n, int per_block, unsigned cap) {
  int64_t g = (n + per_block - 1) / per_block;
  return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

int launch_absmax(const float* x, int64_t n, unsigned* word, hipStream_t st) {
  DCF_HIP(hipMemsetAsync(word, 0, sizeof(unsigned), st));
  if (n > 0) hipLaunchKernelGGL(k_absmax, dim3(grid_for(n, 1024, 2048)), dim3(256), 0, st, x, n, word);
  DCF_HIP(hipGetLastError());
  return 0;
}

int launch_wgrad(const ConvGradArgs& a, hipStream_t st) {
  if (a.N <= 2) {
    const dim3 grid((a.Cin + 63) / 64, a.nslices);
    if (a.k == 3 && a.N == 1) hipLaunchKernelGGL((k_wgrad_small<3, 1>), grid, dim3(64), 0, st, a);
    else if (a.k == 3) hipLaunchKernelGGL((k_wgrad_small<3, 2>), grid, dim3(64), 0, st, a);
    else if (a.N == 1) hipLaunchKernelGGL((k_wgrad_small<1, 1>), grid, dim3(64), 0, st, a);
    else hipLaunchKernelGGL((k_wgrad_small<1, 2>), grid, dim3(64), 0, st, a);
  } else {
    const dim3 grid(((a.N + 63) / 64) * ((a.Cin + 63) / 64), a.nslices);
    if (a.k == 3) hipLaunchKernelGGL(k_wgrad<3>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_wgrad<1>, grid, dim3(256), 0, st, a);
  }
  DCF_HIP(hipGetLastError());
  return 0;
}

int launch_ln_bwd(const LnBwdArgs& a, int nwg, hipStream_t st) {
  const size_t lds = a.part ? (size_t)8 * a.C * sizeof(float) : 0;
  const int nch = (a.C + 255) / 256;
  if (nch == 1) hipLaunchKernelGGL(k_ln_bwd<1>, dim3(nwg), dim3(256), lds, st, a);
  else if (nch == 2) hipLaunchKernelGGL(k_ln_bwd<2>, dim3(nwg), dim3(256), lds, st, a);
  else if (nch == 3) hipLaunchKernelGGL(k_ln_bwd<3>, dim3(nwg), dim3(256), lds, st, a);
  else hipLaunchKernelGGL(k_ln_bwd<4>, dim3(nwg), dim3(256), lds, st, a);
  DCF_HIP(hipGetLastError());
  return 0;
}

// The sticky numerics word of the three exports: a device word the reduce / finish kernels raise, mirrored into pinned host
// memory by a copy queued at the end of every call; the next call reads the mirror without waiting on anything.
struct CgStatus {
  unsigned* dev = nullptr;
  volatile unsigned* host = nullptr;
  const void* guard = nullptr;          // the dcf_guard_state a step guard armed (include/decafnet_hip_guard.h), or nullptr
};
static CgStatus g_cg;
static std::mutex g_cg_mu;

static int cg_alloc() {                 // under g_cg_mu
  if (g_cg.dev) return 0;
  unsigned* d = nullptr;
  void* h = nullptr;
  DCF_HIP(hipMalloc((void**)&d, sizeof(unsigned)));
  DCF_HIP(hipMemset(d, 0, sizeof(unsigned)));
  DCF_HIP(hipHostMalloc(&h, sizeof(unsigned), hipHostMallocDefault));
  *(volatile unsigned*)h = 0u;
  g_cg.dev = d; g_cg.host = (volatile unsigned*)h;
  return 0;
}

int cg_begin(const char* what, hipStream_t st, unsigned** word) {
  std::lock_guard<std::mutex> lk(g_cg_mu);
  if (cg_alloc()) return -1;
  // armed: the word stays on the device until the guarded norm reads and clears it there; no call fails for it
  if (!g_cg.guard && *g_cg.host) {
    *g_cg.host = 0u;
    DCF_HIP(hipMemsetAsync(g_cg.dev, 0, sizeof(unsigned), st));
    set_error("%s: an earlier gradient call of this process produced a non-finite sum (inf / NaN in dY or X, |X| >= 4094 or "
              "|W| >= 255.9 beyond the f16x3 operand range): its results are not trustworthy; the flag is now cleared", what);
    return -1;
  }
  *word = g_cg.dev;
  return 0;
}
int cg_end(hipStream_t st) {
  std::lock_guard<std::mutex> lk(g_cg_mu);
  if (g_cg.guard) return 0;             // armed: the host mirror is not fed, so nothing stale is left in it when the guard disarms
  DCF_HIP(hipMemcpyAsync((void*)g_cg.host, g_cg.dev, sizeof(unsigned), hipMemcpyDeviceToHost, st));
  return 0;
}

int cg_guard_arm(const void* state) {
  std::lock_guard<std::mutex> lk(g_cg_mu);
  if (cg_alloc()) return -1;
  g_cg.guard = state;
  return 0;
}
int cg_guard_disarm(hipStream_t st) {
  std::lock_guard<std::mutex> lk(g_cg_mu);
  if (!g_cg.guard) return 0;
  g_cg.guard = nullptr;
  // what was raised while armed and never consumed by a guarded norm surfaces at the next call, as it would have without the guard
  DCF_HIP(hipMemcpyAsync((void*)g_cg.host, g_cg.dev, sizeof(unsigned), hipMemcpyDeviceToHost, st));
  return 0;
}
unsigned* cg_guard_word(const void* state) {
  std::lock_guard<std::mutex> lk(g_cg_mu);
  return state && g_cg.guard == state ? g_cg.dev : nullptr;
}

}  // namespace dcf

using namespace dcf;

extern "C" {

int dcf_op_conv_bwd_weight(const float* X, const uint8_t* mask, const float* dY, float* dW_ock, float* db, int32_t B, int32_t T,
                           int32_t Cin, int32_t N, int32_t k, int32_t accumulate, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  DCF_CHECK(X && dY && dW_ock && B > 0 && T > 0, "dcf_op_conv_bwd_weight: null argument or empty batch");
  DCF_CHECK(k == 1 || k == 3, "dcf_op_conv_bwd_weight: k = %d (1 or 3)", k);
  DCF_CHECK(Cin > 0 && Cin % 32 == 0, "dcf_op_conv_bwd_weight: Cin = %d must be a positive multiple of 32", Cin);
  DCF_CHECK(N == 1 || N == 2 || (N > 0 && N % 32 == 0), "dcf_op_conv_bwd_weight: N = %d must be 1, 2 or a multiple of 32", N);
  DCF_CHECK((int64_t)B * T < (1ll << 31) - 64, "dcf_op_conv_bwd_weight: %lld rows (< 2^31)", (long long)B * T);
  const int rows = B * T;
  unsigned* status = nullptr;
  if (cg_begin("dcf_op_conv_bwd_weight", st, &status)) return -1;
  ConvGradArgs a{};
  a.X = X; a.dY = dY; a.rows = rows; a.Cin = Cin; a.N = N; a.k = k;
  if (N <= 2) {
    a.slice_rows = CG_SMALL_SLICE;
  } else {
    const int per = (rows + CG_MAX_SLICES - 1) / CG_MAX_SLICES;
    a.slice_rows = (per + WG_ROWS - 1) / WG_ROWS * WG_ROWS;
  }
  a.nslices = (rows + a.slice_rows - 1) / a.slice_rows;
  const int64_t count = (int64_t)N * k * Cin;
  StreamScratch sc(st);
  float *part = nullptr, *dbpart = nullptr;
  uint8_t* flags = nullptr;
  unsigned* word = nullptr;
  if (sc.take(&part, (size_t)a.nslices * count) || sc.take(&dbpart, (size_t)a.nslices * N)) return -1;
  if (sc.take(&flags, (size_t)rows) || sc.take(&word, 1)) return -1;
  hipLaunchKernelGGL(k_seqflags, dim3((rows + 255) / 256), dim3(256), 0, st, mask, flags, T, rows, 0);
  int rc = launch_absmax(dY, (int64_t)rows * N, word, st);
  a.flags = flags; a.absmax = word; a.part = part; a.dbpart = db ? dbpart : nullptr;
  if (rc == 0) rc = launch_wgrad(a, st);
  if (rc == 0) {
    hipLaunchKernelGGL(k_cg_reduce, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, part, a.nslices, count, (int)count, word,
                       N <= 2 ? 1.f : 1.f / WG_SX, dW_ock, k, Cin, accumulate, status);
    if (db)
      hipLaunchKernelGGL(k_cg_reduce, dim3((N + 255) / 256), dim3(256), 0, st, dbpart, a.nslices, (int64_t)N, N, word, 1.f, db, 1, 1,
                         accumulate, status);
    if (hipGetLastError() != hipSuccess) { set_error("dcf_op_conv_bwd_weight: launch failed"); rc = -1; }
  }
  rc = sc.end(rc);
  return rc == 0 ? cg_end(st) : rc;
}

int dcf_op_conv_bwd_data(const float* dY, const uint8_t* mask, const float* W_ock, float* dX, int32_t B, int32_t T, int32_t Cin,
                         int32_t N, int32_t k, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  DCF_CHECK(dY && W_ock && dX && B > 0 && T > 0, "dcf_op_conv_bwd_data: null argument or empty batch");
  DCF_CHECK(k == 1 || k == 3, "dcf_op_conv_bwd_data: k = %d (1 or 3)", k);
  DCF_CHECK(Cin > 0 && Cin % 32 == 0, "dcf_op_conv_bwd_data: Cin = %d must be a positive multiple of 32", Cin);
  DCF_CHECK(N == 1 || N == 2 || (N > 0 && N % 32 == 0), "dcf_op_conv_bwd_data: N = %d must be 1, 2 or a multiple of 32", N);
  DCF_CHECK((int64_t)B * T < (1ll << 31) - 64, "dcf_op_conv_bwd_data: %lld rows (< 2^31)", (long long)B * T);
  const int rows = B * T;
  unsigned* status = nullptr;
  if (cg_begin("dcf_op_conv_bwd_data", st, &status)) return -1;
  StreamScratch sc(st);
  uint8_t* flags = nullptr;
  if (sc.take(&flags, (size_t)rows)) return -1;
  int rc = 0;
  if (N <= 2) {
    hipLaunchKernelGGL(k_seqflags, dim3((rows + 255) / 256), dim3(256), 0, st, mask, flags, T, rows, 0);
    const dim3 grid(grid_for((int64_t)rows * Cin, 256, 8192));
    if (k == 3 && N == 1) hipLaunchKernelGGL((k_dgrad_small<3, 1>), grid, dim3(256), 0, st, dY, flags, W_ock, dX, (int64_t)rows, Cin);
    else if (k == 3) hipLaunchKernelGGL((k_dgrad_small<3, 2>), grid, dim3(256), 0, st, dY, flags, W_ock, dX, (int64_t)rows, Cin);
    else if (N == 1) hipLaunchKernelGGL((k_dgrad_small<1, 1>), grid, dim3(256), 0, st, dY, flags, W_ock, dX, (int64_t)rows, Cin);
    else hipLaunchKernelGGL((k_dgrad_small<1, 2>), grid, dim3(256), 0, st, dY, flags, W_ock, dX, (int64_t)rows, Cin);
    if (hipGetLastError() != hipSuccess) { set_error("dcf_op_conv_bwd_data: launch failed"); rc = -1; }
    rc = sc.end(rc);
    return rc == 0 ? cg_end(st) : rc;
  }
  const int K = k * N;
  float *dys = nullptr, *wp = nullptr;
  unsigned short* planes = nullptr;
  unsigned* word = nullptr;
  if (sc.take(&dys, (size_t)rows * N) || sc.take(&wp, (size_t)Cin * K)) return -1;
  if (sc.take(&planes, (size_t)3 * Cin * K) || sc.take(&word, 1)) return -1;
  // neighbour flags from the sequence ends alone: dY at a padded row is a legitimate operand
  hipLaunchKernelGGL(k_seqflags, dim3((rows + 255) / 256), dim3(256), 0, st, (const uint8_t*)nullptr, flags, T, rows, 1);
  rc = launch_absmax(dY, (int64_t)rows * N, word, st);
  if (rc == 0) {
    hipLaunchKernelGGL(k_scale_copy, dim3(grid_for((int64_t)rows * N, 1024, 4096)), dim3(256), 0, st, dY, dys, (int64_t)rows * N, word);
    hipLaunchKernelGGL(k_permute_wT, dim3((Cin * K + 255) / 256), dim3(256), 0, st, W_ock, wp, N, Cin, k);
    rc = launch_split_planes(wp, planes, Cin, K, K, st, GEMM_F16X3, status);
  }
  if (rc == 0) {
    GemmArgs g{};
    g.A = dys; g.lda = N; g.W = wp; g.ldw = K; g.Ws = planes; g.C = dX; g.ldc = Cin; g.M = rows; g.N = Cin; g.K = K;
    g.status = status;
    g.a_scale = 1.f;                 // the scratch copy is already scaled into [2^14, 2^15)
    if (k == 3) { g.cin = N; g.nbr = flags; }
    rc = launch_gemm_split(&g, 1, k == 3 ? A_ROWS_TAP3 : A_ROWS, GEMM_F16X3, st);
  }
  if (rc == 0) {
    hipLaunchKernelGGL(k_dx_finish, dim3(grid_for((int64_t)rows * (Cin / 4), 256, 8192)), dim3(256), 0, st, dX, mask, word, (int64_t)rows,
                       Cin / 4, status);
    if (hipGetLastError() != hipSuccess) { set_error("dcf_op_conv_bwd_data: launch failed"); rc = -1; }
  }
  rc = sc.end(rc);
  return rc == 0 ? cg_end(st) : rc;
}

static int conv5s2_check(const char* what, int32_t B, int32_t T, int32_t Cin, int32_t N) {
  DCF_CHECK(B > 0 && T > 0, "%s: empty batch", what);
  DCF_CHECK(T % 2 == 0, "%s: T = %d must be even (stride 2)", what, T);
  DCF_CHECK(Cin > 0 && Cin % 32 == 0, "%s: Cin = %d must be a positive multiple of 32", what, Cin);
  DCF_CHECK(N > 0 && N % 32 == 0, "%s: N = %d must be a positive multiple of 32", what, N);
  DCF_CHECK((int64_t)B * T < (1ll << 31) - 64, "%s: %lld rows (< 2^31)", what, (long long)B * T);
  return 0;
}

int dcf_op_conv5s2_split(const float* X, const uint8_t* mask, const float* W_ock, float* Y, int32_t B, int32_t T, int32_t Cin,
                         int32_t N, int32_t nterms, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  DCF_CHECK(X && W_ock && Y, "dcf_op_conv5s2_split: null argument");
  if (conv5s2_check("dcf_op_conv5s2_split", B, T, Cin, N)) return -1;
  DCF_CHECK(nterms == GEMM_F16X3 || nterms == GEMM_BF16X6, "dcf_op_conv5s2_split: nterms = %d (16 = f16x3, 6 = bf16x6)", nterms);
  const int rows_in = B * T, rows = rows_in / 2, K = 5 * Cin;
  StreamScratch sc(st);
  float *col = nullptr, *wf = nullptr;
  uint8_t* ones = nullptr;
  unsigned short* planes = nullptr;
  if (sc.take(&col, (size_t)rows * K) || sc.take(&wf, (size_t)N * K)) return -1;
  if (sc.take(&planes, (size_t)3 * N * K)) return -1;
  if (!mask) {
    if (sc.take(&ones, (size_t)rows_in)) return -1;
    DCF_HIP(hipMemsetAsync(ones, 1, (size_t)rows_in, st));
  }
  hipLaunchKernelGGL(k_permute_w5, dim3((N * K + 255) / 256), dim3(256), 0, st, W_ock, wf, N, Cin);
  int rc = launch_im2col5s2(X, Cin, mask ? mask : ones, col, B, T, Cin, st);
  if (rc == 0) rc = launch_split_planes(wf, planes, N, K, K, st, nterms);
  if (rc == 0) {
    GemmArgs g{};
    g.A = col; g.lda = K; g.W = wf; g.ldw = 0; g.Ws = planes; g.C = Y; g.ldc = N; g.M = rows; g.N = N; g.K = K;
    rc = launch_gemm_split(&g, 1, A_ROWS, nterms, st);
  }
  rc = sc.end(rc);
  return rc;
}

int dcf_op_conv5s2_bwd_weight(const float* X, const uint8_t* mask, const float* dY, float* dW_ock, int32_t B, int32_t T, int32_t Cin,
                              int32_t N, int32_t accumulate, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  DCF_CHECK(X && dY && dW_ock, "dcf_op_conv5s2_bwd_weight: null argument");
  if (conv5s2_check("dcf_op_conv5s2_bwd_weight", B, T, Cin, N)) return -1;
  const int To = T / 2, rows = B * To;
  unsigned* status = nullptr;
  if (cg_begin("dcf_op_conv5s2_bwd_weight", st, &status)) return -1;
  ConvGradArgs a{};
  a.X = X; a.dY = dY; a.rows = rows; a.Cin = Cin; a.N = N; a.k = 5;
  const int per = (rows + CG_MAX_SLICES - 1) / CG_MAX_SLICES;
  a.slice_rows = (per + WG_ROWS - 1) / WG_ROWS * WG_ROWS;
  a.nslices = (rows + a.slice_rows - 1) / a.slice_rows;
  const int64_t count = (int64_t)N * 5 * Cin;
  StreamScratch sc(st);
  float* part = nullptr;
  uint8_t* flags = nullptr;
  unsigned* word = nullptr;
  if (sc.take(&part, (size_t)a.nslices * count) || sc.take(&flags, (size_t)rows)) return -1;
  if (sc.take(&word, 1)) return -1;
  // per output row: does an output row to the left / right exist in its sequence (the input rows' mask is read by the kernel)
  hipLaunchKernelGGL(k_seqflags, dim3((rows + 255) / 256), dim3(256), 0, st, (const uint8_t*)nullptr, flags, To, rows, 1);
  int rc = launch_absmax(dY, (int64_t)rows * N, word, st);
  a.flags = flags; a.absmax = word; a.part = part; a.dbpart = nullptr;
  if (rc == 0) {
    const dim3 grid(((N + 63) / 64) * ((Cin + 63) / 64), a.nslices);
    hipLaunchKernelGGL(k_wgrad5, grid, dim3(256), 0, st, a, mask);
    hipLaunchKernelGGL(k_cg_reduce, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, part, a.nslices, count, (int)count, word,
                       1.f / WG_SX, dW_ock, 5, Cin, accumulate, status);
    if (hipGetLastError() != hipSuccess) { set_error("dcf_op_conv5s2_bwd_weight: launch failed"); rc = -1; }
  }
  rc = sc.end(rc);
  return rc == 0 ? cg_end(st) : rc;
}

int dcf_op_conv5s2_bwd_data(const float* dY, const uint8_t* mask, const float* W_ock, float* dX, int32_t B, int32_t T, int32_t Cin,
                            int32_t N, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  DCF_CHECK(dY && W_ock && dX, "dcf_op_conv5s2_bwd_data: null argument");
  if (conv5s2_check("dcf_op_conv5s2_bwd_data", B, T, Cin, N)) return -1;
  const int To = T / 2, rows = B * To, K = 3 * N;
  unsigned* status = nullptr;
  if (cg_begin("dcf_op_conv5s2_bwd_data", st, &status)) return -1;
  StreamScratch sc(st);
  uint8_t* flags = nullptr;
  float *dys = nullptr, *wp = nullptr;
  unsigned short* planes = nullptr;
  unsigned* word = nullptr;
  const size_t img = (size_t)Cin * K;
  if (sc.take(&flags, (size_t)rows) || sc.take(&dys, (size_t)rows * N)) return -1;
  if (sc.take(&wp, 2 * img) || sc.take(&planes, 2 * 3 * img)) return -1;
  if (sc.take(&word, 1)) return -1;
  // neighbour flags of the OUTPUT rows from the sequence ends alone: dY at a padded output row is a legitimate operand
  hipLaunchKernelGGL(k_seqflags, dim3((rows + 255) / 256), dim3(256), 0, st, (const uint8_t*)nullptr, flags, To, rows, 1);
  int rc = launch_absmax(dY, (int64_t)rows * N, word, st);
  if (rc == 0) {
    hipLaunchKernelGGL(k_scale_copy, dim3(grid_for((int64_t)rows * N, 1024, 4096)), dim3(256), 0, st, dY, dys, (int64_t)rows * N, word);
    for (int par = 0; par < 2 && rc == 0; ++par) {
      hipLaunchKernelGGL(k_permute_w5T, dim3((unsigned)((img + 255) / 256)), dim3(256), 0, st, W_ock, wp + par * img, N, Cin, par);
      rc = launch_split_planes(wp + par * img, planes + par * 3 * img, Cin, K, K, st, GEMM_F16X3, status);
    }
  }
  if (rc == 0) {
    // input rows 2 u (parity 0) and 2 u + 1 (parity 1) of dX: row u of GEMM `par` lands at dX + (2 u + par) Cin
    GemmArgs g[2] = {};
    for (int par = 0; par < 2; ++par) {
      g[par].A = dys; g[par].lda = N; g[par].W = wp + par * img; g[par].ldw = K; g[par].Ws = planes + par * 3 * img;
      g[par].C = dX + (size_t)par * Cin; g[par].ldc = 2 * (int64_t)Cin; g[par].M = rows; g[par].N = Cin; g[par].K = K;
      g[par].status = status; g[par].a_scale = 1.f; g[par].cin = N; g[par].nbr = flags;
    }
    rc = launch_gemm_split(g, 2, A_ROWS_TAP3, GEMM_F16X3, st);
  }
  if (rc == 0) {
    hipLaunchKernelGGL(k_dx_finish, dim3(grid_for((int64_t)2 * rows * (Cin / 4), 256, 8192)), dim3(256), 0, st, dX, mask, word, (int64_t)2 * rows,
                       Cin / 4, status);
    if (hipGetLastError() != hipSuccess) { set_error("dcf_op_conv5s2_bwd_data: launch failed"); rc = -1; }
  }
  rc = sc.end(rc);
  return rc == 0 ? cg_end(st) : rc;
}

int dcf_op_layernorm_bwd(const float* X, const float* w, const float* b, const float* dOut, float* dX, float* dw, float* db,
                         int32_t rows, int32_t C, int32_t relu, int32_t accumulate, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  DCF_CHECK(X && dOut && dX && rows > 0, "dcf_op_layernorm_bwd: null argument or no rows");
  DCF_CHECK(C > 0 && C % 32 == 0 && C <= 1024, "dcf_op_layernorm_bwd: C = %d must be a multiple of 32 up to 1024", C);
  DCF_CHECK((w == nullptr) == (b == nullptr), "dcf_op_layernorm_bwd: w and b come together");
  DCF_CHECK(w || (!dw && !db), "dcf_op_layernorm_bwd: dw / db without an affine LayerNorm");
  unsigned* status = nullptr;
  if (cg_begin("dcf_op_layernorm_bwd", st, &status)) return -1;
  LnBwdArgs a{};
  a.X = X; a.w = w; a.b = b; a.dOut = dOut; a.dX = dX; a.rows = rows; a.C = C; a.relu = relu;
  a.rows_per_wave = (rows + 2047) / 2048;                      // <= 512 workgroups of four waves: a fixed function of `rows`
  const int nwg = (rows + 4 * a.rows_per_wave - 1) / (4 * a.rows_per_wave);
  StreamScratch sc(st);
  float* part = nullptr;
  if ((dw || db) && sc.take(&part, (size_t)nwg * 2 * C)) return -1;
  a.part = part;
  int rc = launch_ln_bwd(a, nwg, st);
  if (rc == 0 && part) {
    if (dw)
      hipLaunchKernelGGL(k_cg_reduce, dim3((C + 255) / 256), dim3(256), 0, st, part, nwg, (int64_t)2 * C, C, (const unsigned*)nullptr, 1.f, dw, 1,
                         1, accumulate, status);
    if (db)
      hipLaunchKernelGGL(k_cg_reduce, dim3((C + 255) / 256), dim3(256), 0, st, part + C, nwg, (int64_t)2 * C, C, (const unsigned*)nullptr, 1.f, db,
                         1, 1, accumulate, status);
    if (hipGetLastError() != hipSuccess) { set_error("dcf_op_layernorm_bwd: launch failed"); rc = -1; }
  }
  rc = sc.end(rc);
  return rc == 0 ? cg_end(st) : rc;
}

}  // extern "C"
