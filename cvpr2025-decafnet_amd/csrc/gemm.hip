// fp32 GEMM on the gfx950 matrix cores: C[M][N] = A[M][K] * W[N][K]^T (+ fused epilogues).
//
// Why fp32 MFMA: the reference runs in fp32 with TF32 disabled (eval.py:38-41) and the parity
// bar is 1e-3 on logits after ~60 chained layers, so the dense convolutions use
// v_mfma_f32_32x32x2_f32 (exact fp32 FMA chain, 157 TFLOP/s dense peak on MI355X).
//
// Tiling (64-wide wavefronts, 4 waves / workgroup):
//   workgroup tile BM x BN = (WM*TM*32) x (WN*TN*32), K step 32.
//   A and W tiles are staged in LDS as [row][36] floats (pitch 36 = 4*9 keeps every 16-lane
//   ds_read_b128 group on 64 distinct banks).  Lane l = (r = l&31, h = l>>5) reads 4
//   consecutive k values A[r][8*kk + 4*h .. +3] with ONE ds_read_b128 and feeds them to 4
//   successive MFMAs; the k index inside an 8-chunk is therefore permuted identically for A
//   and W, which leaves the dot product unchanged.
//   The next K tile is prefetched global->registers while the current one is multiplied.
#include <cstdio>
#include <cstdlib>

#include "gemm_common.h"

namespace dcf {


template <int WM, int WN, int TM, int TN, int AMODE, int BK>
__global__ __launch_bounds__(256, (TM * TN >= 3 ? 2 : 3)) void gemm_f32_kernel(GemmBatch batch) {
  constexpr int PITCH = BK + 4;             // 36 = 4*9 / 68 = 4*17: odd multiples of 4 keep b128 reads conflict free
  constexpr int C4 = BK / 4;                // f32x4 per tile row
  constexpr int BM = WM * TM * 32;
  constexpr int BN = WN * TN * 32;
  constexpr int A_F4 = BM * BK / 4 / 256;  // f32x4 per thread for the A tile
  constexpr int B_F4 = BN * BK / 4 / 256;
  constexpr int APITCH_KM = BM + 4;         // A_CHANMAJOR: LDS tile is [k][m]
  static_assert(WM * WN == 4, "4 waves per workgroup");
  static_assert((BM * BK / 4) % 256 == 0 && (BN * BK / 4) % 256 == 0, "tile/threads mismatch");

  extern __shared__ float smem[];
  float* As = smem;                                                  // [BM][PITCH] or [BK][APITCH_KM]
  float* Bs = smem + (AMODE == A_CHANMAJOR ? BK * APITCH_KM : BM * PITCH);  // [BN][PITCH]

  // select by value (a dynamically indexed by-value kernarg array would be spilled to scratch)
  const GemmArgs p = blockIdx.z == 0 ? batch.g[0] : (blockIdx.z == 1 ? batch.g[1] : batch.g[2]);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WN;
  const int wn = wave % WN;
  const int r = lane & 31;
  const int h = lane >> 5;
  int m0, n0;
  if (!tile_origin<BM, BN>(p, m0, n0)) return;
  const int M = p.M, K = p.K;
  const int KT = K / BK;


  // Row predicates / base pointers of this thread's A-tile slots are K-invariant: resolve them once so
  // that the K loop issues nothing but 16-byte loads (a mask byte load inside the loop would force an
  // s_waitcnt vmcnt(0) in front of the MFMAs and expose the whole W-tile fetch every step).
  const float* a_ptr[A_F4];
  unsigned a_flag[A_F4];
#pragma unroll
  for (int i = 0; i < A_F4; ++i) {
    int idx = i * 256 + tid;
    if constexpr (AMODE == A_CHANMAJOR) {
      constexpr int TPR = BM / 4;
      int kr = idx / TPR, m4 = idx % TPR;
      a_ptr[i] = p.A + (int64_t)kr * p.lda + m0 + m4 * 4;
      a_flag[i] = (unsigned)(m0 + m4 * 4);
    } else {
      int row = idx / C4, c4 = idx % C4;
      int m = m0 + row;
      unsigned f = 0;
      if (m < M) {
        if constexpr (AMODE == A_ROWS) f = (p.flags & G_AMASK) ? (p.rowmask[m] ? 1u : 0u) : 1u;
        else f = p.nbr[m];
      }
      a_flag[i] = f;
      a_ptr[i] = p.A + (int64_t)(m < M ? m : 0) * p.lda + c4 * 4;
    }
  }
  const f32x4* w_ptr[B_F4];
#pragma unroll
  for (int i = 0; i < B_F4; ++i) {
    int idx = i * 256 + tid;
    int row = idx / C4, c4 = idx % C4;
    w_ptr[i] = reinterpret_cast<const f32x4*>(p.W + (int64_t)(n0 + row) * p.ldw + c4 * 4);
  }

  auto load_tiles = [&](int kt, f32x4 (&areg)[A_F4], f32x4 (&breg)[B_F4]) __attribute__((always_inline)) {
    const int k0 = kt * BK;
    // ---- W tile: rows n0..n0+BN, cols k0..k0+32 (always in range: N % BN == 0, K % 32 == 0)
#pragma unroll
    for (int i = 0; i < B_F4; ++i) breg[i] = w_ptr[i][k0 / 4];
    // ---- A tile
    if constexpr (AMODE == A_ROWS) {
#pragma unroll
      for (int i = 0; i < A_F4; ++i) {
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (a_flag[i]) v = *reinterpret_cast<const f32x4*>(a_ptr[i] + k0);
        areg[i] = v;
      }
    } else if constexpr (AMODE == A_ROWS_TAP3) {
      const int tap = k0 / p.cin;           // cin % 32 == 0 so a K tile never straddles taps
      const int c0 = k0 - tap * p.cin;
      const unsigned bit = tap == 0 ? 2u : (tap == 1 ? 1u : 4u);
      const int64_t shift = (int64_t)(tap - 1) * p.lda + c0;
#pragma unroll
      for (int i = 0; i < A_F4; ++i) {
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (a_flag[i] & bit) v = *reinterpret_cast<const f32x4*>(a_ptr[i] + shift);
        areg[i] = v;
      }
    } else {  // A_CHANMAJOR: 32 k-rows x BM m, f32x4 along m
      const bool vec = (p.lda & 3) == 0;
#pragma unroll
      for (int i = 0; i < A_F4; ++i) {
        const int m = (int)a_flag[i];
        const float* src = a_ptr[i] + (int64_t)k0 * p.lda;
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (vec && m + 3 < M) {
          v = *reinterpret_cast<const f32x4*>(src);
        } else {
          if (m + 0 < M) v.x = src[0];
          if (m + 1 < M) v.y = src[1];
          if (m + 2 < M) v.z = src[2];
          if (m + 3 < M) v.w = src[3];
        }
        areg[i] = v;
      }
    }
  };

  auto store_tiles = [&](const f32x4 (&areg)[A_F4], const f32x4 (&breg)[B_F4]) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < B_F4; ++i) {
      int idx = i * 256 + tid;
      int row = idx / C4, c4 = idx % C4;
      *reinterpret_cast<f32x4*>(Bs + row * PITCH + c4 * 4) = breg[i];
    }
    if constexpr (AMODE == A_CHANMAJOR) {
      constexpr int TPR = BM / 4;
#pragma unroll
      for (int i = 0; i < A_F4; ++i) {
        int idx = i * 256 + tid;
        int kr = idx / TPR, m4 = idx % TPR;
        *reinterpret_cast<f32x4*>(As + kr * APITCH_KM + m4 * 4) = areg[i];
      }
    } else {
#pragma unroll
      for (int i = 0; i < A_F4; ++i) {
        int idx = i * 256 + tid;
        int row = idx / C4, c4 = idx % C4;
        *reinterpret_cast<f32x4*>(As + row * PITCH + c4 * 4) = areg[i];
      }
    }
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  auto compute = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int kk = 0; kk < BK / 8; ++kk) {
      f32x4 a[TM], b[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        int row = (wm * TM + i) * 32 + r;
        if constexpr (AMODE == A_CHANMAJOR) {
          const float* q = As + (kk * 8 + h * 4) * APITCH_KM + row;
          a[i] = f32x4{q[0], q[APITCH_KM], q[2 * APITCH_KM], q[3 * APITCH_KM]};
        } else {
          a[i] = *reinterpret_cast<const f32x4*>(As + row * PITCH + kk * 8 + h * 4);
        }
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        int row = (wn * TN + j) * 32 + r;
        b[j] = *reinterpret_cast<const f32x4*>(Bs + row * PITCH + kk * 8 + h * 4);
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].x, b[j].x, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].y, b[j].y, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].z, b[j].z, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].w, b[j].w, acc[i][j], 0, 0, 0);
        }
    }
  };

  // one K tile in flight: fetched global->registers while the previous tile is multiplied.  (Keeping
  // two tiles in flight was measured and buys nothing: a lone workgroup is bound by its two barriers
  // and the LDS round trip per K tile, not by the global fetch.)
  f32x4 areg[A_F4], breg[B_F4];
  load_tiles(0, areg, breg);
  for (int kt = 0; kt < KT; ++kt) {
    __syncthreads();
    store_tiles(areg, breg);
    __syncthreads();
    load_tiles(kt + 1 < KT ? kt + 1 : kt, areg, breg);   // unconditional (last iteration re-reads its own tile)
    compute();
  }

  gemm_epilogue<WM, WN, TM, TN>(p, acc, m0, n0, wm, wn, r, h);
}

template <int WM, int WN, int TM, int TN, int BK = 32>
static int launch_cfg(const GemmBatch& b, int count, GemmAMode mode, hipStream_t stream) {
  constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
  const GemmArgs& p = b.g[0];
  dim3 grid(tile_grid<BM, BN>(p), 1, count);
  char name[96];
  snprintf(name, sizeof(name), "gemm_f32<%dx%dx%d,%s>", BM, BN, BK, mode == A_ROWS ? "rows" : mode == A_ROWS_TAP3 ? "tap3" : "chanmajor");
  const double mnk = (double)count * p.M * (double)p.N * p.K;
  ProfScope prof(name, stream, 2.0 * mnk,
                 4.0 * count * ((double)p.M * p.K / (mode == A_ROWS_TAP3 ? 3 : 1) + (double)p.N * p.K + (double)p.M * p.N * ((p.flags & G_RES) ? 2 : 1)));
  constexpr int PITCH = BK + 4;
  size_t lds_rows = (size_t)(BM + BN) * PITCH * sizeof(float);
  size_t lds_km = (size_t)(BK * (BM + 4) + BN * PITCH) * sizeof(float);
  DCF_CHECK(p.K % BK == 0 && (mode != A_ROWS_TAP3 || p.cin % BK == 0), "launch_gemm: K/cin not a multiple of BK=%d", BK);
  switch (mode) {
    case A_ROWS:
      hipLaunchKernelGGL((gemm_f32_kernel<WM, WN, TM, TN, A_ROWS, BK>), grid, dim3(256), lds_rows, stream, b);
      break;
    case A_ROWS_TAP3:
      hipLaunchKernelGGL((gemm_f32_kernel<WM, WN, TM, TN, A_ROWS_TAP3, BK>), grid, dim3(256), lds_rows, stream, b);
      break;
    case A_CHANMAJOR:
      hipLaunchKernelGGL((gemm_f32_kernel<WM, WN, TM, TN, A_CHANMAJOR, BK>), grid, dim3(256), lds_km, stream, b);
      break;
    default:
      DCF_CHECK(false, "launch_gemm: the fp32 kernel has no A mode %d (half operands run on the split tile kernels)", (int)mode);
  }
  DCF_HIP(hipGetLastError());
  return 0;
}

int launch_gemm(const GemmArgs* g, int count, GemmAMode mode, hipStream_t stream) {
  DCF_CHECK(count >= 1 && count <= 3, "launch_gemm: count %d out of range", count);
  GemmBatch b{};
  for (int i = 0; i < 3; ++i) {
    b.g[i] = g[i < count ? i : 0];
    if (b.g[i].ldw == 0) b.g[i].ldw = b.g[i].K;
  }
  const GemmArgs& p = g[0];
  for (int i = 0; i < count; ++i) {
    DCF_CHECK(g[i].M == p.M && g[i].N == p.N && g[i].K == p.K, "launch_gemm: grouped shapes differ");
    DCF_CHECK(g[i].A && g[i].W && g[i].C, "launch_gemm: null operand");
    DCF_CHECK((g[i].lda % 4) == 0 || mode == A_CHANMAJOR, "launch_gemm: lda %% 4 != 0");
    DCF_CHECK(b.g[i].ldw % 4 == 0 && b.g[i].ldw >= g[i].K, "launch_gemm: bad ldw");
    if (mode == A_ROWS_TAP3) DCF_CHECK(g[i].nbr && g[i].cin % 32 == 0 && g[i].K == 3 * g[i].cin, "launch_gemm: bad tap3 args");
    if (g[i].flags & (G_AMASK | G_RES_MASK | G_OUT_MASK)) DCF_CHECK(g[i].rowmask, "launch_gemm: rowmask missing");
    if (g[i].flags & G_RES) DCF_CHECK(g[i].R, "launch_gemm: residual missing");
    DCF_CHECK(!g[i].stats_out && !g[i].stats_in, "launch_gemm: row statistics are carried by the split kernels only");
  }
  if (p.M <= 0) return 0;
  DCF_CHECK(p.K > 0 && p.K % 32 == 0, "launch_gemm: K=%d must be a positive multiple of 32", p.K);
  DCF_CHECK(p.N > 0 && p.N % 32 == 0, "launch_gemm: N=%d must be a positive multiple of 32", p.N);
  // Tile choice: the largest tile that still gives every CU >= 2 workgroups (one wave per SIMD cannot
  // overlap its own global->LDS staging with its MFMAs); small problems take the smallest tile so that
  // the launch is spread over as many CUs as possible.
  const int N = p.N;
  auto wgs = [&](int bm, int bn) { return (long)((p.M + bm - 1) / bm) * (N / bn) * count; };
  constexpr long WANT = 512;
  // DCF_GEMM_CFG="BMxBN" forces a tile for experiments (tools/gemm_sweep.py); ignored if it does not divide N
  static const char* forced = getenv("DCF_GEMM_CFG");
  if (forced) {
    int bm = 0, bn = 0, bk = 32;
    const int nf = sscanf(forced, "%dx%dx%d", &bm, &bn, &bk);
    const bool k64ok = p.K % 64 == 0 && (mode != A_ROWS_TAP3 || p.cin % 64 == 0);
    if (nf >= 2 && bn > 0 && N % bn == 0 && bk == 64 && k64ok) {
      if (bm == 64 && bn == 128) return launch_cfg<2, 2, 1, 2, 64>(b, count, mode, stream);
      if (bm == 64 && bn == 64) return launch_cfg<2, 2, 1, 1, 64>(b, count, mode, stream);
      if (bm == 128 && bn == 64) return launch_cfg<4, 1, 1, 2, 64>(b, count, mode, stream);
      if (bm == 128 && bn == 128) return launch_cfg<4, 1, 1, 4, 64>(b, count, mode, stream);
    }
    if (nf >= 2 && bn > 0 && N % bn == 0 && bk == 32) {
      if (bm == 64 && bn == 256) return launch_cfg<2, 2, 1, 4>(b, count, mode, stream);
      if (bm == 64 && bn == 128) return launch_cfg<2, 2, 1, 2>(b, count, mode, stream);
      if (bm == 64 && bn == 64) return launch_cfg<2, 2, 1, 1>(b, count, mode, stream);
      if (bm == 128 && bn == 32) return launch_cfg<4, 1, 1, 1>(b, count, mode, stream);
      if (bm == 128 && bn == 64) return launch_cfg<4, 1, 1, 2>(b, count, mode, stream);
      if (bm == 128 && bn == 96) return launch_cfg<4, 1, 1, 3>(b, count, mode, stream);
      if (bm == 128 && bn == 128) return launch_cfg<4, 1, 1, 4>(b, count, mode, stream);
      if (bm == 128 && bn == 160) return launch_cfg<4, 1, 1, 5>(b, count, mode, stream);
      if (bm == 129 && bn == 128) return launch_cfg<2, 2, 2, 2>(b, count, mode, stream);   // 128x128, 64x64 per wave
    }
  }
  if (N % 256 == 0 && wgs(64, 256) >= WANT) return launch_cfg<2, 2, 1, 4>(b, count, mode, stream);
  if (N % 160 == 0 && N % 64 != 0) return launch_cfg<4, 1, 1, 5>(b, count, mode, stream);
  if (N % 128 == 0 && wgs(64, 128) >= WANT) return launch_cfg<2, 2, 1, 2>(b, count, mode, stream);
  if (N % 96 == 0 && N % 64 != 0) return launch_cfg<4, 1, 1, 3>(b, count, mode, stream);
  if (N % 64 == 0) return launch_cfg<2, 2, 1, 1>(b, count, mode, stream);
  return launch_cfg<4, 1, 1, 1>(b, count, mode, stream);
}

}  // namespace dcf
