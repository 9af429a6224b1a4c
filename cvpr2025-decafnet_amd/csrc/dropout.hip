// Dropout / drop-path kernels of the training forward (contract: dropout.h, include/decafnet_hip.h).
//
// The engine keeps activations token-major, rows [b][t] x C; the reference's element index is channel-major,
// e = (b * C + c) * T + t.  A thread takes a 4 x 4 block: four consecutive positions t = 4 tq .. 4 tq + 3 of one sequence
// (one 16-byte access per row) times four consecutive channels.  When T % 4 == 0 the four positions of one channel are one
// Philox counter block (e = 4 j .. 4 j + 3), so a block costs four Philox calls; otherwise every element draws its own.
#include "../../include/decafnet_hip.h"
#include "common.h"
#include "dropout.h"

namespace dcf {

constexpr int DROP_NT = 256;

__global__ __launch_bounds__(DROP_NT) void k_dropout(float* __restrict__ X, int64_t ld, int nseq, int C, int T, int b0,
                                                     uint64_t seed, DropSite d) {
  const int C4 = C / 4, TQ = (T + 3) / 4;
  const int64_t id = (int64_t)blockIdx.x * DROP_NT + threadIdx.x;
  if (id >= (int64_t)nseq * TQ * C4) return;
  const int c4 = (int)(id % C4);
  const int64_t q = id / C4;
  const int s = (int)(q / TQ), t0 = (int)(q % TQ) * 4;
  const unsigned bits = block_keep(seed, d, (int64_t)b0 + s, C, T, 4 * c4, t0);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (t0 + i >= T) break;
    f32x4* p = reinterpret_cast<f32x4*>(X + ((int64_t)s * T + t0 + i) * ld + 4 * c4);
    f32x4 v = *p;
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) v[cc] = ((bits >> (4 * i + cc)) & 1u) ? v[cc] * d.scale : 0.f;
    *p = v;
  }
}

int launch_dropout(float* X, int64_t ld, int rows, int C, int T, int b0, uint64_t seed, const DropSite& d, hipStream_t st) {
  if (d.p <= 0.f) return 0;
  DCF_CHECK(X && T > 0 && rows % T == 0 && C % 4 == 0 && ld % 4 == 0 && b0 >= 0, "launch_dropout: bad geometry (rows %d, T %d, C %d)", rows, T, C);
  const int64_t n = (int64_t)(rows / T) * ((T + 3) / 4) * (C / 4);
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_dropout, dim3((unsigned)((n + DROP_NT - 1) / DROP_NT)), dim3(DROP_NT), 0, st, X, ld, rows / T, C, T, b0, seed, d);
  DCF_HIP(hipGetLastError());
  return 0;
}

__global__ __launch_bounds__(DROP_NT) void k_drop_residual(DropResArgs a) {
  const int C4 = a.C / 4, TQ = (a.T + 3) / 4, nseq = a.rows / a.T;
  const int64_t id = (int64_t)blockIdx.x * DROP_NT + threadIdx.x;
  if (id >= (int64_t)nseq * TQ * C4) return;
  const int c4 = (int)(id % C4);
  const int64_t q = id / C4;
  const int s = (int)(q / TQ), t0 = (int)(q % TQ) * 4;
  const int64_t bg = (int64_t)a.b0 + s;
  const unsigned bits = block_keep(a.seed, a.drop, bg, a.C, a.T, 4 * c4, t0);
  float dp = 1.f;                                              // drop-path: one decision per sample (blocks.py:685-694)
  if (a.path.p > 0.f) dp = drop_keep(a.seed, a.path.site, (uint64_t)bg, a.path.p) ? a.path.scale : 0.f;
  const f32x4 ls = *reinterpret_cast<const f32x4*>(a.ls + 4 * c4);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (t0 + i >= a.T) break;
    const int64_t r = (int64_t)s * a.T + t0 + i;
    const float m = a.rowmask ? (a.rowmask[r] ? 1.f : 0.f) : 1.f;
    const f32x4 h = *reinterpret_cast<const f32x4*>(a.H + r * a.ldh + 4 * c4);
    const f32x4 x = *reinterpret_cast<const f32x4*>(a.R + r * a.ldr + 4 * c4);
    f32x4 o;
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) {
      float v = a.out_mask ? h[cc] * m : h[cc];
      v = ((bits >> (4 * i + cc)) & 1u) ? v * a.drop.scale : 0.f;
      o[cc] = (a.res_mask ? x[cc] * m : x[cc]) + ls[cc] * v * dp;
    }
    *reinterpret_cast<f32x4*>(a.out + r * a.ldo + 4 * c4) = o;
  }
}

int launch_drop_residual(const DropResArgs& a, hipStream_t st) {
  DCF_CHECK(a.out && a.R && a.H && a.ls && a.T > 0 && a.rows % a.T == 0 && a.C % 4 == 0 && a.ldo % 4 == 0 && a.ldr % 4 == 0 &&
            a.ldh % 4 == 0 && a.b0 >= 0, "launch_drop_residual: bad geometry (rows %d, T %d, C %d)", a.rows, a.T, a.C);
  DCF_CHECK(!(a.res_mask || a.out_mask) || a.rowmask, "launch_drop_residual: masking needs the row mask");
  const int64_t n = (int64_t)(a.rows / a.T) * ((a.T + 3) / 4) * (a.C / 4);
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_drop_residual, dim3((unsigned)((n + DROP_NT - 1) / DROP_NT)), dim3(DROP_NT), 0, st, a);
  DCF_HIP(hipGetLastError());
  return 0;
}

// the keep bits of elements e0 .. e0 + n - 1 of one site (dcf_debug_dropout_keep)
__global__ __launch_bounds__(DROP_NT) void k_dropout_keep(uint64_t seed, uint32_t site, uint64_t e0, int64_t n, float p,
                                                          uint8_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * DROP_NT + threadIdx.x;
  if (i >= n) return;
  out[i] = drop_keep(seed, site, e0 + (uint64_t)i, p) ? 1 : 0;
}

}  // namespace dcf

int dcf_debug_dropout_keep(int64_t seed, int32_t site, int64_t e0, int64_t n, float p, uint8_t* out, void* stream) {
  DCF_CHECK(out && e0 >= 0 && n >= 0 && n <= (1ll << 31) * 64, "dcf_debug_dropout_keep: bad arguments");
  DCF_CHECK(p >= 0.f && p < 1.f, "dcf_debug_dropout_keep: p = %g outside [0, 1)", (double)p);
  if (n == 0) return 0;
  hipLaunchKernelGGL(dcf::k_dropout_keep, dim3((unsigned)((n + dcf::DROP_NT - 1) / dcf::DROP_NT)), dim3(dcf::DROP_NT), 0,
                     (hipStream_t)stream, (uint64_t)seed, (uint32_t)site, (uint64_t)e0, n, p, out);
  DCF_HIP(hipGetLastError());
  return 0;
}
