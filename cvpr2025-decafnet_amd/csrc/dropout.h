// Dropout and drop-path of the training forward (blocks.py:392, :535-538, :586-590, :649, :685-694; tcn.py:27) on a
// counter-based random stream: Philox4x32-10 keyed by a 64-bit seed.  The keep decision of an element is a function of
// (seed, site, element index) alone -- not of tiling, launch geometry or the engine's row layout -- so a CPU restatement
// reproduces every mask bit for bit (contract: include/decafnet_hip.h, dcf_model_set_dropout).
//
//   counter = (j & 0xffffffff, j >> 32, site, 0), j = e >> 2; key = (seed & 0xffffffff, seed >> 32); element e takes word e & 3
//   u = (word >> 8) * 2^-24; kept iff u >= p; a kept value is multiplied by scale = 1 / (1 - p) (fp32, computed on the host)
//   e = (b * C + c) * T_l + t for dropout on a (B', C, T_l) tensor of the reference, e = b for drop-path
//   site = group << 16 | layer << 4 | sub (DROP_* below)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dcf {

// site groups
constexpr uint32_t DROP_G_FUSION = 1, DROP_G_STEM = 2, DROP_G_BRANCH = 3, DROP_G_REFINE = 4;
// site subs
constexpr uint32_t DROP_PROJ = 0, DROP_FFN_HID = 1, DROP_FFN_OUT = 2, DROP_PATH_ATTN = 3, DROP_PATH_FFN = 4, DROP_TCN = 5;
__host__ __device__ constexpr uint32_t drop_site(uint32_t group, uint32_t layer, uint32_t sub) {
  return group << 16 | layer << 4 | sub;
}

struct Philox4 { uint32_t x, y, z, w; };

__host__ __device__ __forceinline__ uint32_t mulhi32(uint32_t a, uint32_t b) {
  return (uint32_t)(((uint64_t)a * b) >> 32);
}
__host__ __device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
    const uint32_t hi0 = mulhi32(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = mulhi32(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
  }
  return Philox4{c0, c1, c2, c3};
}
// the four words of counter block j = e >> 2 of `site`
__host__ __device__ __forceinline__ Philox4 drop_block(uint64_t seed, uint32_t site, uint64_t j) {
  return philox4x32_10((uint32_t)j, (uint32_t)(j >> 32), site, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
}
__host__ __device__ __forceinline__ bool drop_keep_word(uint32_t word, float p) {
  return (float)(word >> 8) * 5.9604644775390625e-08f >= p;        // 2^-24: exact in fp32
}
__host__ __device__ __forceinline__ uint32_t philox_word(const Philox4& v, int i) {
  return i == 0 ? v.x : (i == 1 ? v.y : (i == 2 ? v.z : v.w));
}
// keep bit of one element
__host__ __device__ __forceinline__ bool drop_keep(uint64_t seed, uint32_t site, uint64_t e, float p) {
  return drop_keep_word(philox_word(drop_block(seed, site, e >> 2), (int)(e & 3)), p);
}

// one dropout site: p == 0 is the identity
struct DropSite {
  uint32_t site = 0;
  float p = 0.f, scale = 1.f;
};

// keep bits of the 4 x 4 block (positions t0 .. t0 + 3 of sequence bg, channels c0 .. c0 + 3): bit 4 i + cc = (t0 + i, c0 + cc)
__device__ __forceinline__ unsigned block_keep(uint64_t seed, const DropSite& d, int64_t bg, int C, int T, int c0, int t0) {
  if (d.p <= 0.f) return 0xffffu;
  unsigned bits = 0;
#pragma unroll
  for (int cc = 0; cc < 4; ++cc) {
    const uint64_t e0 = (uint64_t)((bg * C + c0 + cc) * (int64_t)T + t0);
    if ((T & 3) == 0) {
      const Philox4 v = drop_block(seed, d.site, e0 >> 2);
#pragma unroll
      for (int i = 0; i < 4; ++i) bits |= (unsigned)drop_keep_word(philox_word(v, i), d.p) << (4 * i + cc);
    } else {
      for (int i = 0; i < 4 && t0 + i < T; ++i) bits |= (unsigned)drop_keep(seed, d.site, e0 + i, d.p) << (4 * i + cc);
    }
  }
  return bits;
}

// dropout in place on rows [b][t] (T rows per sequence, C columns, pitch ld) of a (B', C, T) tensor of the reference; the
// first row is sequence b0 of the reference's batch
int launch_dropout(float* X, int64_t ld, int rows, int C, int T, int b0, uint64_t seed, const DropSite& d, hipStream_t st);

// the residual update of a block with its dropouts (replaces the G_RES epilogue while dropout is on):
//   out = R * (res_mask ? m : 1) + ls[c] * dp(b) * drop(H * (out_mask ? m : 1))
// dp(b) = (kept ? path.scale : 0), drawn from (seed, path.site, e = b); `out` may alias R (element-wise)
struct DropResArgs {
  float* out; int64_t ldo;
  const float* R; int64_t ldr;
  const float* H; int64_t ldh;
  const uint8_t* rowmask; int res_mask, out_mask;
  const float* ls;
  int rows, C, T, b0;
  uint64_t seed;
  DropSite drop, path;
};
int launch_drop_residual(const DropResArgs& a, hipStream_t st);

}  // namespace dcf
