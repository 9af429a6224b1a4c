// Building blocks shared by the gradient kernels (*_grad.hip): the arithmetic that "same bits on every run" rests on, one
// definition each.
#pragma once
#include "common.h"

namespace dcf {

__device__ __forceinline__ f32x4 ld4(const float* __restrict__ p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* __restrict__ p, const f32x4& v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ f32x4 zero4() { return f32x4{0.f, 0.f, 0.f, 0.f}; }

// the 4-channel partial of a dot product with its contraction written out, so that two kernels that form the same product (the
// query-side and the key-side kernel of an attention backward) get the same bits for the same operands whatever the compiler would
// have fused
__device__ __forceinline__ float dotp(const f32x4& a, const f32x4& b) {
  return __builtin_fmaf(a.x, b.x, a.y * b.y) + __builtin_fmaf(a.z, b.z, a.w * b.w);
}

// exp(x), x <= 0 (or barely above): v_exp_f32 of the rounded product x * log2(e), times 1 + ln 2 * (what the rounding of the product
// and of the constant dropped).  The forward's one-instruction form has a relative error of |x| 2^-24; the gradient rule leaves
// ~2^-20 of the largest element for everything, and dS = p (dP - delta) is a difference, so the residual is carried (3 more
// vector instructions per score and head).  Scores below -1e5 (the -1e4 of a padded key among them: 0 either way) are clamped so that
// the product stays finite.
__device__ __forceinline__ float exp_res(float x) {
  constexpr float L2E = 1.44269504088896340736f, L2E_LO = 1.925963033500003e-8f, LN2 = 0.69314718055994530942f;
  x = fmaxf(x, -1e5f);
  const float t = x * L2E;
  const float r = __builtin_fmaf(x, L2E_LO, __builtin_fmaf(x, L2E, -t));
  const float e = __builtin_amdgcn_exp2f(t);
  return __builtin_fmaf(e, r * LN2, e);
}

// ---- the fixed-order blocked sum of slice partials ------------------------------------------------
// sum += sum_s part[s * stride + i], s < nparts, in one order that depends on nparts alone: a balanced tree over 8 consecutive
// parts (a missing part counts as 0), a balanced tree over 8 of those, then the groups of 64 added in ascending order -- nine
// roundings on the path of a part at 512 parts instead of 511, no atomics, and a slicing that is a constant of the operator, not
// of the device: the same bits on every run.
//
// The loop is a macro that a reduce kernel expands in place (`float sum = 0.f; DCF_BLOCKED_SUM(sum, ...);`), and blocked_sum()
// below is the same text as a device function.  The kernels whose loop was written in place keep it in place: inlined from a
// function, the loop's exit block lands behind the loop, the compiler lays the same instructions out in another order, and
// k_cg_reduce measured 2 us slower per call at 510 parts (profiles/grad_common.md).
//
// DCF_BLOCKED_SUM_ROLLED is the same tree, operation for operation: the second level runs as a loop that keeps the three pending
// subtree sums in registers (s0: one tree of 8, s1: two, s2: four or eight) instead of holding all eight.  It has 8 loads in
// flight where the unrolled form has 64; k_fg_reduce (front_grad.hip) uses it because the unrolled form's scalar address
// arithmetic did not fit the scalar registers there.
__device__ __forceinline__ float tree_sum8(const float (&v)[8]) {
  return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
}

#define DCF_BLOCKED_SUM(sum, part, nparts, stride, i)                                      \
  for (int g2_ = 0; g2_ < (nparts); g2_ += 64) {                                           \
    float l1_[8];                                                                          \
    _Pragma("unroll") for (int u_ = 0; u_ < 8; ++u_) {                                     \
      float v_[8];                                                                         \
      _Pragma("unroll") for (int t_ = 0; t_ < 8; ++t_) {                                   \
        const int sl_ = g2_ + 8 * u_ + t_;                                                 \
        v_[t_] = sl_ < (nparts) ? (part)[(int64_t)sl_ * (stride) + (i)] : 0.f;             \
      }                                                                                    \
      l1_[u_] = tree_sum8(v_);                                                             \
    }                                                                                      \
    (sum) += tree_sum8(l1_);                                                               \
  }

#define DCF_BLOCKED_SUM_ROLLED(sum, part, nparts, stride, i)                               \
  {                                                                                        \
    const float* __restrict__ pp_ = (part) + (i);                                          \
    for (int g2_ = 0; g2_ < (nparts); g2_ += 64) {                                         \
      float s0_ = 0.f, s1_ = 0.f, s2_ = 0.f;                                               \
      _Pragma("unroll 1") for (int u_ = 0; u_ < 8; ++u_) {                                 \
        float v_[8];                                                                       \
        _Pragma("unroll") for (int t_ = 0; t_ < 8; ++t_) {                                 \
          const int sl_ = g2_ + 8 * u_ + t_;                                               \
          v_[t_] = sl_ < (nparts) ? pp_[(int64_t)sl_ * (stride)] : 0.f;                    \
        }                                                                                  \
        float x_ = tree_sum8(v_);                                                          \
        if (!(u_ & 1)) { s0_ = x_; continue; }                                             \
        x_ = s0_ + x_;                                                                     \
        if (!(u_ & 2)) { s1_ = x_; continue; }                                             \
        x_ = s1_ + x_;                                                                     \
        s2_ = (u_ & 4) ? s2_ + x_ : x_;                                                    \
      }                                                                                    \
      (sum) += s2_;                                                                        \
    }                                                                                      \
  }

__device__ __forceinline__ float blocked_sum(const float* __restrict__ part, int nparts, int64_t stride, int i) {
  float sum = 0.f;
  DCF_BLOCKED_SUM(sum, part, nparts, stride, i);
  return sum;
}

}  // namespace dcf
