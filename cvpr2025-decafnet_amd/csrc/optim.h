// The training update as multi-tensor kernels: gradient norm + clip coefficient, in-place gradient scaling, and the fused
// Adam / AdamW step with the EMA copy (csrc/optim.hip).  The table types are those of include/decafnet_hip.h (dcf_optim_row,
// dcf_optim_group); this header holds the element arithmetic, shared by the 16-byte and the scalar path of every kernel so that a
// value never depends on the path that moved it.
#pragma once
#include "../../include/decafnet_hip.h"
#include "common.h"

namespace dcf {

static_assert(sizeof(dcf_optim_row) == 64, "dcf_optim_row is 64 bytes: the host builds it as a packed record");
static_assert(sizeof(dcf_optim_group) == 40, "dcf_optim_group is 40 bytes");

constexpr int OPT_NT = 256;                         // threads per workgroup
constexpr int OPT_VEC = 4;                          // fp32 per 16-byte access
constexpr int OPT_STRIDE = OPT_NT * OPT_VEC;        // elements one sweep of the workgroup covers
constexpr int OPT_SWEEPS = DCF_OPTIM_CHUNK / OPT_STRIDE;
static_assert(DCF_OPTIM_CHUNK % OPT_STRIDE == 0, "a chunk is a whole number of workgroup sweeps");

struct OptimGroups {
  dcf_optim_group g[DCF_OPTIM_MAX_GROUPS];
};

// No contraction in the element arithmetic: every product and sum below rounds once, in the order written, in both paths.
// The sum of squares of a lane's elements uses an explicit fma chain.
__device__ __forceinline__ float sumsq4(float acc, f32x4 x) {
  acc = __fmaf_rn(x[0], x[0], acc);
  acc = __fmaf_rn(x[1], x[1], acc);
  acc = __fmaf_rn(x[2], x[2], acc);
  acc = __fmaf_rn(x[3], x[3], acc);
  return acc;
}

// one element of the Adam / AdamW update (torch/optim/adam.py, the single-tensor form); g is the stored gradient
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, const dcf_optim_group& h, float coef) {
#pragma clang fp contract(off)
  g = g * coef;
  if (h.mode == DCF_OPTIM_ADAMW) p = p * (1.f - h.lr * h.weight_decay);
  else g = g + h.weight_decay * p;
  m = h.b1 * m + h.one_minus_b1 * g;
  v = h.b2 * v + h.one_minus_b2 * (g * g);
  const float denom = sqrtf(v) / h.sqrt_bc2 + h.eps;
  p = p - (h.lr / h.bc1) * (m / denom);
}

// torch's lerp(p, ema, beta) (ATen/native/Lerp.h): two branches, so that beta = 0 gives p's bits and beta = 1 ema's
__device__ __forceinline__ float ema_elem(float p, float e, float beta) {
#pragma clang fp contract(off)
  const float d = e - p;
  return beta < 0.5f ? p + beta * d : e - d * (1.f - beta);
}

// Four consecutive elements at index i of a tensor of n elements: one 16-byte access when the tensor's address is 16-byte aligned and
// all four are inside, else one access per element that is inside (the others read 0 and are not written).
__device__ __forceinline__ f32x4 load4(const float* __restrict__ base, long long i, long long n, bool aligned) {
  if (aligned && i + OPT_VEC <= n) return *reinterpret_cast<const f32x4*>(base + i);
  f32x4 r = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < OPT_VEC; ++j)
    if (i + j < n) r[j] = base[i + j];
  return r;
}
__device__ __forceinline__ void store4(float* __restrict__ base, long long i, long long n, bool aligned, f32x4 x) {
  if (aligned && i + OPT_VEC <= n) {
    *reinterpret_cast<f32x4*>(base + i) = x;
    return;
  }
#pragma unroll
  for (int j = 0; j < OPT_VEC; ++j)
    if (i + j < n) base[i + j] = x[j];
}
__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace dcf
