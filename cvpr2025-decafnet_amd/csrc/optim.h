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

// The bodies of the table kernels, shared by optim.hip and optim_guard.hip (include/decafnet_hip_guard.h): one workgroup of OPT_NT
// threads owns one chunk of DCF_OPTIM_CHUNK elements of one tensor, which it finds through the chunk map and the row's chunk prefix.
struct OptimTable {
  const dcf_optim_row* rows;
  const int32_t* chunk_map;
};

// The sum of squares of the workgroup's chunk -> partial[blockIdx.x].  Lane t owns the elements [s * 1024 + 4 t, + 4) of the chunk for
// s = 0 .. OPT_SWEEPS-1, in both the 16-byte and the scalar path: the lane's fp32 sum runs over the same elements in the same order
// either way.  NULL_G: a row whose g is NULL counts as one without a gradient (the guarded export; the plain one reads the flag alone).
template <bool NULL_G>
__device__ __forceinline__ void optim_sumsq_chunk(OptimTable tb, double* __restrict__ partial) {
  __shared__ double s_wave[OPT_NT / 64];
  const dcf_optim_row r = tb.rows[__builtin_amdgcn_readfirstlane(tb.chunk_map[blockIdx.x])];
  float acc = 0.f;
  if (!(r.flags & DCF_OPTIM_NO_GRAD) && (!NULL_G || r.g != nullptr)) {
    const float* g = static_cast<const float*>(r.g);
    const bool al = aligned16(g);
    const long long base = ((long long)blockIdx.x - r.chunk0) * DCF_OPTIM_CHUNK;
#pragma unroll
    for (int s = 0; s < OPT_SWEEPS; ++s) {
      const long long i = base + s * OPT_STRIDE + threadIdx.x * OPT_VEC;
      if (i < r.n) acc = sumsq4(acc, load4(g, i, r.n, al));
    }
  }
  double d = (double)acc;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) d += __shfl_xor(d, o);      // a butterfly: every lane ends with the same sum, in a fixed order
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = d;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < OPT_NT / 64; ++w) t += s_wave[w];
    partial[blockIdx.x] = t;
  }
}

// The sum of the chunk partials in one workgroup: thread t adds the partials t, t + NT, ... in order, then thread 0 adds the threads
// in order.  The total is valid in thread 0 alone; s_sum holds OPT_NT doubles.
__device__ __forceinline__ double optim_sum_partials(const double* __restrict__ partial, long long n_chunks, double* s_sum) {
  double s = 0.0;
  for (long long i = threadIdx.x; i < n_chunks; i += OPT_NT) s += partial[i];
  s_sum[threadIdx.x] = s;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0)
    for (int i = 0; i < OPT_NT; ++i) t += s_sum[i];
  return t;
}

// the norm of a sum of squares and torch.nn.utils.clip_grad_norm_'s coefficient: clamp(max_norm / (norm + 1e-6), max = 1) in fp32; a
// NaN passes the clamp as it does there
__device__ __forceinline__ void optim_norm_coef(double sumsq, float max_norm, float& norm, float& coef) {
  norm = (float)sqrt(sumsq);
  coef = 1.f;
  if (max_norm > 0.f) {
    const float c = max_norm / (norm + 1e-6f);
    coef = c > 1.f ? 1.f : c;
  } else if (norm != norm) {
    coef = norm;
  }
}

// The sweeps of the workgroup's chunk of row r: the Adam / AdamW update where has_g, the EMA copy where has_e.  Shared by every update
// kernel (optim.hip, optim_guard.hip, optim_clock.hip).  `group_of()` yields the row's group record, uniform over the workgroup; it is
// a callable so that the record is read where it always was, after the addresses are looked at.
template <bool EMA, class GroupOf>
__device__ __forceinline__ void optim_adam_sweeps(const dcf_optim_row& r, bool has_g, bool has_e, GroupOf group_of,
                                                  const float* __restrict__ coef_dev, float beta) {
  float* p = static_cast<float*>(r.p);
  const float* g = static_cast<const float*>(r.g);
  float* m = static_cast<float*>(r.exp_avg);
  float* v = static_cast<float*>(r.exp_avg_sq);
  float* e = static_cast<float*>(r.ema);
  const bool al_p = aligned16(p), al_g = aligned16(g), al_m = aligned16(m), al_v = aligned16(v), al_e = aligned16(e);
  const dcf_optim_group h = group_of();
  const float coef = coef_dev ? *coef_dev : 1.f;
  const long long base = ((long long)blockIdx.x - r.chunk0) * DCF_OPTIM_CHUNK;
#pragma unroll
  for (int s = 0; s < OPT_SWEEPS; ++s) {
    const long long i = base + s * OPT_STRIDE + threadIdx.x * OPT_VEC;
    if (i >= r.n) break;
    f32x4 xp = load4(p, i, r.n, al_p);
    if (has_g) {
      const f32x4 xg = load4(g, i, r.n, al_g);
      f32x4 xm = load4(m, i, r.n, al_m);
      f32x4 xv = load4(v, i, r.n, al_v);
#pragma unroll
      for (int j = 0; j < OPT_VEC; ++j) {
        float ep = xp[j], em = xm[j], ev = xv[j];
        adam_elem(ep, xg[j], em, ev, h, coef);
        xp[j] = ep, xm[j] = em, xv[j] = ev;
      }
      store4(p, i, r.n, al_p, xp);
      store4(m, i, r.n, al_m, xm);
      store4(v, i, r.n, al_v, xv);
    }
    if (has_e) {
      f32x4 xe = load4(e, i, r.n, al_e);
#pragma unroll
      for (int j = 0; j < OPT_VEC; ++j) xe[j] = ema_elem(xp[j], xe[j], beta);
      store4(e, i, r.n, al_e, xe);
    }
  }
}

// The Adam / AdamW update of the workgroup's chunk, with the EMA copy when EMA.  GATED (the guarded export): `gate` points to one
// device word, the same for the whole grid; a non-zero word means return before anything is written.  Its load is issued with the
// chunk map's and waited for only after the row is there, so the gate costs one scalar load and no latency of its own.
template <bool EMA, bool GATED = false>
__device__ __forceinline__ void optim_adam_chunk(OptimTable tb, const OptimGroups& hs, const float* __restrict__ coef_dev, float beta,
                                                 const int32_t* __restrict__ gate = nullptr) {
  const int32_t closed = GATED ? *gate : 0;
  const dcf_optim_row r = tb.rows[__builtin_amdgcn_readfirstlane(tb.chunk_map[blockIdx.x])];
  const bool has_g = !(r.flags & DCF_OPTIM_NO_GRAD);
  const bool has_e = EMA && r.ema != nullptr;
  if (GATED && closed != 0) return;
  if (!has_g && !has_e) return;
  optim_adam_sweeps<EMA>(
      r, has_g, has_e,
      [&] { return hs.g[__builtin_amdgcn_readfirstlane(r.group) & (DCF_OPTIM_MAX_GROUPS - 1)]; },   // uniform: read from the kernel arguments
      coef_dev, beta);
}

// the argument checks every table export starts with; -1 with the message set
static inline int optim_check_table(const char* who, const dcf_optim_row* table, const int32_t* chunk_map, int32_t n_tensors, int64_t n_chunks) {
  DCF_CHECK(n_tensors >= 0 && n_chunks >= 0, "%s: negative count (n_tensors %d, n_chunks %lld)", who, (int)n_tensors, (long long)n_chunks);
  DCF_CHECK(n_chunks <= 0x7fffffffll, "%s: %lld chunks exceed one grid", who, (long long)n_chunks);
  DCF_CHECK(n_chunks == 0 || (table && chunk_map), "%s: null table", who);
  DCF_CHECK(n_chunks == 0 || n_tensors > 0, "%s: %lld chunks but no tensors", who, (long long)n_chunks);
  return 0;
}

// the by-value group array of an Adam launch, checked; -1 with the message set
static inline int optim_check_groups(const char* who, const dcf_optim_group* groups, int32_t n_groups, OptimGroups& hs) {
  DCF_CHECK(n_groups >= 0, "%s: negative count (n_groups %d)", who, (int)n_groups);
  DCF_CHECK(n_groups <= DCF_OPTIM_MAX_GROUPS, "%s: %d groups, at most %d", who, (int)n_groups, DCF_OPTIM_MAX_GROUPS);
  DCF_CHECK(n_groups == 0 || groups, "%s: null groups", who);
  hs = {};
  for (int i = 0; i < n_groups; ++i) {
    DCF_CHECK(groups[i].mode == DCF_OPTIM_ADAMW || groups[i].mode == DCF_OPTIM_ADAM, "%s: unknown mode %d in group %d", who,
              (int)groups[i].mode, i);
    hs.g[i] = groups[i];
  }
  return 0;
}

}  // namespace dcf
