// The training update (libs/worker_v2.py:320-325: clip_grad_norm_, optimizer.step(), _ema_update) as three multi-tensor kernels over
// a device table of parameter tensors (include/decafnet_hip.h: dcf_optim_row, the chunk map).  One workgroup owns one chunk of
// DCF_OPTIM_CHUNK elements of one tensor: it reads its tensor index from the chunk map and its position in the tensor from the row's
// chunk prefix, so nothing scans the table.  fp32 on the vector ALU; no atomics; sums across lanes, waves and chunks are fp64 in a
// fixed order, so the norm has the same bits whatever ran where.
//
// The update is HBM bound: p, g, exp_avg, exp_avg_sq and ema read, p, exp_avg, exp_avg_sq and ema written: 36 bytes per element
// (28 without the EMA copy), all through 16-byte accesses of which every lane has DCF_OPTIM_CHUNK / 1024 per array in flight.
#include "optim.h"

namespace dcf {

struct OptimTable {
  const dcf_optim_row* rows;
  const int32_t* chunk_map;
};

// lane t of the workgroup owns the elements [s * 1024 + 4 t, + 4) of the chunk for s = 0 .. OPT_SWEEPS-1, in both the 16-byte and
// the scalar path: the lane's fp32 sum runs over the same elements in the same order either way
__global__ __launch_bounds__(OPT_NT) void k_optim_sumsq(OptimTable tb, double* __restrict__ partial) {
  __shared__ double s_wave[OPT_NT / 64];
  const dcf_optim_row r = tb.rows[__builtin_amdgcn_readfirstlane(tb.chunk_map[blockIdx.x])];
  float acc = 0.f;
  if (!(r.flags & DCF_OPTIM_NO_GRAD)) {
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

// one workgroup: thread t adds the partials t, t + NT, ... in order, then thread 0 adds the threads in order
__global__ __launch_bounds__(OPT_NT) void k_optim_norm_final(const double* __restrict__ partial, long long n_chunks, float max_norm,
                                                             float* __restrict__ norm_out, float* __restrict__ coef_out) {
  __shared__ double s_sum[OPT_NT];
  double s = 0.0;
  for (long long i = threadIdx.x; i < n_chunks; i += OPT_NT) s += partial[i];
  s_sum[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < OPT_NT; ++i) t += s_sum[i];
    const float norm = (float)sqrt(t);
    float coef = 1.f;
    if (max_norm > 0.f) {
      // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max = 1) in fp32; a NaN passes the clamp as it does there
      const float c = max_norm / (norm + 1e-6f);
      coef = c > 1.f ? 1.f : c;
    } else if (norm != norm) {
      coef = norm;
    }
    if (norm_out) *norm_out = norm;
    if (coef_out) *coef_out = coef;
  }
}

__global__ __launch_bounds__(OPT_NT) void k_optim_scale(OptimTable tb, const float* __restrict__ scale) {
  const dcf_optim_row r = tb.rows[__builtin_amdgcn_readfirstlane(tb.chunk_map[blockIdx.x])];
  if (r.flags & DCF_OPTIM_NO_GRAD) return;
  const float c = *scale;
  float* g = static_cast<float*>(r.g);
  const bool al = aligned16(g);
  const long long base = ((long long)blockIdx.x - r.chunk0) * DCF_OPTIM_CHUNK;
#pragma unroll
  for (int s = 0; s < OPT_SWEEPS; ++s) {
    const long long i = base + s * OPT_STRIDE + threadIdx.x * OPT_VEC;
    if (i >= r.n) break;
    f32x4 x = load4(g, i, r.n, al);
#pragma unroll
    for (int j = 0; j < OPT_VEC; ++j) x[j] = x[j] * c;
    store4(g, i, r.n, al, x);
  }
}

template <bool EMA>
__global__ __launch_bounds__(OPT_NT) void k_optim_adam(OptimTable tb, OptimGroups hs, const float* __restrict__ coef_dev, float beta) {
  const dcf_optim_row r = tb.rows[__builtin_amdgcn_readfirstlane(tb.chunk_map[blockIdx.x])];
  const bool has_g = !(r.flags & DCF_OPTIM_NO_GRAD);
  const bool has_e = EMA && r.ema != nullptr;
  if (!has_g && !has_e) return;
  float* p = static_cast<float*>(r.p);
  const float* g = static_cast<const float*>(r.g);
  float* m = static_cast<float*>(r.exp_avg);
  float* v = static_cast<float*>(r.exp_avg_sq);
  float* e = static_cast<float*>(r.ema);
  const bool al_p = aligned16(p), al_g = aligned16(g), al_m = aligned16(m), al_v = aligned16(v), al_e = aligned16(e);
  const dcf_optim_group h = hs.g[__builtin_amdgcn_readfirstlane(r.group) & (DCF_OPTIM_MAX_GROUPS - 1)];   // uniform: read from the kernel arguments
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

static int check_table(const char* who, const dcf_optim_row* table, const int32_t* chunk_map, int32_t n_tensors, int64_t n_chunks) {
  DCF_CHECK(n_tensors >= 0 && n_chunks >= 0, "%s: negative count (n_tensors %d, n_chunks %lld)", who, (int)n_tensors, (long long)n_chunks);
  DCF_CHECK(n_chunks <= 0x7fffffffll, "%s: %lld chunks exceed one grid", who, (long long)n_chunks);
  DCF_CHECK(n_chunks == 0 || (table && chunk_map), "%s: null table", who);
  DCF_CHECK(n_chunks == 0 || n_tensors > 0, "%s: %lld chunks but no tensors", who, (long long)n_chunks);
  return 0;
}

}  // namespace dcf

extern "C" {

int dcf_optim_grad_norm(const dcf_optim_row* table, const int32_t* chunk_map, int32_t n_tensors, int64_t n_chunks, float max_norm,
                        float* norm_out, float* coef_out, void* stream) {
  if (dcf::check_table("dcf_optim_grad_norm", table, chunk_map, n_tensors, n_chunks)) return -1;
  DCF_CHECK(norm_out || coef_out, "dcf_optim_grad_norm: no output");
  hipStream_t st = (hipStream_t)stream;
  dcf::StreamScratch sc(st);
  double* partial = nullptr;
  if (n_chunks > 0 && sc.take(&partial, (size_t)n_chunks)) return -1;
  hipError_t e = hipSuccess;
  {
    dcf::ProfScope prof("optim_grad_norm", st, 0.0, 4.0 * (double)n_chunks * DCF_OPTIM_CHUNK);
    if (n_chunks > 0) {
      hipLaunchKernelGGL(dcf::k_optim_sumsq, dim3((unsigned)n_chunks), dim3(dcf::OPT_NT), 0, st, dcf::OptimTable{table, chunk_map}, partial);
      e = hipGetLastError();
    }
    if (e == hipSuccess) {
      hipLaunchKernelGGL(dcf::k_optim_norm_final, dim3(1), dim3(dcf::OPT_NT), 0, st, (const double*)partial, (long long)n_chunks, max_norm,
                         norm_out, coef_out);
      e = hipGetLastError();
    }
  }
  DCF_HIP(e);                  // a launch error first: it is the cause, a failed release only follows from it
  return sc.end(0);
}

int dcf_optim_scale(const dcf_optim_row* table, const int32_t* chunk_map, int32_t n_tensors, int64_t n_chunks, const float* scale,
                    void* stream) {
  if (dcf::check_table("dcf_optim_scale", table, chunk_map, n_tensors, n_chunks)) return -1;
  DCF_CHECK(scale, "dcf_optim_scale: null scale");
  if (n_chunks == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  dcf::ProfScope prof("optim_scale", st, 0.0, 8.0 * (double)n_chunks * DCF_OPTIM_CHUNK);
  hipLaunchKernelGGL(dcf::k_optim_scale, dim3((unsigned)n_chunks), dim3(dcf::OPT_NT), 0, st, dcf::OptimTable{table, chunk_map}, scale);
  DCF_HIP(hipGetLastError());
  return 0;
}

int dcf_optim_adam_step(const dcf_optim_row* table, const int32_t* chunk_map, int32_t n_tensors, int64_t n_chunks,
                        const dcf_optim_group* groups, int32_t n_groups, const float* coef, int32_t with_ema, float ema_beta, void* stream) {
  if (dcf::check_table("dcf_optim_adam_step", table, chunk_map, n_tensors, n_chunks)) return -1;
  DCF_CHECK(n_groups >= 0, "dcf_optim_adam_step: negative count (n_groups %d)", (int)n_groups);
  DCF_CHECK(n_groups <= DCF_OPTIM_MAX_GROUPS, "dcf_optim_adam_step: %d groups, at most %d", (int)n_groups, DCF_OPTIM_MAX_GROUPS);
  DCF_CHECK(n_groups == 0 || groups, "dcf_optim_adam_step: null groups");
  dcf::OptimGroups hs = {};
  for (int i = 0; i < n_groups; ++i) {
    DCF_CHECK(groups[i].mode == DCF_OPTIM_ADAMW || groups[i].mode == DCF_OPTIM_ADAM, "dcf_optim_adam_step: unknown mode %d in group %d",
              (int)groups[i].mode, i);
    hs.g[i] = groups[i];
  }
  // a row's group index is read on the device: the rows past n_groups of the by-value array are zero and never named by a valid table
  if (n_chunks == 0) return 0;
  DCF_CHECK(n_groups > 0, "dcf_optim_adam_step: %lld chunks but no groups", (long long)n_chunks);
  hipStream_t st = (hipStream_t)stream;
  dcf::ProfScope prof("optim_adam_step", st, 0.0, (with_ema ? 36.0 : 28.0) * (double)n_chunks * DCF_OPTIM_CHUNK);
  const dcf::OptimTable tb{table, chunk_map};
  if (with_ema) hipLaunchKernelGGL(dcf::k_optim_adam<true>, dim3((unsigned)n_chunks), dim3(dcf::OPT_NT), 0, st, tb, hs, coef, ema_beta);
  else hipLaunchKernelGGL(dcf::k_optim_adam<false>, dim3((unsigned)n_chunks), dim3(dcf::OPT_NT), 0, st, tb, hs, coef, ema_beta);
  DCF_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
