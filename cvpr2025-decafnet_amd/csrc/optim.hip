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

__global__ __launch_bounds__(OPT_NT) void k_optim_sumsq(OptimTable tb, double* __restrict__ partial) {
  optim_sumsq_chunk<false>(tb, partial);
}

// one workgroup: thread t adds the partials t, t + NT, ... in order, then thread 0 adds the threads in order
__global__ __launch_bounds__(OPT_NT) void k_optim_norm_final(const double* __restrict__ partial, long long n_chunks, float max_norm,
                                                             float* __restrict__ norm_out, float* __restrict__ coef_out) {
  __shared__ double s_sum[OPT_NT];
  const double t = optim_sum_partials(partial, n_chunks, s_sum);
  if (threadIdx.x == 0) {
    float norm, coef;
    optim_norm_coef(t, max_norm, norm, coef);
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
  optim_adam_chunk<EMA>(tb, hs, coef_dev, beta);
}

}  // namespace dcf

extern "C" {

int dcf_optim_grad_norm(const dcf_optim_row* table, const int32_t* chunk_map, int32_t n_tensors, int64_t n_chunks, float max_norm,
                        float* norm_out, float* coef_out, void* stream) {
  if (dcf::optim_check_table("dcf_optim_grad_norm", table, chunk_map, n_tensors, n_chunks)) return -1;
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
  if (dcf::optim_check_table("dcf_optim_scale", table, chunk_map, n_tensors, n_chunks)) return -1;
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
  if (dcf::optim_check_table("dcf_optim_adam_step", table, chunk_map, n_tensors, n_chunks)) return -1;
  dcf::OptimGroups hs;
  if (dcf::optim_check_groups("dcf_optim_adam_step", groups, n_groups, hs)) return -1;
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
