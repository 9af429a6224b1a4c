// The guarded training update (include/decafnet_hip_guard.h): the gradient norm of optim.hip whose one-workgroup final pass also
// decides whether the step may be applied, and the Adam / AdamW / EMA update that reads the decision and returns where it says skip.
// The chunk kernels are the bodies of optim.h, shared with optim.hip: the same sums in the same order, the same element arithmetic.
// The decision never leaves the device: dcf_guard_state is written by thread 0 of the final pass with ordinary stores and read by
// every workgroup of the update through one uniform load.
#include "../../include/decafnet_hip_guard.h"
#include "conv_grad.h"
#include "optim.h"

namespace dcf {

static_assert(sizeof(dcf_guard_state) == 48, "dcf_guard_state is 48 bytes: the host builds it as a packed record");

__global__ __launch_bounds__(OPT_NT) void k_guard_sumsq(OptimTable tb, double* __restrict__ partial) {
  optim_sumsq_chunk<true>(tb, partial);
}

__device__ __forceinline__ bool non_finite(double x) { return !(__builtin_fabs(x) <= 1.7976931348623157e308); }

// One workgroup.  The sum is optim_sum_partials, as in k_optim_norm_final.  Which rows are bad is only looked up when the total is
// not finite (uniform after the barrier): thread t then walks the rows t, t + NT, ... and the chunks of each, and the workgroup
// counts the bad rows and takes the lowest with integer operations on LDS.
__global__ __launch_bounds__(OPT_NT) void k_guard_norm_final(const double* __restrict__ partial, long long n_chunks,
                                                             const dcf_optim_row* __restrict__ rows, int n_tensors, float max_norm,
                                                             float* __restrict__ norm_out, float* __restrict__ coef_out,
                                                             dcf_guard_state* __restrict__ state, unsigned* __restrict__ conv_word) {
  __shared__ double s_sum[OPT_NT];
  __shared__ int s_any, s_first, s_count;
  // The partials are sums of squares: none is negative, and fp64 cannot overflow on 2^31 of them (each at most 256 x 3.4e38), so the
  // total is non-finite exactly when a partial is.
  const double t = optim_sum_partials(partial, n_chunks, s_sum);
  if (threadIdx.x == 0) s_any = non_finite(t), s_first = 0x7fffffff, s_count = 0;
  __syncthreads();
  if (s_any) {
    for (int r = threadIdx.x; r < n_tensors; r += OPT_NT) {
      const dcf_optim_row row = rows[r];
      if ((row.flags & DCF_OPTIM_NO_GRAD) || row.g == nullptr) continue;
      const long long c1 = row.chunk0 + (row.n + DCF_OPTIM_CHUNK - 1) / DCF_OPTIM_CHUNK;
      bool b = false;
      for (long long c = row.chunk0 < 0 ? 0 : row.chunk0; c < c1 && c < n_chunks; ++c) b |= non_finite(partial[c]);
      if (b) {
        atomicAdd(&s_count, 1);
        atomicMin(&s_first, r);
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    float norm, coef;
    optim_norm_coef(t, max_norm, norm, coef);
    unsigned word = 0u;
    if (conv_word) {
      word = *conv_word;
      *conv_word = 0u;
    }
    const bool skip = s_any != 0 || word != 0u;
    if (skip) coef = 0.f;
    if (norm_out) *norm_out = norm;
    if (coef_out) *coef_out = coef;
    const long long applied = state->applied, skipped = state->skipped;
    state->verdict = skip ? DCF_GUARD_SKIP : DCF_GUARD_APPLY;
    if (skip) {
      state->first_bad_row = s_count ? s_first : -1;
      state->n_bad_rows = s_count;
      state->conv_flag = (int)word;
      state->last_skipped_attempt = applied + skipped;
      state->skipped = skipped + 1;
    } else {
      state->applied = applied + 1;
    }
  }
}

template <bool EMA>
__global__ __launch_bounds__(OPT_NT) void k_guard_adam(OptimTable tb, OptimGroups hs, const float* __restrict__ coef_dev,
                                                       const dcf_guard_state* __restrict__ state, float beta) {
  static_assert(DCF_GUARD_APPLY == 0, "the gate of optim_adam_chunk is open at 0");
  optim_adam_chunk<EMA, true>(tb, hs, coef_dev, beta, &state->verdict);     // one word, the same for the whole grid
}

}  // namespace dcf

extern "C" {

int dcf_guard_ext_version(void) { return DCF_GUARD_EXT_VERSION; }

int dcf_guard_grad_norm(const dcf_optim_row* table, const int32_t* chunk_map, int32_t n_tensors, int64_t n_chunks, float max_norm,
                        float* norm_out, float* coef_out, dcf_guard_state* state, void* stream) {
  if (dcf::optim_check_table("dcf_guard_grad_norm", table, chunk_map, n_tensors, n_chunks)) return -1;
  DCF_CHECK(state, "dcf_guard_grad_norm: null state");
  DCF_CHECK((reinterpret_cast<uintptr_t>(state) & 7) == 0, "dcf_guard_grad_norm: the state record must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  unsigned* word = dcf::cg_guard_word(state);              // nullptr unless this state is the armed one
  dcf::StreamScratch sc(st);
  double* partial = nullptr;
  if (n_chunks > 0 && sc.take(&partial, (size_t)n_chunks)) return -1;
  hipError_t e = hipSuccess;
  {
    dcf::ProfScope prof("guard_grad_norm", st, 0.0, 4.0 * (double)n_chunks * DCF_OPTIM_CHUNK);
    if (n_chunks > 0) {
      hipLaunchKernelGGL(dcf::k_guard_sumsq, dim3((unsigned)n_chunks), dim3(dcf::OPT_NT), 0, st, dcf::OptimTable{table, chunk_map}, partial);
      e = hipGetLastError();
    }
    if (e == hipSuccess) {
      hipLaunchKernelGGL(dcf::k_guard_norm_final, dim3(1), dim3(dcf::OPT_NT), 0, st, (const double*)partial, (long long)n_chunks, table,
                         (int)(n_chunks > 0 ? n_tensors : 0), max_norm, norm_out, coef_out, state, word);
      e = hipGetLastError();
    }
  }
  DCF_HIP(e);                  // a launch error first: it is the cause, a failed release only follows from it
  return sc.end(0);
}

int dcf_guard_adam_step(const dcf_optim_row* table, const int32_t* chunk_map, int32_t n_tensors, int64_t n_chunks,
                        const dcf_optim_group* groups, int32_t n_groups, const float* coef, const dcf_guard_state* state,
                        int32_t with_ema, float ema_beta, void* stream) {
  if (dcf::optim_check_table("dcf_guard_adam_step", table, chunk_map, n_tensors, n_chunks)) return -1;
  DCF_CHECK(state, "dcf_guard_adam_step: null state");
  dcf::OptimGroups hs;
  if (dcf::optim_check_groups("dcf_guard_adam_step", groups, n_groups, hs)) return -1;
  if (n_chunks == 0) return 0;
  DCF_CHECK(n_groups > 0, "dcf_guard_adam_step: %lld chunks but no groups", (long long)n_chunks);
  hipStream_t st = (hipStream_t)stream;
  dcf::ProfScope prof("guard_adam_step", st, 0.0, (with_ema ? 36.0 : 28.0) * (double)n_chunks * DCF_OPTIM_CHUNK);
  const dcf::OptimTable tb{table, chunk_map};
  if (with_ema) hipLaunchKernelGGL(dcf::k_guard_adam<true>, dim3((unsigned)n_chunks), dim3(dcf::OPT_NT), 0, st, tb, hs, coef, state, ema_beta);
  else hipLaunchKernelGGL(dcf::k_guard_adam<false>, dim3((unsigned)n_chunks), dim3(dcf::OPT_NT), 0, st, tb, hs, coef, state, ema_beta);
  DCF_HIP(hipGetLastError());
  return 0;
}

int dcf_guard_arm(const dcf_guard_state* state, void* stream) {
  (void)stream;                // the word is allocated and zeroed synchronously the first time; nothing is queued
  DCF_CHECK(state, "dcf_guard_arm: null state");
  return dcf::cg_guard_arm(state);
}

int dcf_guard_disarm(void* stream) { return dcf::cg_guard_disarm((hipStream_t)stream); }

}  // extern "C"
