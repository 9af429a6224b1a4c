// The device-side pieces of a fit on several ranks (include/decafnet_hip_fit.h).
//
// dcf_op_loss_table_mean: what Evaluator._calc_loss and Evaluator.run make of the per-query losses -- the division by max(n_pos, 1),
// the NaN-skipping mean per video, the plain mean over the videos -- for a table of dcf_point_objective rows that never left the
// device.  One lane per video walks that video's rows in query order; one workgroup then adds the per-video values in an order
// that depends on V alone (lane-strided sums, a halving tree in LDS).  The fp32 divisions are __fdiv_rn and this file is compiled
// with -ffp-contract=off, like eval_metric.hip: every operation is rounded on its own, as the restatement of tests/eval_loss_ref.py
// rounds it.  No atomics.
//
// dcf_guard_word_publish / dcf_guard_word_merge: one thread each, between the armed guard's conv-gradient word (conv_grad.h) and a
// float that rides on the step's loss-norm all-reduce.
#include "../../include/decafnet_hip_fit.h"
#include "common.h"
#include "conv_grad.h"

namespace dcf {

constexpr int FIT_NT = 256;

__device__ __forceinline__ double fit_qnan() { return __longlong_as_double(0x7ff8000000000000ll); }

__global__ __launch_bounds__(FIT_NT) void k_loss_per_video(const float* __restrict__ rows, const long long* __restrict__ offsets, int V,
                                                           double* __restrict__ per_video) {
  const long long v = (long long)blockIdx.x * FIT_NT + threadIdx.x;
  if (v >= V) return;
  const long long q0 = offsets[v], q1 = offsets[v + 1];
  double s_cls = 0.0, s_reg = 0.0;
  long long n_cls = 0, n_reg = 0;
  for (long long q = q0; q < q1; ++q) {
    const float focal2 = rows[4 * q + 1], iou = rows[4 * q + 2], n_pos = rows[4 * q + 3];
    const float norm = n_pos < 1.f ? 1.f : n_pos;                  // torch.clamp(min=1): a NaN stays
    const float cls = __fdiv_rn(focal2, norm), reg = __fdiv_rn(iou, norm);
    if (cls == cls) { s_cls = __dadd_rn(s_cls, (double)cls); ++n_cls; }
    if (reg == reg) { s_reg = __dadd_rn(s_reg, (double)reg); ++n_reg; }
  }
  per_video[2 * v] = n_cls ? __ddiv_rn(s_cls, (double)n_cls) : fit_qnan();
  per_video[2 * v + 1] = n_reg ? __ddiv_rn(s_reg, (double)n_reg) : fit_qnan();
}

// One workgroup.  Lane t adds the videos t, t + 256, ... in ascending order, then the lanes meet in a halving tree.
__global__ __launch_bounds__(FIT_NT) void k_loss_over_videos(const double* __restrict__ per_video, int V, double* __restrict__ out2) {
  __shared__ double s[2][FIT_NT];
  const int t = threadIdx.x;
  double a = 0.0, b = 0.0;
  for (int v = t; v < V; v += FIT_NT) {
    a = __dadd_rn(a, per_video[2 * v]);
    b = __dadd_rn(b, per_video[2 * v + 1]);
  }
  s[0][t] = a;
  s[1][t] = b;
  __syncthreads();
  for (int h = FIT_NT / 2; h >= 1; h >>= 1) {
    if (t < h) {
      s[0][t] = __dadd_rn(s[0][t], s[0][t + h]);
      s[1][t] = __dadd_rn(s[1][t], s[1][t + h]);
    }
    __syncthreads();
  }
  if (t < 2) out2[t] = __ddiv_rn(s[t][0], (double)V);
}

__global__ void k_guard_word_publish(const unsigned* __restrict__ word, float* __restrict__ slot) { *slot = *word != 0u ? 1.f : 0.f; }

__global__ void k_guard_word_merge(unsigned* __restrict__ word, const float* __restrict__ slot) {
  if (!(*slot == 0.f)) atomicOr(word, (unsigned)DCF_GUARD_REMOTE);
}

}  // namespace dcf

extern "C" {

int dcf_fit_ext_version(void) { return DCF_FIT_EXT_VERSION; }

int dcf_op_loss_table_mean(const float* rows, const int64_t* offsets, int32_t V, double* per_video, double* out2, void* stream) {
  const char* who = "dcf_op_loss_table_mean";
  DCF_CHECK(rows && offsets && out2, "%s: null %s", who, !rows ? "rows" : !offsets ? "offsets" : "out2");
  DCF_CHECK(V >= 1, "%s: V %d (>= 1)", who, (int)V);
  DCF_CHECK(reinterpret_cast<uintptr_t>(rows) % 4 == 0, "%s: rows not aligned to 4 bytes", who);
  DCF_CHECK(reinterpret_cast<uintptr_t>(offsets) % 8 == 0 && reinterpret_cast<uintptr_t>(per_video) % 8 == 0 &&
                reinterpret_cast<uintptr_t>(out2) % 8 == 0,
            "%s: offsets / per_video / out2 not aligned to 8 bytes", who);
  hipStream_t st = (hipStream_t)stream;
  dcf::StreamScratch sc(st);
  if (per_video == nullptr && sc.take(&per_video, (size_t)V * 2)) return -1;
  hipError_t e = hipSuccess;
  {
    // the algorithmic traffic: the offsets and the per-video pairs, written and read once (the rows are known on the device only)
    dcf::ProfScope prof("loss_table_mean", st, 0.0, 40.0 * (double)V + 16.0);
    const unsigned grid = (unsigned)(((long long)V + dcf::FIT_NT - 1) / dcf::FIT_NT);
    hipLaunchKernelGGL(dcf::k_loss_per_video, dim3(grid), dim3(dcf::FIT_NT), 0, st, rows, reinterpret_cast<const long long*>(offsets), (int)V,
                       per_video);
    e = hipGetLastError();
    if (e == hipSuccess) {
      hipLaunchKernelGGL(dcf::k_loss_over_videos, dim3(1), dim3(dcf::FIT_NT), 0, st, (const double*)per_video, (int)V, out2);
      e = hipGetLastError();
    }
  }
  DCF_HIP(e);                  // a launch error first: it is the cause, a failed release only follows from it
  return sc.end(0);
}

static int fit_word(const char* who, const dcf_guard_state* state, const float* slot, unsigned** word) {
  DCF_CHECK(state && slot, "%s: null %s", who, !state ? "state" : "slot");
  DCF_CHECK(reinterpret_cast<uintptr_t>(slot) % 4 == 0, "%s: slot not aligned to 4 bytes", who);
  *word = dcf::cg_guard_word(state);
  DCF_CHECK(*word, "%s: the state is not the armed guard's (dcf_guard_arm first): the conv-gradient word belongs to the armed guard alone", who);
  return 0;
}

int dcf_guard_word_publish(const dcf_guard_state* state, float* slot, void* stream) {
  unsigned* word = nullptr;
  if (fit_word("dcf_guard_word_publish", state, slot, &word)) return -1;
  hipLaunchKernelGGL(dcf::k_guard_word_publish, dim3(1), dim3(1), 0, (hipStream_t)stream, (const unsigned*)word, slot);
  DCF_HIP(hipGetLastError());
  return 0;
}

int dcf_guard_word_merge(const dcf_guard_state* state, const float* slot, void* stream) {
  unsigned* word = nullptr;
  if (fit_word("dcf_guard_word_merge", state, slot, &word)) return -1;
  hipLaunchKernelGGL(dcf::k_guard_word_merge, dim3(1), dim3(1), 0, (hipStream_t)stream, word, slot);
  DCF_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
