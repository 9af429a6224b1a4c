// The training log's meters in device memory (include/decafnet_hip_steplog.h).
//
// dcf_op_steplog_add: the K loss scalars of a step, each in an allocation of its own, into a (K, 6) table of doubles and K + 1
// counters.  The pointers travel by value with the launch; one lane per key, one more for the step count.  Plain loads and stores:
// a table belongs to one stream, and the stream's order is the order of the sums.
// dcf_op_steplog_flush: the table turned into the numbers of a log line and emptied, by the same lanes in the same launch.
//
// A handful of scalars: nothing here has a roofline.  The additions and divisions are __dadd_rn / __ddiv_rn, each rounded on its own,
// as the restatement of tests/steplog_ref.py rounds them.
#include "../../include/decafnet_hip_steplog.h"
#include "common.h"

namespace dcf {

constexpr int SL_NT = 64;                                     // one wavefront: K + 1 <= 17 lanes work
constexpr int SL_COLS = DCF_STEPLOG_COLS;
static_assert(DCF_STEPLOG_MAX_KEYS + 1 <= SL_NT, "one lane per key and one for the steps");

struct SteplogVals {
  const float* p[DCF_STEPLOG_MAX_KEYS];
};

__device__ __forceinline__ double sl_qnan() { return __longlong_as_double(0x7ff8000000000000ll); }

// IEEE 754 leaves sign and payload of a NaN that an operation makes to the implementation: the tables hold the one quiet NaN
__device__ __forceinline__ double sl_canon(double v) { return v != v ? sl_qnan() : v; }

// |v| < inf: false for both infinities and for a NaN
__device__ __forceinline__ bool sl_finite(double v) { return fabs(v) < __longlong_as_double(0x7ff0000000000000ll); }

__global__ __launch_bounds__(SL_NT) void k_steplog_add(SteplogVals vals, int K, double* __restrict__ stats, long long* __restrict__ counts) {
  const int k = threadIdx.x;
  if (k == K) counts[K] = counts[K] + 1;
  if (k >= K) return;
  const double v = sl_canon((double)*vals.p[k]);              // exact
  double* row = stats + (size_t)k * SL_COLS;
  row[0] = sl_canon(__dadd_rn(row[0], v));
  row[4] = v;
  if (sl_finite(v)) {
    const long long n = counts[k];
    row[1] = __dadd_rn(row[1], v);
    if (n == 0 || v < row[2]) row[2] = v;
    if (n == 0 || v > row[3]) row[3] = v;
    counts[k] = n + 1;
  }
}

__global__ __launch_bounds__(SL_NT) void k_steplog_flush(double* __restrict__ stats, long long* __restrict__ counts, int K,
                                                         double* __restrict__ out) {
  const int k = threadIdx.x;
  if (k > K) return;
  const long long steps = counts[K];
  double* o = out + (size_t)k * SL_COLS;
  if (k < K) {
    double* row = stats + (size_t)k * SL_COLS;
    const long long n = counts[k];
    o[0] = steps ? sl_canon(__ddiv_rn(row[0], (double)steps)) : 0.0;
    o[1] = n ? __ddiv_rn(row[1], (double)n) : sl_qnan();
    o[2] = n ? row[2] : sl_qnan();
    o[3] = n ? row[3] : sl_qnan();
    o[4] = row[4];
    o[5] = (double)n;
    for (int c = 0; c < SL_COLS - 1; ++c) row[c] = 0.0;       // the reserved column keeps its bits
  } else if (k == K) {
    o[0] = (double)steps;
    for (int c = 1; c < SL_COLS; ++c) o[c] = 0.0;
  }
  // every lane has read counts[K] before any lane writes it: one wavefront would do without, the barrier says so
  __syncthreads();
  if (k <= K) counts[k] = 0;
}

}  // namespace dcf

extern "C" {

int dcf_steplog_ext_version(void) { return DCF_STEPLOG_EXT_VERSION; }

static int steplog_tables(const char* who, int32_t K, const void* stats, const void* counts) {
  DCF_CHECK(K >= 1 && K <= DCF_STEPLOG_MAX_KEYS, "%s: K %d (1 <= K <= %d)", who, (int)K, DCF_STEPLOG_MAX_KEYS);
  DCF_CHECK(stats && counts, "%s: null %s", who, !stats ? "stats" : "counts");
  DCF_CHECK(reinterpret_cast<uintptr_t>(stats) % 8 == 0 && reinterpret_cast<uintptr_t>(counts) % 8 == 0,
            "%s: stats / counts not aligned to 8 bytes", who);
  return 0;
}

int dcf_op_steplog_add(const float* const* vals, int32_t K, double* stats, int64_t* counts, void* stream) {
  const char* who = "dcf_op_steplog_add";
  DCF_CHECK(vals, "%s: null vals", who);
  if (steplog_tables(who, K, stats, counts)) return -1;
  dcf::SteplogVals v{};
  for (int k = 0; k < K; ++k) {
    DCF_CHECK(vals[k], "%s: vals[%d] is null", who, k);
    DCF_CHECK(reinterpret_cast<uintptr_t>(vals[k]) % 4 == 0, "%s: vals[%d] not aligned to 4 bytes", who, k);
    v.p[k] = vals[k];
  }
  hipLaunchKernelGGL(dcf::k_steplog_add, dim3(1), dim3(dcf::SL_NT), 0, (hipStream_t)stream, v, (int)K, stats,
                     reinterpret_cast<long long*>(counts));
  DCF_HIP(hipGetLastError());
  return 0;
}

int dcf_op_steplog_flush(double* stats, int64_t* counts, int32_t K, double* out, void* stream) {
  const char* who = "dcf_op_steplog_flush";
  if (steplog_tables(who, K, stats, counts)) return -1;
  DCF_CHECK(out, "%s: null out", who);
  DCF_CHECK(reinterpret_cast<uintptr_t>(out) % 8 == 0, "%s: out not aligned to 8 bytes", who);
  hipLaunchKernelGGL(dcf::k_steplog_flush, dim3(1), dim3(dcf::SL_NT), 0, (hipStream_t)stream, stats, reinterpret_cast<long long*>(counts),
                     (int)K, out);
  DCF_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
