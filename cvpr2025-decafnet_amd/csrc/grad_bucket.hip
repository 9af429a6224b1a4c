// The gradient bucket pack of the data-parallel step (include/decafnet_hip_dist.h): every gradient of one bucket is copied, times
// 1 / world, into its slice of the flat arena that the all-reduce then sums over the ranks (what DistributedDataParallel's reducer
// does with one copy kernel per tensor).  The table, the chunk map and the element helpers are the optimizer's (csrc/optim.h): one
// workgroup owns one chunk of DCF_OPTIM_CHUNK elements of one tensor and finds it through the chunk map, nothing scans the table.
//
// HBM bound: one read and one write, 8 bytes per element (4 for a row without a gradient), through 16-byte accesses where the
// tensor's address allows them and element by element where not; a value does not depend on the path that moved it.
#include "../../include/decafnet_hip_dist.h"
#include "optim.h"

namespace dcf {

template <bool MUL>
__global__ __launch_bounds__(OPT_NT) void k_grad_pack(const dcf_optim_row* __restrict__ rows, const int32_t* __restrict__ chunk_map, float scale) {
  const dcf_optim_row r = rows[__builtin_amdgcn_readfirstlane(chunk_map[blockIdx.x])];
  float* dst = static_cast<float*>(r.p);
  const float* src = static_cast<const float*>(r.g);
  const bool has_g = !(r.flags & DCF_OPTIM_NO_GRAD) && src != nullptr;
  const bool al_d = aligned16(dst), al_s = aligned16(src);
  const long long base = ((long long)blockIdx.x - r.chunk0) * DCF_OPTIM_CHUNK;
#pragma unroll
  for (int s = 0; s < OPT_SWEEPS; ++s) {
    const long long i = base + s * OPT_STRIDE + threadIdx.x * OPT_VEC;
    if (i >= r.n) break;
    f32x4 x = {0.f, 0.f, 0.f, 0.f};
    if (has_g) {
      x = load4(src, i, r.n, al_s);
      if (MUL) {
#pragma unroll
        for (int j = 0; j < OPT_VEC; ++j) x[j] = x[j] * scale;
      }
    }
    store4(dst, i, r.n, al_d, x);
  }
}

}  // namespace dcf

extern "C" {

int dcf_dist_ext_version(void) { return DCF_DIST_EXT_VERSION; }

int dcf_dist_pack_grads(const dcf_optim_row* table, const int32_t* chunk_map, int32_t n_tensors, int64_t n_chunks, float scale, void* stream) {
  const char* who = "dcf_dist_pack_grads";
  DCF_CHECK(n_tensors >= 0 && n_chunks >= 0, "%s: negative count (n_tensors %d, n_chunks %lld)", who, (int)n_tensors, (long long)n_chunks);
  DCF_CHECK(n_chunks <= 0x7fffffffll, "%s: %lld chunks exceed one grid", who, (long long)n_chunks);
  DCF_CHECK(n_chunks == 0 || (table && chunk_map), "%s: null table", who);
  DCF_CHECK(n_chunks == 0 || n_tensors > 0, "%s: %lld chunks but no tensors", who, (long long)n_chunks);
  if (n_chunks == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  dcf::ProfScope prof("dist_pack_grads", st, 0.0, 8.0 * (double)n_chunks * DCF_OPTIM_CHUNK);
  if (scale == 1.0f) hipLaunchKernelGGL(dcf::k_grad_pack<false>, dim3((unsigned)n_chunks), dim3(dcf::OPT_NT), 0, st, table, chunk_map, scale);
  else hipLaunchKernelGGL(dcf::k_grad_pack<true>, dim3((unsigned)n_chunks), dim3(dcf::OPT_NT), 0, st, table, chunk_map, scale);
  DCF_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
