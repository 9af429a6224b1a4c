// The Adam / AdamW / EMA update with the step counts on the device (include/decafnet_hip_clock.h).  The chunk kernel is the update of
// optim.h with the group record completed in the kernel: the workgroup reads its row's count and, from the group's table, the pair of
// bias corrections that belongs to count + 1 -- uniform loads -- and then runs optim_adam_sweeps, the sweeps every other update
// runs.  A second kernel of one thread per row advances the counts afterwards: the chunk kernel writes none, so no workgroup reads a
// count that another one of the same launch has written.  Under a guard (include/decafnet_hip_guard.h) both kernels read the verdict
// and return on a skip.
#include "../../include/decafnet_hip_clock.h"
#include "optim.h"

namespace dcf {

// the bias-correction table of one parameter group: pairs {bc1, sqrt_bc2}, pair t - 1 for the count t.  16 bytes, so that the pointer
// and the length of the row's group come with one load from the kernel arguments
struct ClockTable {
  const float* bc;
  long long len;
};
struct ClockTables {
  ClockTable t[DCF_OPTIM_MAX_GROUPS];
};

// The loads a workgroup has to wait for in turn are kept to the chain of the guarded update plus one: the verdict goes out with the
// chunk map's entry (GATED, as in optim_adam_chunk), the row's count with the row, the group's table entry with its record; only the
// pair of corrections itself is a further step.
template <bool EMA, bool GATED>
__global__ __launch_bounds__(OPT_NT) void k_clock_adam(OptimTable tb, OptimGroups hs, ClockTables bc, const long long* __restrict__ steps,
                                                       const float* __restrict__ coef_dev, const int32_t* __restrict__ gate, float beta) {
  static_assert(DCF_GUARD_APPLY == 0, "the gate is open at 0");
  const int32_t closed = GATED ? *gate : 0;                    // one word, the same for the whole grid
  const int ri = __builtin_amdgcn_readfirstlane(tb.chunk_map[blockIdx.x]);
  const long long count = steps[ri];                           // read for every row, used where the row has a gradient
  const dcf_optim_row r = tb.rows[ri];
  const bool has_g = !(r.flags & DCF_OPTIM_NO_GRAD);
  const bool has_e = EMA && r.ema != nullptr;
  if (GATED && closed != 0) return;
  if (!has_g && !has_e) return;
  optim_adam_sweeps<EMA>(
      r, has_g, has_e,
      [&] {                                                    // the group record, completed here: everything in it is uniform
        const int k = __builtin_amdgcn_readfirstlane(r.group) & (DCF_OPTIM_MAX_GROUPS - 1);
        dcf_optim_group h = hs.g[k];                           // read from the kernel arguments, like the table entry
        const ClockTable tab = bc.t[k];
        const long long t = count + 1;
        h.bc1 = 1.f, h.sqrt_bc2 = 1.f;                         // past the end of the table both corrections have rounded to 1
        if (has_g && t >= 1 && t <= tab.len) {
          const float* pair = tab.bc + 2 * (t - 1);
          h.bc1 = pair[0], h.sqrt_bc2 = pair[1];
        }
        return h;
      },
      coef_dev, beta);
}

// one thread per row, after the chunk kernel on the same stream: the count of every row that has a gradient advances
__global__ __launch_bounds__(OPT_NT) void k_clock_tick(const dcf_optim_row* __restrict__ rows, int n_tensors, long long* __restrict__ steps,
                                                       const int32_t* __restrict__ gate) {
  if (gate && *gate != 0) return;
  const int r = blockIdx.x * OPT_NT + threadIdx.x;
  if (r >= n_tensors) return;
  if (rows[r].flags & DCF_OPTIM_NO_GRAD) return;
  steps[r] = steps[r] + 1;
}

}  // namespace dcf

extern "C" {

int dcf_clock_ext_version(void) { return DCF_CLOCK_EXT_VERSION; }

int dcf_clock_adam_step(const dcf_optim_row* table, const int32_t* chunk_map, int32_t n_tensors, int64_t n_chunks,
                        const dcf_optim_group* groups, int32_t n_groups, const float* const* bc_tables, const int32_t* bc_len,
                        int64_t* steps, const float* coef, const dcf_guard_state* guard_state, int32_t with_ema, float ema_beta,
                        void* stream) {
  const char* who = "dcf_clock_adam_step";
  if (dcf::optim_check_table(who, table, chunk_map, n_tensors, n_chunks)) return -1;
  dcf::OptimGroups hs;
  if (dcf::optim_check_groups(who, groups, n_groups, hs)) return -1;
  if (n_tensors == 0) return 0;
  DCF_CHECK(table, "%s: null table", who);
  DCF_CHECK(steps, "%s: null steps", who);
  DCF_CHECK((reinterpret_cast<uintptr_t>(steps) & 7) == 0, "%s: steps must be 8-byte aligned", who);
  dcf::ClockTables bc = {};
  if (n_chunks > 0) {
    DCF_CHECK(n_groups > 0, "%s: %lld chunks but no groups", who, (long long)n_chunks);
    DCF_CHECK(bc_tables && bc_len, "%s: null bc_tables", who);
  }
  if (bc_tables && bc_len) {
    for (int k = 0; k < n_groups; ++k) {
      DCF_CHECK(bc_len[k] >= 0, "%s: negative bc_len %d of group %d", who, (int)bc_len[k], k);
      DCF_CHECK(bc_len[k] == 0 || bc_tables[k], "%s: null bc_tables entry of group %d with bc_len %d", who, k, (int)bc_len[k]);
      bc.t[k].bc = bc_tables[k], bc.t[k].len = bc_len[k];
    }
  }
  hipStream_t st = (hipStream_t)stream;
  const int32_t* gate = guard_state ? &guard_state->verdict : nullptr;
  hipError_t e = hipSuccess;
  {
    dcf::ProfScope prof("clock_adam_step", st, 0.0, (with_ema ? 36.0 : 28.0) * (double)n_chunks * DCF_OPTIM_CHUNK);
    const dcf::OptimTable tb{table, chunk_map};
    const long long* counts = reinterpret_cast<const long long*>(steps);
    if (n_chunks > 0) {
      const dim3 grid((unsigned)n_chunks), block(dcf::OPT_NT);
      if (with_ema && gate) hipLaunchKernelGGL((dcf::k_clock_adam<true, true>), grid, block, 0, st, tb, hs, bc, counts, coef, gate, ema_beta);
      else if (with_ema) hipLaunchKernelGGL((dcf::k_clock_adam<true, false>), grid, block, 0, st, tb, hs, bc, counts, coef, gate, ema_beta);
      else if (gate) hipLaunchKernelGGL((dcf::k_clock_adam<false, true>), grid, block, 0, st, tb, hs, bc, counts, coef, gate, ema_beta);
      else hipLaunchKernelGGL((dcf::k_clock_adam<false, false>), grid, block, 0, st, tb, hs, bc, counts, coef, gate, ema_beta);
      e = hipGetLastError();
    }
    if (e == hipSuccess) {                                     // never the counts without the update
      hipLaunchKernelGGL(dcf::k_clock_tick, dim3((unsigned)((n_tensors + dcf::OPT_NT - 1) / dcf::OPT_NT)), dim3(dcf::OPT_NT), 0, st, table,
                         (int)n_tensors, reinterpret_cast<long long*>(steps), gate);
      e = hipGetLastError();
    }
  }
  DCF_HIP(e);
  return 0;
}

}  // extern "C"
