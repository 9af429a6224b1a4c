// Batch assembly of the training data path (include/decafnet_hip_batch.h): B windows of a device-resident feature bank, stored as
// the files hold them -- row-major (rows, C) --, become one padded channel-major (B, C, T_out) batch and its (B, T_out) mask.  A
// ragged transpose: what the reference's loader does per step on the host with a transpose per video, a zero-filled buffer and a
// copy per sample.
//
// One workgroup moves one square tile of SIDE x SIDE elements through LDS.  Every lane moves one dword per access on both sides:
// one fp32 element, or two binary16 elements (SIDE = 64 resp. 128), so a wave reads 256 contiguous bytes of a bank row (coalesced
// along C) and writes 256 contiguous bytes of an output row (coalesced along t).  The LDS image is the tile already transposed,
// [channel][t] with a pitch of 65 dwords: the store phase reads dword `lane` of a row (conflict free); the load phase writes dwords
// down a column at a stride of 65 (fp32: conflict free) or 130 dwords (binary16: two-way, which a ds_write_b32 has for free).  The
// binary16 form loads two bank rows per step and regroups the four halves of (c, c + 1) x (t, t + 1) in registers, so that it writes
// whole dwords to LDS like the fp32 form (with one half-word LDS store per element it ran at 0.44 of a copy's rate, so at 0.53).
//
// The pair accesses of the binary16 form are guarded per lane, not assumed: a bank row of odd C or an odd first row starts on a
// 2-byte boundary, an output row of odd T_out likewise; such a lane moves its two elements one by one, and so does the lane that
// holds the last element of an odd row.  Tiles that lie wholly in the padding (t0 >= n) read nothing and store zeros.  No scratch.
#include "../../include/decafnet_hip_batch.h"
#include "common.h"

namespace dcf {

constexpr int ASM_NT = 256;                      // four waves: wave w owns the tile rows w, w + 4, ... of either phase
constexpr int ASM_WAVES = ASM_NT / DCF_WAVE;

template <typename E>
struct AsmTile {
  static constexpr int V = 4 / (int)sizeof(E);   // elements per lane and access
  static constexpr int SIDE = DCF_WAVE * V;      // the tile's side in elements
  static constexpr int PITCH = SIDE + V;         // 65 dwords
};

__device__ __forceinline__ bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

template <typename E>
__global__ __launch_bounds__(ASM_NT) void k_assemble_rows(const E* __restrict__ bank, const int64_t* __restrict__ desc, int C, long long T_out,
                                                          E* __restrict__ out, uint8_t* __restrict__ mask) {
  constexpr int V = AsmTile<E>::V, SIDE = AsmTile<E>::SIDE, DW_PITCH = AsmTile<E>::PITCH / V;
  __shared__ uint32_t tile_dw[SIDE * DW_PITCH];
  const int b = blockIdx.z, lane = threadIdx.x & (DCF_WAVE - 1), wave = threadIdx.x / DCF_WAVE;
  const long long t0 = (long long)blockIdx.x * SIDE;
  const int c0 = blockIdx.y * SIDE;
  const long long off = desc[2 * b];
  long long n = desc[2 * b + 1];
  n = n < 0 ? 0 : (n > T_out ? T_out : n);       // no descriptor writes outside out / mask
  if (mask != nullptr && blockIdx.y == 0 && (int)threadIdx.x < SIDE) {
    const long long t = t0 + threadIdx.x;
    if (t < T_out) mask[(long long)b * T_out + t] = t < n ? 1 : 0;
  }
  const bool live = t0 < n;                      // block uniform: a tile in the padding loads nothing
  if (live) {
    const int c = c0 + V * lane;
    // this lane's dword of bank row t: V elements from channel c on, zeros past the window and past C
    auto row_dword = [&](long long t) -> uint32_t {
      if (t >= n || c >= C) return 0u;
      const E* src = bank + (off + t * C + c);
      if (V == 1 || (c + V <= C && aligned4(src))) return *reinterpret_cast<const uint32_t*>(src);
      uint32_t w = src[0];
      if (c + 1 < C) w |= (uint32_t)src[V - 1] << 16;
      return w;
    };
    if constexpr (V == 1) {
#pragma unroll 4
      for (int r = wave; r < SIDE; r += ASM_WAVES) tile_dw[lane * DW_PITCH + r] = row_dword(t0 + r);
    } else {
      // two rows per step: the halves of (c, c + 1) x (t, t + 1) regrouped in registers into the two dwords of the image
#pragma unroll 4
      for (int r = wave; r < SIDE / 2; r += ASM_WAVES) {
        const uint32_t w0 = row_dword(t0 + 2 * r), w1 = row_dword(t0 + 2 * r + 1);
        tile_dw[(2 * lane) * DW_PITCH + r] = (w0 & 0xffffu) | (w1 << 16);
        tile_dw[(2 * lane + 1) * DW_PITCH + r] = (w0 >> 16) | (w1 & 0xffff0000u);
      }
    }
    __syncthreads();
  }
  const long long t = t0 + V * lane;
  if (t >= T_out) return;
  for (int r = wave; r < SIDE; r += ASM_WAVES) {
    const int c = c0 + r;
    if (c >= C) break;
    const uint32_t w = live ? tile_dw[r * DW_PITCH + lane] : 0u;
    E* dst = out + (((long long)b * C + c) * T_out + t);
    if (V == 1 || (t + V <= T_out && aligned4(dst))) {
      *reinterpret_cast<uint32_t*>(dst) = w;
    } else {
      dst[0] = (E)(w & 0xffffu);
      if (t + 1 < T_out) dst[1] = (E)(w >> 16);
    }
  }
}

template <typename E>
static int launch_assemble(const void* bank, const int64_t* desc, int B, int C, long long T_out, void* out, uint8_t* mask, hipStream_t st) {
  constexpr int SIDE = AsmTile<E>::SIDE;
  const long long gx = (T_out + SIDE - 1) / SIDE, gy = (C + SIDE - 1) / SIDE;
  DCF_CHECK(gx <= 0x7fffffffll && gy <= 65535 && B <= 65535, "dcf_op_assemble_rows: B %d, C %d, T_out %lld exceed one grid", B, C, T_out);
  hipLaunchKernelGGL(k_assemble_rows<E>, dim3((unsigned)gx, (unsigned)gy, (unsigned)B), dim3(ASM_NT), 0, st, static_cast<const E*>(bank), desc,
                     C, T_out, static_cast<E*>(out), mask);
  DCF_HIP(hipGetLastError());
  return 0;
}

}  // namespace dcf

extern "C" {

int dcf_batch_ext_version(void) { return DCF_BATCH_EXT_VERSION; }

int32_t dcf_op_assemble_rows(const void* bank, int32_t elem_bytes, const int64_t* desc, int32_t B, int32_t C, int64_t T_out, void* out,
                             uint8_t* mask, void* stream) {
  const char* who = "dcf_op_assemble_rows";
  DCF_CHECK(elem_bytes == 2 || elem_bytes == 4, "%s: elem_bytes %d (2 or 4)", who, (int)elem_bytes);
  DCF_CHECK(B >= 1 && C >= 1 && T_out >= 1, "%s: B %d, C %d, T_out %lld (all >= 1)", who, (int)B, (int)C, (long long)T_out);
  DCF_CHECK(bank && desc && out, "%s: null %s", who, !bank ? "bank" : (!desc ? "desc" : "out"));
  DCF_CHECK(reinterpret_cast<uintptr_t>(bank) % elem_bytes == 0 && reinterpret_cast<uintptr_t>(out) % elem_bytes == 0,
            "%s: bank / out not aligned to elem_bytes %d", who, (int)elem_bytes);
  DCF_CHECK(reinterpret_cast<uintptr_t>(desc) % 8 == 0, "%s: desc not aligned to 8 bytes", who);
  hipStream_t st = (hipStream_t)stream;
  // the algorithmic traffic: out and mask once, the rows at most once (the row counts live on the device: the bound is what is reported)
  dcf::ProfScope prof("assemble_rows", st, 0.0, (2.0 * elem_bytes * C + (mask ? 1.0 : 0.0)) * (double)B * (double)T_out);
  if (elem_bytes == 2) return dcf::launch_assemble<uint16_t>(bank, desc, B, C, T_out, out, mask, st);
  return dcf::launch_assemble<uint32_t>(bank, desc, B, C, T_out, out, mask, st);
}

}  // extern "C"
