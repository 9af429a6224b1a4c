// Selected-clip training (include/decafnet_hip_front_select.h): vid_map of the training step and its weight gradient on the packed
// expert rows of the clips the top-k gates keep -- front_grad.hip with the zero rows of the expert half left out.
//
//   forward   P1c = rows W1^T   ONE row-major product over the packed rows of all videos (launch_gemm_split A_ROWS, f16x3, where
//             E % 128 == 0; the fp32 tile GEMM otherwise), P2[v] = shallow[v]^T W2^T once per video exactly as front_grad.hip forms it;
//             Y[q,t,:] = bias + m ( g P1c[row_first[v] + pos[v,t], :] + P2[v,t,:] + c w3 )   k_vidmap_combine_sel (rowops.hip) with the
//             row -> video table of this call
//   backward  k_fs_rowsums: one pass over dY, as k_fg_rowsums makes it, with R1 going to the COMPACT R1c (n_rows, E) at row
//             row_first[v] + pos[v,t] where pos >= 0 (R1c is zeroed first: a packed row that no clip points at holds zeros, nothing
//             uninitialised reaches the matrix cores whatever pos holds); R2, the db and the dw3 partials unchanged
//             dW1[e,d] = sum_i R1c[i,e] rows[i,d]   k_fs_wgrad
//             dW2 from R2 and shallow: k_fg_wgrad of front_grad.hip (launch_front_wgrad, one pair); dw3, db: k_fg_reduce
//
// k_fs_wgrad is k_wgrad<1> of conv_grad.hip without row flags: BOTH operands are token-major, the reduction index (the packed row) is
// strided in both, a thread reads 8 consecutive rows of one column and writes them to LDS as one 16-byte vector per fp16 plane.
// f16x3 on v_mfma_f32_32x32x16_f16: R scaled by the power of two conv_grad.h derives from the bits of max |R1c| (launch_absmax, a
// device word: no host wait), rows pre-scaled by 2^4; a workgroup owns a 64 (e) x 64 (d) tile of dW1 and one slice of the packed rows;
// the fp32 partials of the slices go to scratch and k_fg_reduce adds them in the fixed blocked order of grad_common.h.  The number
// of slices follows from (n_rows, E, D) alone.  LDS: pitch 40 halfs per (plane, column) = 80 B, so every 16-byte vector is aligned and
// the eight lanes of a ds_read_b128 phase fall on distinct bank groups (the rules of conv_grad.hip's header).
//
// rows stored as IEEE binary16 (k_fs_wgrad<true>): read as stored, no fp32 copy.  The value times 2^4 is the hi plane of the fp32 form
// and its lo plane is exactly zero, so ONE X plane is staged and two products are issued (r_lo . x_hi, r_hi . x_hi), as in
// k_fg_wgrad<true>.  Where the base of rows is 16-byte aligned (D % 32 == 0 keeps every row aligned then) a thread loads the 16 bytes
// of 8 consecutive channels of one row and transposes them into LDS with eight 2-byte stores; otherwise 2-byte loads in the fp32
// form's pattern.  Both leave the same values in LDS: the same bits.
#include <type_traits>

#include "../../include/decafnet_hip_front_select.h"
#include "conv_grad.h"
#include "engine.h"
#include "front_grad.h"
#include "gemm.h"
#include "grad_common.h"
#include "rowops.h"

namespace dcf {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int FS_ROWS = 32;       // packed rows per LDS chunk (two k-steps of 16)
constexpr int FS_PITCH = 40;      // halfs per (plane, column): 32 rows + 8 pad = 80 B
constexpr float FS_SX = 16.f;     // feature pre-scale (conv_grad.hip WG_SX)
constexpr int FS_WANT_WGS = 2048; // workgroups the weight-gradient grid aims at when it chooses the number of row slices
constexpr int FS_STRIP = 64;      // clips per workgroup of k_fs_rowsums (one partial of db / dw3 each)

// rfirst[v] = first packed row of video v, v <= n (constant indices: a dynamically indexed by-value argument would go to scratch)
__global__ __launch_bounds__(64) void k_fs_first(SelFirst f, int n, int* __restrict__ rfirst) {
  const int i = threadIdx.x;
  if (i > n) return;
  int mine = 0;
#pragma unroll
  for (int j = 0; j < 17; ++j) mine = j == i ? f.r[j] : mine;
  rfirst[i] = mine;
}

// k_fg_rowsums (front_grad.hip) with the expert half's row sums written to the packed rows: workgroup (strip s, video b), wave w takes
// the clips t0 + w, t0 + w + 4, ... of the strip, adds the rows of the video's queries in their order and writes
// R1c[rfirst[b] + pos[b,t], :] (where 0 <= pos < the video's row count) and R2[b,t,:]; the sums over ITS clips of dY (db) and m c dY
// (dw3) stay in registers, the four waves are added in a fixed order and go to part[(b nstrips + s)][2][E].
template <int NCH>
__global__ __launch_bounds__(256) void k_fs_rowsums(const float* __restrict__ dY, const float* __restrict__ gate, const uint8_t* __restrict__ mask,
                                                   const float* __restrict__ correl, const int* __restrict__ qoff, const int* __restrict__ rfirst,
                                                   const int* __restrict__ pos, float* __restrict__ R1c, float* __restrict__ R2,
                                                   float* __restrict__ part, int T, int E) {
  extern __shared__ float s_fs[];             // [4 waves][2][E]
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.y, t0 = blockIdx.x * FS_STRIP;
  const int t1 = t0 + FS_STRIP < T ? t0 + FS_STRIP : T;
  const int q0 = qoff[b], q1 = qoff[b + 1];
  const int f0 = rfirst[b], nrow = rfirst[b + 1] - f0;
  Row<NCH> db, dw3;
  db.zero(); dw3.zero();
  for (int t = t0 + wave; t < t1; t += 4) {
    Row<NCH> r1, r2;
    r1.zero(); r2.zero();
    for (int q = q0; q < q1; ++q) {
      const int64_t row = (int64_t)q * T + t;
      Row<NCH> d;
      d.load(dY + row * E, E, lane);
      const float m = mask[row] ? 1.f : 0.f;
      const float mg = m * gate[row];
      const float mc = correl ? m * correl[row] : 0.f;
#pragma unroll
      for (int j = 0; j < NCH; ++j) {
        db.v[j] += d.v[j];
        r2.v[j] += m * d.v[j];
        r1.v[j] += mg * d.v[j];
        dw3.v[j] += mc * d.v[j];
      }
    }
    const int pr = pos[(int64_t)b * T + t];
    if (pr >= 0 && pr < nrow) r1.store(R1c + (int64_t)(f0 + pr) * E, E, lane);
    if (R2) r2.store(R2 + ((int64_t)b * T + t) * E, E, lane);
  }
  db.store(s_fs + (wave * 2 + 0) * E, E, lane);
  dw3.store(s_fs + (wave * 2 + 1) * E, E, lane);
  __syncthreads();
  const int64_t po = ((int64_t)b * gridDim.x + blockIdx.x) * 2 * E;
  for (int i = threadIdx.x; i < 2 * E; i += 256)
    part[po + i] = (s_fs[i] + s_fs[2 * E + i]) + (s_fs[4 * E + i] + s_fs[6 * E + i]);
}

// dW[n][c] = sum_i R[i][n] X[i][c] over the packed rows i < rows, both operands token-major
struct FsWgradArgs {
  const float* R;          // (rows, N) row sums of the upstream gradient
  const void* X;           // (rows, C) expert rows: fp32, or binary16 for the half form of the kernel
  const unsigned* absmax;  // device word: bits of max |R|
  float* part;             // (nslices, N, C) partial sums in the scaled domain
  int rows, N, C, slice_rows;
};

// the X operand of a thread on its way to LDS: 8 rows of one column (fp32 values, or halves one by one), or -- VEC -- the 16 bytes of 8
// consecutive channels of one row
template <bool HALF> struct FsXRegs { float v[8]; };
template <> struct FsXRegs<true> { f16x8 v; };

// accumulator element e of lane (h, r32): n = 4 h + (e & 3) + 8 (e >> 2) (the A operand's row), c = r32 (the B operand's column)
template <bool HALF>
__global__ __launch_bounds__(256) void k_fs_wgrad(FsWgradArgs p) {
  constexpr int XPL = HALF ? 1 : 2;                 // planes of the X tile
  using x_elem = std::conditional_t<HALF, _Float16, float>;
  __shared__ __attribute__((aligned(16))) _Float16 s_r[2 * 64 * FS_PITCH];
  __shared__ __attribute__((aligned(16))) _Float16 s_x[XPL * 64 * FS_PITCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int N = p.N, C = p.C;
  const int tiles_c = (C + 63) / 64;
  const int tn = blockIdx.x / tiles_c, tc = blockIdx.x - tn * tiles_c;
  const int slice = blockIdx.y;
  const int r_begin = slice * p.slice_rows;
  const int r_end = r_begin + p.slice_rows < p.rows ? r_begin + p.slice_rows : p.rows;
  float inv;
  const float s = cg_scale(*p.absmax, inv);
  // R and (scalar form) X: lane -> column, wave -> 8 consecutive rows of the chunk
  const int n_g = tn * 64 + lane, c_g = tc * 64 + lane;
  const bool n_ok = n_g < N, c_ok = c_g < C;
  const float* __restrict__ rp = p.R + n_g;
  const x_elem* __restrict__ Xb = static_cast<const x_elem*>(p.X);
  const x_elem* __restrict__ xp = Xb + (c_ok ? c_g : 0);
  // VEC form of X (uniform per launch): thread -> (row tid & 31 of the chunk, channels 8 (tid >> 5) .. + 7 of the tile)
  const bool vec = HALF && (reinterpret_cast<uintptr_t>(p.X) & 15) == 0;
  const int vr = tid & 31, vg = tid >> 5;
  const bool vc_ok = tc * 64 + vg * 8 < C;          // (C is a multiple of 32: a group of 8 channels is whole or absent)
  const x_elem* __restrict__ vp = Xb + tc * 64 + (vc_ok ? vg * 8 : 0);
  const int h = lane >> 5, r32 = lane & 31;
  const int wn = wave & 1, wc = wave >> 1;
  const bool active = tn * 64 + wn * 32 < N && tc * 64 + wc * 32 < C;      // (N, C are multiples of 32: a 32-block is whole or absent)
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;

  float rv[8];
  FsXRegs<HALF> xv;
  auto load = [&](int r0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int r = r0 + wave * 8 + i;
      rv[i] = (n_ok && r < r_end) ? rp[(int64_t)r * N] : 0.f;
    }
    if constexpr (HALF) {
      if (vec) {
        const int r = r0 + vr;
        const f16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
        xv.v = (vc_ok && r < r_end) ? *reinterpret_cast<const f16x8*>(vp + (int64_t)r * C) : z;
        return;
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int r = r0 + wave * 8 + i;
      xv.v[i] = (c_ok && r < r_end) ? xp[(int64_t)r * C] : (x_elem)0;
    }
  };

  load(r_begin);
  for (int r0 = r_begin; r0 < r_end; r0 += FS_ROWS) {
    {
      f16x8 rh, rl;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float v = rv[i] * s;
        const _Float16 hi = (_Float16)v;
        rh[i] = hi;
        rl[i] = (_Float16)(v - (float)hi);
      }
      *reinterpret_cast<f16x8*>(&s_r[(0 * 64 + lane) * FS_PITCH + wave * 8]) = rh;
      *reinterpret_cast<f16x8*>(&s_r[(1 * 64 + lane) * FS_PITCH + wave * 8]) = rl;
      if constexpr (HALF) {
        const f16x8 xh = xv.v * (_Float16)FS_SX;       // exact; there is no lo plane
        if (vec) {
#pragma unroll
          for (int i = 0; i < 8; ++i) s_x[(vg * 8 + i) * FS_PITCH + vr] = xh[i];
        } else {
          *reinterpret_cast<f16x8*>(&s_x[lane * FS_PITCH + wave * 8]) = xh;
        }
      } else {
        f16x8 xh, xl;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float v = xv.v[i];
          const _Float16 hi = (_Float16)(v * FS_SX);
          xh[i] = hi;
          xl[i] = (_Float16)__builtin_fmaf(v, FS_SX, -(float)hi);
        }
        *reinterpret_cast<f16x8*>(&s_x[(0 * 64 + lane) * FS_PITCH + wave * 8]) = xh;
        *reinterpret_cast<f16x8*>(&s_x[(1 * 64 + lane) * FS_PITCH + wave * 8]) = xl;
      }
    }
    __syncthreads();
    if (r0 + FS_ROWS < r_end) load(r0 + FS_ROWS);      // the next chunk travels while this one is multiplied
    if (active) {
#pragma unroll
      for (int ks = 0; ks < FS_ROWS / 16; ++ks) {
        const int ko = ks * 16 + h * 8;
        const f16x8 a_hi = *reinterpret_cast<const f16x8*>(&s_r[(0 * 64 + wn * 32 + r32) * FS_PITCH + ko]);
        const f16x8 a_lo = *reinterpret_cast<const f16x8*>(&s_r[(1 * 64 + wn * 32 + r32) * FS_PITCH + ko]);
        const f16x8 b_hi = *reinterpret_cast<const f16x8*>(&s_x[(0 * 64 + wc * 32 + r32) * FS_PITCH + ko]);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_lo, b_hi, acc, 0, 0, 0);
        if constexpr (!HALF) {
          const f16x8 b_lo = *reinterpret_cast<const f16x8*>(&s_x[(1 * 64 + wc * 32 + r32) * FS_PITCH + ko]);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, b_lo, acc, 0, 0, 0);
        }
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, b_hi, acc, 0, 0, 0);
      }
    }
    __syncthreads();
  }

  if (active) {
    const int c = tc * 64 + wc * 32 + r32;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int n = tn * 64 + wn * 32 + 4 * h + (e & 3) + 8 * (e >> 2);
      p.part[((int64_t)slice * N + n) * C + c] = acc[e];
    }
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------
struct FsShape {
  int nvid, D, T, E, Cin, rows_q, n_rows;      // rows_q = B', n_rows = row_first[nvid]
  SelFirst first;
};

static bool fs_aligned(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

static int fs_check(const char* what, const void* rows, const int32_t* row_first, const int32_t* pos, const float* gate, const uint8_t* mask,
                    const int32_t* nq, int32_t nvid, int32_t D, int32_t T, int32_t E, bool msf, bool scat, FsShape* s) {
  DCF_CHECK(rows && row_first && pos && gate && mask && nq, "%s: null argument", what);
  DCF_CHECK(nvid >= 1 && nvid <= DCF_MAX_VIDEOS, "%s: nvid = %d (1 .. %d videos per call)", what, nvid, DCF_MAX_VIDEOS);
  DCF_CHECK(T >= 1, "%s: T = %d (>= 1)", what, T);
  DCF_CHECK(D > 0 && D % 32 == 0, "%s: D = %d must be a positive multiple of 32", what, D);
  DCF_CHECK(E > 0 && E % 32 == 0 && E <= 1024, "%s: E = %d must be a positive multiple of 32, at most 1024", what, E);
  int64_t rq = 0;
  for (int v = 0; v < nvid; ++v) {
    DCF_CHECK(nq[v] >= 1, "%s: nq[%d] = %d (every video has at least one query)", what, v, nq[v]);
    rq += nq[v];
    DCF_CHECK(rq * T < (1ll << 31) - 64, "%s: %lld rows (< 2^31)", what, (long long)rq * T);
  }
  DCF_CHECK(row_first[0] == 0, "%s: row_first[0] = %d (the packed rows start at 0)", what, row_first[0]);
  for (int v = 0; v < nvid; ++v)
    DCF_CHECK(row_first[v + 1] > row_first[v] && row_first[v + 1] - row_first[v] <= T,
              "%s: row_first[%d] = %d, row_first[%d] = %d (strictly increasing, at most T = %d rows per video)", what, v, row_first[v], v + 1,
              row_first[v + 1], T);
  DCF_CHECK((int64_t)nvid * D * T < (1ll << 40), "%s: feature tensor too large", what);
  s->nvid = nvid; s->D = D; s->T = T; s->E = E; s->Cin = D + (msf ? D : 0) + (scat ? 1 : 0); s->rows_q = (int)rq;
  s->n_rows = row_first[nvid];
  for (int v = 0; v <= 16; ++v) s->first.r[v] = v <= nvid ? row_first[v] : row_first[nvid];
  return 0;
}

// dcf_op_vidmap_selected (half = false) and dcf_op_vidmap_selected_h (half = true: rows upcast once into scratch; shallow read by the
// split tile path's A_CHANMAJOR_H mode where it applies and upcast otherwise, as dcf_op_vidmap_shared_h decides)
static int fs_forward(const char* what, const void* rows_in, const int32_t* row_first, const int32_t* pos, const void* shallow_in, bool half,
                      const float* W, const float* bias, const float* gate, const uint8_t* mask, const float* correl, const int32_t* nq,
                      float* Y, int32_t nvid, int32_t D, int32_t T, int32_t E, hipStream_t st) {
  FsShape s{};
  DCF_CHECK(W && bias && Y, "%s: null argument", what);
  if (fs_check(what, rows_in, row_first, pos, gate, mask, nq, nvid, D, T, E, shallow_in != nullptr, correl != nullptr, &s)) return -1;
  DCF_CHECK(half || fs_aligned(rows_in, 16), "%s: fp32 rows need a 16-byte aligned base", what);
  bool native = false;                               // the shallow product reads the halves as stored
  if (half && shallow_in) {
    const int want = debug_option("half_native", 1);
    native = want != 0 && E % 128 == 0 && T % 4 == 0 && fs_aligned(shallow_in, 8);
    DCF_CHECK(native || want != 2, "%s: the shallow product cannot read the half features natively (E %% 128 != 0, T %% 4 != 0 or a pointer "
                                   "that is not 8-byte aligned) and the option half_native = 2 forbids the upcast", what);
  }
  unsigned* status = nullptr;
  if (cg_begin(what, st, &status)) return -1;
  const int Cin = s.Cin, n_rows = s.n_rows;
  const size_t pe = (size_t)nvid * T * E, px = (size_t)nvid * D * T, pr = (size_t)n_rows * D;
  StreamScratch sc(st);
  const float* rows = static_cast<const float*>(rows_in);
  const void* shallow = shallow_in;
  if (half) {
    float *up1 = nullptr, *up2 = nullptr;
    if (sc.take(&up1, pr) || (shallow_in && !native && sc.take(&up2, px))) return -1;
    if (launch_half_to_f32(static_cast<const uint16_t*>(rows_in), up1, (int64_t)pr, st)) return -1;
    rows = up1;
    if (shallow_in && !native) {
      if (launch_half_to_f32(static_cast<const uint16_t*>(shallow_in), up2, (int64_t)px, st)) return -1;
      shallow = up2;
    }
  }
  const size_t xbytes = native ? sizeof(uint16_t) : sizeof(float);
  const bool split1 = E % 128 == 0;                                                       // the row GEMM of the expert half
  const bool split2 = shallow && (native || (E % 128 == 0 && T % 4 == 0 && fs_aligned(shallow, 16)));   // the channel-major GEMM
  int *tabs = nullptr, *vtab = nullptr;
  float *P1c = nullptr, *P2 = nullptr, *W1c = nullptr, *W2c = nullptr, *w3c = nullptr;
  unsigned short *pl1 = nullptr, *pl2 = nullptr;
  if (sc.take(&tabs, (size_t)nvid + 1) || sc.take(&vtab, (size_t)s.rows_q)) return -1;
  int* qoff = tabs;
  if (sc.take(&P1c, (size_t)n_rows * E) || (shallow && sc.take(&P2, pe))) return -1;
  if (split1 ? sc.take(&pl1, (size_t)3 * E * D) : sc.take(&W1c, (size_t)E * D)) return -1;
  if (shallow && (split2 ? sc.take(&pl2, (size_t)3 * E * D) : sc.take(&W2c, (size_t)E * D))) return -1;
  if (correl && sc.take(&w3c, (size_t)E)) return -1;
  int rc = launch_front_qtables(nvid, nq, qoff, vtab, st);
  if (rc == 0 && (W1c || W2c || w3c)) rc = launch_front_unpack_w(W, Cin, D, E, W1c, W2c, w3c, st);
  if (rc == 0 && split1) rc = launch_split_planes(W, pl1, E, D, Cin, st, GEMM_F16X3, status);
  if (rc == 0 && split2) rc = launch_split_planes(W + D, pl2, E, D, Cin, st, GEMM_F16X3, status);
  if (rc == 0) {                                      // the expert half: every packed row is needed by construction
    GemmArgs g{};
    g.A = rows; g.lda = D; g.C = P1c; g.ldc = E; g.M = n_rows; g.N = E; g.K = D;
    if (split1) { g.W = W; g.ldw = Cin; g.Ws = pl1; g.status = status; }
    else { g.W = W1c; g.ldw = D; }
    rc = split1 ? launch_gemm_split(&g, 1, A_ROWS, GEMM_F16X3, st) : launch_gemm(&g, 1, A_ROWS, st);
  }
  for (int v0 = 0; shallow && v0 < nvid && rc == 0; v0 += 3) {      // the shallow half, three videos per grid
    GemmArgs g[3];
    const int ng = nvid - v0 < 3 ? nvid - v0 : 3;
    for (int i = 0; i < ng; ++i) {
      g[i] = GemmArgs{};
      g[i].A = reinterpret_cast<const float*>(static_cast<const char*>(shallow) + (size_t)(v0 + i) * D * T * xbytes); g[i].lda = T;
      g[i].C = P2 + (size_t)(v0 + i) * T * E; g[i].ldc = E;
      g[i].M = T; g[i].N = E; g[i].K = D;
      if (split2) { g[i].W = W + D; g[i].ldw = Cin; g[i].Ws = pl2; g[i].status = status; }
      else { g[i].W = W2c; g[i].ldw = D; }
    }
    rc = split2 ? launch_gemm_split(g, ng, native ? A_CHANMAJOR_H : A_CHANMAJOR, GEMM_F16X3, st) : launch_gemm(g, ng, A_CHANMAJOR, st);
  }
  if (rc == 0) rc = launch_vidmap_combine_sel(P1c, pos, s.first, P2, bias, gate, mask, w3c, correl, Y, T, s.rows_q * T, E, 0ull, st, vtab);
  rc = sc.end(rc);
  return rc == 0 ? cg_end(st) : rc;
}

// dcf_op_vidmap_selected_bwd (half = false) and dcf_op_vidmap_selected_bwd_h (half = true: both weight-gradient kernels read the
// stored values, for every shape and alignment; nothing is upcast)
static int fs_backward(const char* what, const void* rows, const int32_t* row_first, const int32_t* pos, const void* shallow, bool half,
                       const float* gate, const uint8_t* mask, const float* correl, const int32_t* nq, const float* dY, float* dW, float* db,
                       int32_t nvid, int32_t D, int32_t T, int32_t E, int32_t accumulate, hipStream_t st) {
  FsShape s{};
  DCF_CHECK(dY && dW, "%s: null argument", what);
  if (fs_check(what, rows, row_first, pos, gate, mask, nq, nvid, D, T, E, shallow != nullptr, correl != nullptr, &s)) return -1;
  unsigned* status = nullptr;
  if (cg_begin(what, st, &status)) return -1;
  const int Cin = s.Cin, n_rows = s.n_rows;
  const size_t pe = (size_t)nvid * T * E;
  const int nstrips = (T + FS_STRIP - 1) / FS_STRIP;
  const int tiles = ((E + 63) / 64) * ((D + 63) / 64);
  const int total = FS_WANT_WGS / tiles < 1 ? 1 : (FS_WANT_WGS / tiles > CG_MAX_SLICES ? CG_MAX_SLICES : FS_WANT_WGS / tiles);
  // expert half: slices of the packed rows, whole 32-row chunks, from (n_rows, E, D) alone
  const int slice_rows = ((n_rows + total - 1) / total + FS_ROWS - 1) / FS_ROWS * FS_ROWS;
  const int nslices = (n_rows + slice_rows - 1) / slice_rows;
  // shallow half: T slices of whole gate tiles, as dcf_op_vidmap_shared_bwd cuts them for one pair
  const int want = total / nvid > 1 ? total / nvid : 1;
  const int slice_t = ((T + want - 1) / want + FG_TILE - 1) / FG_TILE * FG_TILE;
  const int spv = (T + slice_t - 1) / slice_t, nslices2 = nvid * spv;
  const int64_t count = (int64_t)E * D;
  StreamScratch sc(st);
  int *tabs = nullptr, *vtab = nullptr;
  float *R1c = nullptr, *R2 = nullptr, *rpart = nullptr, *part = nullptr, *part2 = nullptr;
  unsigned* words = nullptr;
  if (sc.take(&tabs, (size_t)2 * (nvid + 1)) || sc.take(&vtab, (size_t)s.rows_q)) return -1;
  int *qoff = tabs, *rfirst = tabs + nvid + 1;
  if (sc.take(&R1c, (size_t)n_rows * E) || (shallow && sc.take(&R2, pe))) return -1;
  if (sc.take(&rpart, (size_t)nvid * nstrips * 2 * E) || sc.take(&part, (size_t)nslices * count) ||
      (shallow && sc.take(&part2, (size_t)nslices2 * count)) || sc.take(&words, 2))
    return -1;
  int rc = launch_front_qtables(nvid, nq, qoff, vtab, st);
  if (rc == 0) {
    hipLaunchKernelGGL(k_fs_first, dim3(1), dim3(64), 0, st, s.first, nvid, rfirst);
    if (hipMemsetAsync(R1c, 0, (size_t)n_rows * E * sizeof(float), st) != hipSuccess || hipGetLastError() != hipSuccess) {
      set_error("%s: launch failed", what); rc = -1;
    }
  }
  if (rc == 0) {
    const dim3 grid(nstrips, nvid);
    const size_t lds = (size_t)8 * E * sizeof(float);
    const int nch = (E + 255) / 256;
    if (nch == 1) hipLaunchKernelGGL(k_fs_rowsums<1>, grid, dim3(256), lds, st, dY, gate, mask, correl, qoff, rfirst, pos, R1c, R2, rpart, T, E);
    else if (nch == 2) hipLaunchKernelGGL(k_fs_rowsums<2>, grid, dim3(256), lds, st, dY, gate, mask, correl, qoff, rfirst, pos, R1c, R2, rpart, T, E);
    else if (nch == 3) hipLaunchKernelGGL(k_fs_rowsums<3>, grid, dim3(256), lds, st, dY, gate, mask, correl, qoff, rfirst, pos, R1c, R2, rpart, T, E);
    else hipLaunchKernelGGL(k_fs_rowsums<4>, grid, dim3(256), lds, st, dY, gate, mask, correl, qoff, rfirst, pos, R1c, R2, rpart, T, E);
    if (hipGetLastError() != hipSuccess) { set_error("%s: launch failed", what); rc = -1; }
  }
  if (rc == 0) rc = launch_absmax(R1c, (int64_t)n_rows * E, words, st);
  if (rc == 0 && shallow) rc = launch_absmax(R2, (int64_t)pe, words + 1, st);
  if (rc == 0) {
    FsWgradArgs a{};
    a.R = R1c; a.X = rows; a.absmax = words; a.part = part; a.rows = n_rows; a.N = E; a.C = D; a.slice_rows = slice_rows;
    const dim3 grid(tiles, nslices);
    if (half) hipLaunchKernelGGL(k_fs_wgrad<true>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_fs_wgrad<false>, grid, dim3(256), 0, st, a);
    if (hipGetLastError() != hipSuccess) { set_error("%s: launch failed", what); rc = -1; }
  }
  if (rc == 0 && shallow) {
    FrontWgradArgs a{};
    a.R[0] = R2; a.X[0] = shallow; a.absmax[0] = words + 1; a.skip[0] = nullptr; a.part[0] = part2;
    a.R[1] = R2; a.X[1] = shallow; a.absmax[1] = words + 1; a.skip[1] = nullptr; a.part[1] = part2;
    a.nvid = nvid; a.T = T; a.N = E; a.C = D; a.slice_t = slice_t; a.slices_per_video = spv; a.ntiles = (T + FG_TILE - 1) / FG_TILE;
    rc = launch_front_wgrad(a, 1, st, half);
  }
  if (rc == 0) rc = launch_front_reduce(part, nslices, count, (int)count, D, Cin, words, 1.f / FS_SX, dW, accumulate, status, st);
  if (rc == 0 && shallow)
    rc = launch_front_reduce(part2, nslices2, count, (int)count, D, Cin, words + 1, 1.f / FS_SX, dW + D, accumulate, status, st);
  if (rc == 0 && correl)
    rc = launch_front_reduce(rpart + E, nvid * nstrips, (int64_t)2 * E, E, 1, Cin, nullptr, 1.f, dW + (Cin - 1), accumulate, status, st);
  if (rc == 0 && db) rc = launch_front_reduce(rpart, nvid * nstrips, (int64_t)2 * E, E, E, E, nullptr, 1.f, db, accumulate, status, st);
  rc = sc.end(rc);
  return rc == 0 ? cg_end(st) : rc;
}

}  // namespace dcf

using namespace dcf;

extern "C" {

int dcf_front_select_ext_version(void) { return DCF_FRONT_SELECT_EXT_VERSION; }

int dcf_op_vidmap_selected(const float* rows, const int32_t* row_first, const int32_t* pos, const float* shallow, const float* W,
                           const float* bias, const float* gate, const uint8_t* mask, const float* correl, const int32_t* nq, float* Y,
                           int32_t nvid, int32_t D, int32_t T, int32_t E, void* stream) {
  return fs_forward("dcf_op_vidmap_selected", rows, row_first, pos, shallow, false, W, bias, gate, mask, correl, nq, Y, nvid, D, T, E,
                    (hipStream_t)stream);
}

int dcf_op_vidmap_selected_bwd(const float* rows, const int32_t* row_first, const int32_t* pos, const float* shallow, const float* gate,
                               const uint8_t* mask, const float* correl, const int32_t* nq, const float* dY, float* dW, float* db,
                               int32_t nvid, int32_t D, int32_t T, int32_t E, int32_t accumulate, void* stream) {
  return fs_backward("dcf_op_vidmap_selected_bwd", rows, row_first, pos, shallow, false, gate, mask, correl, nq, dY, dW, db, nvid, D, T, E,
                     accumulate, (hipStream_t)stream);
}

int dcf_op_vidmap_selected_h(const uint16_t* rows, const int32_t* row_first, const int32_t* pos, const uint16_t* shallow, const float* W,
                             const float* bias, const float* gate, const uint8_t* mask, const float* correl, const int32_t* nq, float* Y,
                             int32_t nvid, int32_t D, int32_t T, int32_t E, void* stream) {
  return fs_forward("dcf_op_vidmap_selected_h", rows, row_first, pos, shallow, true, W, bias, gate, mask, correl, nq, Y, nvid, D, T, E,
                    (hipStream_t)stream);
}

int dcf_op_vidmap_selected_bwd_h(const uint16_t* rows, const int32_t* row_first, const int32_t* pos, const uint16_t* shallow,
                                 const float* gate, const uint8_t* mask, const float* correl, const int32_t* nq, const float* dY, float* dW,
                                 float* db, int32_t nvid, int32_t D, int32_t T, int32_t E, int32_t accumulate, void* stream) {
  return fs_backward("dcf_op_vidmap_selected_bwd_h", rows, row_first, pos, shallow, true, gate, mask, correl, nq, dY, dW, db, nvid, D, T, E,
                     accumulate, (hipStream_t)stream);
}

}  // extern "C"
