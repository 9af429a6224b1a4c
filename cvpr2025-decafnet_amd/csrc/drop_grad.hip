// Dropout and drop-path of a block as differentiable operators (contract: include/decafnet_hip_train.h; the random stream:
// dropout.h).  Token-major rows [b][t] x C of a (B, C, T) tensor of the reference whose first sequence is sample b0 of its batch:
//
//   dropout                     Y = k X                                  (its own backward: dX = k dY)
//   GELU + dropout (FFN hidden) Y = k gelu(X),  dX = (k dY) gelu'(X)     one pass instead of two, the bits of the two-operator chain
//   residual                    Y = R m_R + ls dp drop(H m_H)            (launch_drop_residual: the bits of the training forward)
//       dR = dY m_R,  dH = ls (dY f) m_H,  dls[c] = sum_rows (dY f) H m_H,   f = dp(b) k(e)
//
// k(e) = kept ? 1 / (1 - p) : 0 from (seed, site, e = ((b0 + b) C + c) T + t), dp(b) alike from (seed, path site, b0 + b).  Nothing is
// stored for the backward: the keep bits are recomputed.  When T % 4 == 0 the four positions t = 4 q .. 4 q + 3 of one channel are the
// four words of one Philox counter block, so the elementwise kernels give a thread four positions of four channels (block_keep) and
// the column reduction, whose waves walk rows in order, refreshes its 16 keep bits every fourth row.  Otherwise every element
// draws its own block.
//
// The column sum dls follows k_ls_bwd (enc_grad.hip) to the letter -- the same row runs, the same workgroup partials, the same
// k_eg_reduce -- so with both probabilities 0 (f = 1) the three outputs have the bits of dcf_op_layerscale_residual_bwd.  Rows of
// a sample whose path was dropped read neither H nor the random stream.
#include "../../include/decafnet_hip_train.h"
#include "dropout.h"
#include "enc_grad.h"
#include "grad_common.h"

namespace dcf {

constexpr int DG_NT = 256;

enum { DG_DROP = 0, DG_GELU_FWD = 1, DG_GELU_BWD = 2 };

// MODE DG_DROP: Y = k X;  DG_GELU_FWD: Y = k gelu(X);  DG_GELU_BWD: Y = (k G) gelu'(X).  Y may alias X or G (element-wise).
template <int MODE>
__global__ __launch_bounds__(DG_NT) void k_dg_elementwise(const float* X, const float* G, float* Y, int nseq, int C, int T, int b0, uint64_t seed,
                                                          DropSite d) {
  const int C4 = C / 4, TQ = (T + 3) / 4;
  const int64_t id = (int64_t)blockIdx.x * DG_NT + threadIdx.x;
  if (id >= (int64_t)nseq * TQ * C4) return;
  const int c4 = (int)(id % C4);
  const int64_t q = id / C4;
  const int s = (int)(q / TQ), t0 = (int)(q % TQ) * 4;
  const unsigned bits = block_keep(seed, d, (int64_t)b0 + s, C, T, 4 * c4, t0);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (t0 + i >= T) break;
    const int64_t off = ((int64_t)s * T + t0 + i) * C + 4 * c4;
    const f32x4 x = ld4(X + off);
    f32x4 g = zero4(), y;
    if (MODE == DG_GELU_BWD) g = ld4(G + off);
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) {
      const bool keep = (bits >> (4 * i + cc)) & 1u;
      if (MODE == DG_DROP) y[cc] = keep ? x[cc] * d.scale : 0.f;
      if (MODE == DG_GELU_FWD) {
        const float a = gelu_exact(x[cc]);
        y[cc] = keep ? a * d.scale : 0.f;
      }
      if (MODE == DG_GELU_BWD) {
        const float gk = keep ? g[cc] * d.scale : 0.f;             // dropout's backward on dY first, then dcf_op_gelu_bwd's product
        y[cc] = gk * gelu_slope(x[cc]);
      }
    }
    st4(Y + off, y);
  }
}

struct DropResGradArgs {
  const float* dY; const float* H; const uint8_t* mR; const uint8_t* mH; const float* ls;
  float* dR; float* dH;
  float* part;             // (nwg, C) per-workgroup sums of dY f H m_H, or nullptr
  int rows, C, T, b0, rows_per_wave;
  uint64_t seed;
  DropSite drop, path;
};

// the four keep bits of channels c .. c + 3 at position t of sample bg (T % 4 != 0: one counter block per element)
__device__ __forceinline__ unsigned row_keep(uint64_t seed, const DropSite& d, int64_t bg, int C, int T, int c, int t) {
  unsigned bits = 0;
#pragma unroll
  for (int cc = 0; cc < 4; ++cc) bits |= (unsigned)drop_keep(seed, d.site, (uint64_t)((bg * C + c + cc) * (int64_t)T + t), d.p) << cc;
  return bits;
}

__global__ __launch_bounds__(256) void k_drop_res_bwd(DropResGradArgs p) {
  __shared__ __attribute__((aligned(16))) float s_ls[4 * 256];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int C = p.C, T = p.T;
  const int c = 256 * blockIdx.y + 4 * lane;
  const bool act = c < C;
  const int64_t r_begin = ((int64_t)blockIdx.x * 4 + wave) * p.rows_per_wave;
  const int64_t r_end = r_begin + p.rows_per_wave < p.rows ? r_begin + p.rows_per_wave : (int64_t)p.rows;
  const bool want_h = p.H != nullptr && p.part != nullptr;
  const bool quads = (T & 3) == 0, dropping = p.drop.p > 0.f;
  const f32x4 ls = (act && p.dH) ? ld4(p.ls + c) : zero4();
  f32x4 acc = zero4();
  int s = -1;                                            // the sample whose drop-path factor `dp` holds
  float dp = 1.f;
  int64_t quad = -1;                                     // T % 4 == 0: `bits` holds the keep bits of rows 4 quad .. 4 quad + 3
  unsigned bits = 0xffffu;
  for (int64_t r = r_begin; r < r_end; ++r) {
    const int sr = (int)(r / T), t = (int)(r - (int64_t)sr * T);
    const int64_t bg = (int64_t)p.b0 + sr;
    if (sr != s) {
      s = sr;
      dp = 1.f;
      if (p.path.p > 0.f) dp = drop_keep(p.seed, p.path.site, (uint64_t)bg, p.path.p) ? p.path.scale : 0.f;
    }
    const bool mr = !p.mR || p.mR[r], mh = (!p.mH || p.mH[r]) && dp != 0.f;      // a dropped sample: no H, no random stream
    if (!act) continue;
    const f32x4 g = ld4(p.dY + r * C + c);
    if (p.dR) st4(p.dR + r * C + c, mr ? g : zero4());
    if (!mh) {
      if (p.dH) st4(p.dH + r * C + c, zero4());
      continue;
    }
    unsigned kb = 0xfu;
    if (dropping) {
      if (quads) {
        if ((r >> 2) != quad) {
          quad = r >> 2;
          bits = block_keep(p.seed, p.drop, bg, C, T, c, t & ~3);
        }
        kb = (bits >> (4 * (t & 3))) & 0xfu;
      } else {
        kb = row_keep(p.seed, p.drop, bg, C, T, c, t);
      }
    }
    const float f = dp * p.drop.scale;
    f32x4 gf;
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) gf[cc] = ((kb >> cc) & 1u) ? g[cc] * f : 0.f;
    if (p.dH) st4(p.dH + r * C + c, ls * gf);
    if (want_h) {
      const f32x4 h = ld4(p.H + r * C + c);
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) acc[cc] = __builtin_fmaf(gf[cc], h[cc], acc[cc]);
    }
  }
  if (!p.part) return;
  st4(s_ls + wave * 256 + 4 * lane, acc);
  __syncthreads();
  const int i = threadIdx.x, cg = 256 * blockIdx.y + i;
  if (cg < C) p.part[(int64_t)blockIdx.x * C + cg] = (s_ls[i] + s_ls[256 + i]) + (s_ls[512 + i] + s_ls[768 + i]);
}

static int dg_check(const char* what, int B, int T, int C, int c_max, int b0, float p) {
  DCF_CHECK(B > 0 && T > 0, "%s: empty batch (B = %d, T = %d)", what, B, T);
  DCF_CHECK(C > 0 && C % 4 == 0 && C <= c_max, "%s: C = %d must be a multiple of 4 up to %d", what, C, c_max);
  DCF_CHECK((int64_t)B * T < (1ll << 31) - 64, "%s: %lld rows (< 2^31)", what, (long long)B * T);
  DCF_CHECK(b0 >= 0, "%s: b0 = %d must not be negative", what, b0);
  DCF_CHECK(p >= 0.f && p < 1.f, "%s: p = %g outside [0, 1)", what, (double)p);
  return 0;
}

static DropSite dg_site(int32_t site, float p) {
  DropSite d;
  d.site = (uint32_t)site;
  d.p = p;
  d.scale = 1.0f / (1.0f - p);
  return d;
}

template <int MODE>
static int dg_elementwise(const float* X, const float* G, float* Y, int B, int T, int C, int b0, int64_t seed, int32_t site, float p, hipStream_t st) {
  const int64_t n = (int64_t)B * ((T + 3) / 4) * (C / 4);
  DCF_CHECK((n + DG_NT - 1) / DG_NT < (1ll << 31), "dropout: %lld thread blocks (< 2^31)", (long long)((n + DG_NT - 1) / DG_NT));
  hipLaunchKernelGGL(k_dg_elementwise<MODE>, dim3((unsigned)((n + DG_NT - 1) / DG_NT)), dim3(DG_NT), 0, st, X, G, Y, B, C, T, b0, (uint64_t)seed,
                     dg_site(site, p));
  DCF_HIP(hipGetLastError());
  return 0;
}

}  // namespace dcf

using namespace dcf;

constexpr int DG_C_ANY = 1 << 20;

extern "C" {

int dcf_train_ext_version(void) { return DCF_TRAIN_EXT_VERSION; }

int dcf_op_dropout(const float* X, float* Y, int32_t B, int32_t T, int32_t C, int32_t b0, int64_t seed, int32_t site, float p, void* stream) {
  DCF_CHECK(X && Y, "dcf_op_dropout: null argument");
  if (dg_check("dcf_op_dropout", B, T, C, DG_C_ANY, b0, p)) return -1;
  DCF_CHECK(aligned16(X) && aligned16(Y), "dcf_op_dropout: pointers must be 16-byte aligned");
  if (p == 0.f && X == Y) return 0;
  return dg_elementwise<DG_DROP>(X, nullptr, Y, B, T, C, b0, seed, site, p, (hipStream_t)stream);
}

int dcf_op_gelu_dropout(const float* X, float* Y, int32_t B, int32_t T, int32_t C, int32_t b0, int64_t seed, int32_t site, float p, void* stream) {
  DCF_CHECK(X && Y, "dcf_op_gelu_dropout: null argument");
  if (dg_check("dcf_op_gelu_dropout", B, T, C, DG_C_ANY, b0, p)) return -1;
  DCF_CHECK(aligned16(X) && aligned16(Y), "dcf_op_gelu_dropout: pointers must be 16-byte aligned");
  return dg_elementwise<DG_GELU_FWD>(X, nullptr, Y, B, T, C, b0, seed, site, p, (hipStream_t)stream);
}

int dcf_op_gelu_dropout_bwd(const float* X, const float* dY, float* dX, int32_t B, int32_t T, int32_t C, int32_t b0, int64_t seed, int32_t site,
                            float p, void* stream) {
  DCF_CHECK(X && dY && dX, "dcf_op_gelu_dropout_bwd: null argument");
  if (dg_check("dcf_op_gelu_dropout_bwd", B, T, C, DG_C_ANY, b0, p)) return -1;
  DCF_CHECK(aligned16(X) && aligned16(dY) && aligned16(dX), "dcf_op_gelu_dropout_bwd: pointers must be 16-byte aligned");
  return dg_elementwise<DG_GELU_BWD>(X, dY, dX, B, T, C, b0, seed, site, p, (hipStream_t)stream);
}

int dcf_op_drop_residual(const float* R, const uint8_t* mR, const float* H, const uint8_t* mH, const float* ls, float* Y, int32_t B, int32_t T,
                         int32_t C, int32_t b0, int64_t seed, int32_t drop_site, float drop_p, int32_t path_site, float path_p, void* stream) {
  DCF_CHECK(R && H && ls && Y, "dcf_op_drop_residual: null argument");
  if (dg_check("dcf_op_drop_residual", B, T, C, 1024, b0, drop_p) || dg_check("dcf_op_drop_residual", B, T, C, 1024, b0, path_p)) return -1;
  DCF_CHECK(aligned16(R) && aligned16(H) && aligned16(ls) && aligned16(Y), "dcf_op_drop_residual: pointers must be 16-byte aligned");
  DCF_CHECK(!mR || !mH || mR == mH, "dcf_op_drop_residual: mR and mH, where both are given, are one array (a block has one mask)");
  if (drop_p == 0.f && path_p == 0.f) return dcf_op_layerscale_residual(R, mR, H, mH, ls, Y, B * T, C, stream);
  DropResArgs a{};
  a.out = Y; a.ldo = C; a.R = R; a.ldr = C; a.H = H; a.ldh = C;
  a.rowmask = mR ? mR : mH; a.res_mask = mR != nullptr; a.out_mask = mH != nullptr;
  a.ls = ls; a.rows = B * T; a.C = C; a.T = T; a.b0 = b0; a.seed = (uint64_t)seed;
  a.drop = dg_site(drop_site, drop_p);
  a.path = dg_site(path_site, path_p);
  return launch_drop_residual(a, (hipStream_t)stream);
}

int dcf_op_drop_residual_bwd(const float* dY, const float* H, const uint8_t* mR, const uint8_t* mH, const float* ls, float* dR, float* dH, float* dls,
                             int32_t B, int32_t T, int32_t C, int32_t b0, int64_t seed, int32_t drop_site, float drop_p, int32_t path_site,
                             float path_p, int32_t accumulate, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  DCF_CHECK(dY, "dcf_op_drop_residual_bwd: null dY");
  DCF_CHECK(!dH || ls, "dcf_op_drop_residual_bwd: dH needs the scale");
  DCF_CHECK(!dls || H, "dcf_op_drop_residual_bwd: dls needs H");
  if (dg_check("dcf_op_drop_residual_bwd", B, T, C, 1024, b0, drop_p) || dg_check("dcf_op_drop_residual_bwd", B, T, C, 1024, b0, path_p)) return -1;
  DCF_CHECK(aligned16(dY) && aligned16(H) && aligned16(ls) && aligned16(dR) && aligned16(dH),
            "dcf_op_drop_residual_bwd: pointers must be 16-byte aligned");
  if (!dR && !dH && !dls) return 0;
  const int rows = B * T;
  DropResGradArgs a{};
  a.dY = dY; a.H = H; a.mR = mR; a.mH = mH; a.ls = ls; a.dR = dR; a.dH = dH; a.rows = rows; a.C = C; a.T = T; a.b0 = b0;
  a.seed = (uint64_t)seed;
  a.drop = dg_site(drop_site, drop_p);
  a.path = dg_site(path_site, path_p);
  a.rows_per_wave = (rows + 4 * EG_MAX_WG - 1) / (4 * EG_MAX_WG);                    // a fixed function of `rows`, as k_ls_bwd
  const int nwg = (rows + 4 * a.rows_per_wave - 1) / (4 * a.rows_per_wave);
  StreamScratch sc(st);
  float* part = nullptr;
  if (dls && sc.take(&part, (size_t)nwg * C)) return -1;
  a.part = part;
  int rc = 0;
  hipLaunchKernelGGL(k_drop_res_bwd, dim3(nwg, (C + 255) / 256), dim3(256), 0, st, a);
  if (dls) launch_eg_reduce(part, nwg, (int64_t)C, C, dls, 1, 1, accumulate, st);
  if (hipGetLastError() != hipSuccess) { set_error("dcf_op_drop_residual_bwd: launch failed"); rc = -1; }
  return sc.end(rc);
}

}  // extern "C"
