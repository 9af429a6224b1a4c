// Clip features stored as IEEE binary16 (include/decafnet_hip_half.h): the upcast kernel of the forwards that cannot read them
// natively, and the two operators of the extension.  The kernels that DO read half values are instantiations of the ones that read
// fp32: gemm_bf16s_kernel<.., A_CHANMAJOR_H, ..> (gemm_bf16s.hip) and k_sidekick_partial_h<NQ> (score.hip).
#include <algorithm>

#include "engine.h"
#include "../../include/decafnet_hip_half.h"

namespace dcf {

typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));

// dst[i] = (float)src[i], exact (subnormals included).  VEC: four values per thread and step (src 8-byte, dst 16-byte aligned), the
// n % 4 last ones one by one
template <bool VEC>
__global__ __launch_bounds__(256) void k_half_to_f32(const _Float16* __restrict__ src, float* __restrict__ dst, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if constexpr (VEC) {
    const int64_t n4 = n >> 2;
    for (int64_t j = i; j < n4; j += stride)
      *reinterpret_cast<f32x4*>(dst + 4 * j) = __builtin_convertvector(*reinterpret_cast<const h16x4*>(src + 4 * j), f32x4);
    i += n4 << 2;
  }
  for (; i < n; i += stride) dst[i] = (float)src[i];
}

int launch_half_to_f32(const uint16_t* src, float* dst, int64_t n, hipStream_t st) {
  if (n <= 0) return 0;
  DCF_CHECK(src && dst, "half_to_f32: null operand");
  ProfScope prof("half_to_f32", st, 0.0, 6.0 * (double)n);
  const bool vec = (reinterpret_cast<uintptr_t>(src) & 7) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
  const int64_t work = vec ? (n + 3) / 4 : n;
  const unsigned blocks = (unsigned)std::min<int64_t>((work + 255) / 256, 8192);
  if (vec) hipLaunchKernelGGL(k_half_to_f32<true>, dim3(blocks), dim3(256), 0, st, reinterpret_cast<const _Float16*>(src), dst, n);
  else hipLaunchKernelGGL(k_half_to_f32<false>, dim3(blocks), dim3(256), 0, st, reinterpret_cast<const _Float16*>(src), dst, n);
  DCF_HIP(hipGetLastError());
  return 0;
}

}  // namespace dcf

extern "C" {

int dcf_half_ext_version(void) { return DCF_HALF_EXT_VERSION; }

int dcf_op_linear_cm_split_h(const uint16_t* A_cm, const float* W, const float* bias, float* C, int32_t M, int32_t N, int32_t K,
                             int32_t nterms, int32_t unscaled, void* stream) {
  return dcf_op_linear_cm_split_ld_h(A_cm, M, W, bias, C, M, N, K, nterms, unscaled, stream);
}

int dcf_op_linear_cm_split_ld_h(const uint16_t* A_cm, int64_t lda, const float* W, const float* bias, float* C, int32_t M, int32_t N,
                                int32_t K, int32_t nterms, int32_t unscaled, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  DCF_CHECK(A_cm && W && C, "dcf_op_linear_cm_split_h: null operand");
  DCF_CHECK(nterms == dcf::GEMM_F16X3 || nterms == dcf::GEMM_BF16X6, "dcf_op_linear_cm_split_h: nterms must be 16 (f16x3) or 6 (bf16x6)");
  DCF_CHECK(M > 0 && M % 4 == 0 && N > 0 && N % 128 == 0 && K > 0 && K % 32 == 0,
            "dcf_op_linear_cm_split_h: needs M %% 4 == 0 (the row pitch of the half operand), N %% 128 == 0, K %% 32 == 0 (got %d x %d x %d)", M, N, K);
  DCF_CHECK(lda >= M && lda % 4 == 0, "dcf_op_linear_cm_split_h: the row pitch lda = %lld must be >= M = %d and lda %% 4 == 0 (8-byte loads of four rows)",
            (long long)lda, M);
  DCF_CHECK((reinterpret_cast<uintptr_t>(A_cm) & 7) == 0, "dcf_op_linear_cm_split_h: the half operand must be 8-byte aligned");
  dcf::StreamScratch sc(st);
  unsigned short* planes = nullptr;
  if (sc.take(&planes, (size_t)3 * N * K)) return -1;
  int rc = dcf::launch_split_planes(W, planes, N, K, K, st, nterms);
  dcf::GemmArgs g = dcf::gemm(reinterpret_cast<const float*>(A_cm), lda, W, bias, C, N, M, N, K);
  g.Ws = planes;
  if (unscaled) g.a_scale = 1.f;
  if (rc == 0) rc = dcf::launch_gemm_split(&g, 1, dcf::A_CHANMAJOR_H, nterms, st);
  return sc.end(rc);
}

int dcf_op_sidekick_h(const uint16_t* shallow, const float* text_cls, float* correl, int32_t D, int32_t T, int32_t nq,
                      int32_t norm, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  DCF_CHECK(shallow && text_cls && correl && D >= 1 && T >= 1 && nq >= 1, "dcf_op_sidekick_h: bad arguments");
  dcf::StreamScratch sc(st);
  float *tn = nullptr, *partial = nullptr;
  if (sc.take(&tn, (size_t)nq * D) || sc.take(&partial, (size_t)dcf::SCORE_SLICES * (nq + 1) * T)) return -1;
  return sc.end(dcf::launch_sidekick(dcf::score_args(reinterpret_cast<const float*>(shallow), text_cls, tn, partial, correl, D, T, nq, norm), st, true));
}

}  // extern "C"
