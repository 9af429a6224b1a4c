// Point annotation (annotate_points_per_video, libs/worker_v2.py:93-133; Trainer._annotate_points, :575-637) and the objective of
// Trainer._microbatch_forward_backward (:441-476) / Evaluator._calc_loss (:1029-1061) on the packed (B', S) outputs of the
// training forward.  Points are not read from memory: coordinate, stride and regression range follow from the index (PointRule).
// The annotation is bit-equal to the reference: strides are powers of two, so i * stride, stride * radius, x / stride and
// 0.5 * (a + b) are exact and a contracted multiply-add gives the bits of the separate operations; what remains are single fp32
// adds, subtracts, min / max and comparisons in the reference's order.  Sums: fixed partials per workgroup, then one ordered pass
// (no floating-point atomics), the split being a function of (B', S) alone.  The gradient of the objective with respect to the
// packed outputs (`total_loss.backward()`, worker_v2.py:467-468, cut at the forward's outputs) is a second instantiation of the same
// kernel: labels and ground-truth offsets come from the same annotate_point, the derivative from loss_elem.h.
#include "../../include/decafnet_hip.h"
#include "common.h"
#include "loss_elem.h"
#include "objective.h"

namespace dcf {

constexpr int OBJ_NT = 256;
constexpr int OBJ_GROUPS = 2;                            // groups of 4 points per thread
constexpr int OBJ_PER_BLOCK = OBJ_NT * OBJ_GROUPS * 4;   // points per workgroup

bool make_point_rule(PointRule& r, int64_t T, int L, double regression_range, double sigma, int use_offset, int64_t max_seq_len,
                     int center_sampling, double radius) {
  if (L < 1 || L > OBJ_MAX_LEVELS || T < 1 || T >= (1 << 23) || (T & ((1ll << (L - 1)) - 1)) != 0) return false;
  if (!(sigma > 0.0 && sigma <= 1.0) || !(regression_range > 0.0) || max_seq_len < T) return false;
  r.T = (int)T;
  r.L = L;
  int o = 0;
  for (int l = 0; l < L; ++l) { r.off[l] = o; o += (int)(T >> l); }
  for (int l = L; l <= OBJ_MAX_LEVELS; ++l) r.off[l] = o;
  r.S = o;
  // model.py:686-696, in the doubles Python computes with; torch.as_tensor(..., dtype=float32) rounds to nearest (:714-716)
  double rr = regression_range;
  r.lo[0] = 0.f;
  r.hi[0] = (float)rr;
  for (int l = 1; l < L; ++l) {
    const double v_min = rr * sigma;
    double v_max = rr * 2;
    if (l == L - 1 && (double)(max_seq_len + 1) > v_max) v_max = (double)(max_seq_len + 1);
    r.lo[l] = (float)v_min;
    r.hi[l] = (float)v_max;
    rr = v_max;
  }
  for (int l = L; l < OBJ_MAX_LEVELS; ++l) r.lo[l] = r.hi[l] = 0.f;
  r.use_offset = use_offset != 0;
  r.radius_sampling = center_sampling != 0;
  r.radius = (float)radius;
  return true;
}

struct PointGt {
  float left, right;                   // ground-truth offsets in units of the stride
  bool in_window, in_range;
};

struct LevelCtx {
  float stride, inv_stride, half, lo, hi;
  float t_min, t_max;                  // sampling window of this level (radius sampling)
};

__device__ __forceinline__ int level_of(const PointRule& r, int i) {
  int l = 0;
  while (l + 1 < r.L && i >= r.off[l + 1]) ++l;
  return l;
}

__device__ __forceinline__ LevelCtx level_ctx(const PointRule& r, int l, float t0, float t1) {
  LevelCtx c;
  c.stride = (float)(1 << l);
  c.inv_stride = 1.0f / c.stride;
  c.half = r.use_offset ? c.stride - 0.5f : 0.f;    // model.py:710-712 adds in place on a strided view of the tics: level l has had 0.5 * 2^k, k <= l
  c.lo = r.lo[l];
  c.hi = r.hi[l];
  const float ctr = 0.5f * (t0 + t1);
  const float rad = c.stride * r.radius;
  c.t_min = fmaxf(ctr - rad, t0);      // .clamp_(min=target[0])
  c.t_max = fminf(ctr + rad, t1);      // .clamp_(max=target[1])
  return c;
}

// j: index of the point inside its level
__device__ __forceinline__ PointGt annotate_point(const PointRule& r, const LevelCtx& c, int j, float t0, float t1) {
  const float x = (float)j * c.stride + c.half;
  const float pt2start = x - t0;
  const float pt2end = t1 - x;
  PointGt g;
  g.left = pt2start * c.inv_stride;    // / stride, a power of two
  g.right = pt2end * c.inv_stride;
  if (r.radius_sampling) g.in_window = (x - c.t_min > 0.f) && (c.t_max - x > 0.f);
  else g.in_window = (pt2start > 0.f) && (pt2end > 0.f);
  const float d = fmaxf(pt2start, pt2end);
  g.in_range = (d >= c.lo) && (d < c.hi);
  return g;
}

__global__ __launch_bounds__(OBJ_NT) void k_annotate(AnnotateArgs p) {
  const int i = blockIdx.x * OBJ_NT + threadIdx.x;
  const int b = blockIdx.y;
  if (i >= p.rule.S) return;
  const float t0 = p.targets[2 * b], t1 = p.targets[2 * b + 1];
  const int l = level_of(p.rule, i);
  const LevelCtx c = level_ctx(p.rule, l, t0, t1);
  const PointGt g = annotate_point(p.rule, c, i - p.rule.off[l], t0, t1);
  const size_t o = (size_t)b * p.rule.S + i;
  p.labels[o] = (g.in_window && g.in_range) ? 1 : 0;
  reinterpret_cast<float2*>(p.offsets)[o] = make_float2(g.left, g.right);
  if (p.in_window) p.in_window[o] = g.in_window ? 1 : 0;
  if (p.in_range) p.in_range[o] = g.in_range ? 1 : 0;
}

struct Acc {
  float f1, f2, iou;
  int npos;
};

__device__ __forceinline__ void objective_point(const ObjectiveArgs& p, const LevelCtx& c, int j, float t0, float t1, bool valid, float x1,
                                                float x2, float ol, float orr, bool two_heads, Acc& a) {
  if (!valid) return;
  const PointGt g = annotate_point(p.rule, c, j, t0, t1);
  const bool pos = g.in_window && g.in_range;
  const float t = pos ? p.t_pos : p.t_neg;
  if (two_heads) a.f1 += focal_elem(x1, t, p.alpha, 2.f, true);
  a.f2 += focal_elem(x2, t, p.alpha, 2.f, true);
  if (pos) {
    a.iou += iou_elem(ol, orr, g.left, g.right, p.kind, p.eps);
    ++a.npos;
  }
}

// Gradient of the objective at one point: the factors of worker_v2.py:447-465 are folded into s_cls (world_size / loss_norm / n_heads
// times the upstream gradient) and s_reg (world_size / loss_norm times loss_weight and the upstream gradient).  0 outside masks
// (logits) and outside labels & masks (offsets).
struct PointGrad {
  float g1, g2, gl, gr;
};

__device__ __forceinline__ PointGrad grad_point(const ObjectiveArgs& p, float s_cls, float s_reg, const LevelCtx& c, int j, float t0, float t1,
                                                bool valid, float x1, float x2, float ol, float orr, bool two_heads) {
  PointGrad o{0.f, 0.f, 0.f, 0.f};
  if (!valid) return o;
  const PointGt g = annotate_point(p.rule, c, j, t0, t1);
  const bool pos = g.in_window && g.in_range;
  const float t = pos ? p.t_pos : p.t_neg;
  if (two_heads) o.g1 = s_cls * focal_grad_elem(x1, t, p.alpha, 2.f, true);
  o.g2 = s_cls * focal_grad_elem(x2, t, p.alpha, 2.f, true);
  if (pos) {
    iou_grad_elem(ol, orr, g.left, g.right, p.kind, p.eps, o.gl, o.gr);
    o.gl *= s_reg;
    o.gr *= s_reg;
  }
  return o;
}

__device__ __forceinline__ void put4(float* dst, float4 v, bool accumulate) {
  float4* d = reinterpret_cast<float4*>(dst);
  if (accumulate) {
    const float4 o = *d;
    v = make_float4(o.x + v.x, o.y + v.y, o.z + v.z, o.w + v.w);
  }
  *d = v;
}

__device__ __forceinline__ void put1(float* dst, float v, bool accumulate) { *dst = accumulate ? *dst + v : v; }

// grid (bpr, nrows): workgroup (k, b) works on the points [k * OBJ_PER_BLOCK, (k + 1) * OBJ_PER_BLOCK) of row b.  VAL: reduces them to
// one partial of the four sums.  GRAD: writes (or, with accumulate, adds) the gradient of every point of the range -- elementwise,
// no atomics, so deterministic by construction.  Both from one pass over the inputs when both are set.
template <bool VAL, bool GRAD>
__global__ __launch_bounds__(OBJ_NT) void k_objective(ObjectiveArgs p, ObjectiveGradArgs q) {
  __shared__ float s_part[OBJ_NT / 64][4];
  const int b = blockIdx.y;
  const int S = p.rule.S;
  const float t0 = p.targets[2 * b], t1 = p.targets[2 * b + 1];
  const bool two = p.logits1 != nullptr;
  const size_t row = (size_t)b * S;
  const float* l1 = two ? p.logits1 + row : nullptr;
  const float* l2 = p.logits2 + row;
  const float* of = p.offsets + 2 * row;
  const uint8_t* mk = p.masks + row;
  float s_cls = 0.f, s_reg = 0.f;
  float *g1 = nullptr, *g2 = nullptr, *go = nullptr;
  bool acc = false;
  if constexpr (GRAD) {
    const double k = (double)q.world_size / (double)*q.loss_norm;
    const double up = q.grad_total ? (double)*q.grad_total : 1.0;
    const double up_cls = q.grad_parts ? (double)q.grad_parts[0] : 0.0, up_reg = q.grad_parts ? (double)q.grad_parts[1] : 0.0;
    s_cls = (float)(k * (up + up_cls) / (two ? 2.0 : 1.0));
    s_reg = (float)(k * ((double)q.loss_weight * up + up_reg));
    g1 = two ? q.g_logits1 + row : nullptr;
    g2 = q.g_logits2 + row;
    go = q.g_offsets + 2 * row;
    acc = q.accumulate != 0;
  }
  Acc a{0.f, 0.f, 0.f, 0};
#pragma unroll
  for (int k = 0; k < OBJ_GROUPS; ++k) {
    const int i0 = (blockIdx.x * (OBJ_NT * OBJ_GROUPS) + k * OBJ_NT + threadIdx.x) * 4;
    if (i0 >= S) continue;
    const int l = level_of(p.rule, i0);
    if (p.vec && i0 + 3 < p.rule.off[l + 1]) {
      // the whole group lies on one level: one level context, 16-byte loads (rows and level starts are multiples of 4 points)
      const LevelCtx c = level_ctx(p.rule, l, t0, t1);
      const uint32_t m4 = *reinterpret_cast<const uint32_t*>(mk + i0);
      const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
      if (m4 == 0) {
        if constexpr (GRAD) {
          if (!acc) {
            if (two) put4(g1 + i0, z, false);
            put4(g2 + i0, z, false);
            put4(go + 2 * i0, z, false);
            put4(go + 2 * i0 + 4, z, false);
          }
        }
        continue;
      }
      const float4 a1 = two ? *reinterpret_cast<const float4*>(l1 + i0) : z;
      const float4 a2 = *reinterpret_cast<const float4*>(l2 + i0);
      const float4 o01 = *reinterpret_cast<const float4*>(of + 2 * i0);
      const float4 o23 = *reinterpret_cast<const float4*>(of + 2 * i0 + 4);
      const int j = i0 - p.rule.off[l];
      if constexpr (VAL) {
        objective_point(p, c, j + 0, t0, t1, (m4 & 0x000000FFu) != 0, a1.x, a2.x, o01.x, o01.y, two, a);
        objective_point(p, c, j + 1, t0, t1, (m4 & 0x0000FF00u) != 0, a1.y, a2.y, o01.z, o01.w, two, a);
        objective_point(p, c, j + 2, t0, t1, (m4 & 0x00FF0000u) != 0, a1.z, a2.z, o23.x, o23.y, two, a);
        objective_point(p, c, j + 3, t0, t1, (m4 & 0xFF000000u) != 0, a1.w, a2.w, o23.z, o23.w, two, a);
      }
      if constexpr (GRAD) {
        const PointGrad d0 = grad_point(p, s_cls, s_reg, c, j + 0, t0, t1, (m4 & 0x000000FFu) != 0, a1.x, a2.x, o01.x, o01.y, two);
        const PointGrad d1 = grad_point(p, s_cls, s_reg, c, j + 1, t0, t1, (m4 & 0x0000FF00u) != 0, a1.y, a2.y, o01.z, o01.w, two);
        const PointGrad d2 = grad_point(p, s_cls, s_reg, c, j + 2, t0, t1, (m4 & 0x00FF0000u) != 0, a1.z, a2.z, o23.x, o23.y, two);
        const PointGrad d3 = grad_point(p, s_cls, s_reg, c, j + 3, t0, t1, (m4 & 0xFF000000u) != 0, a1.w, a2.w, o23.z, o23.w, two);
        if (two) put4(g1 + i0, make_float4(d0.g1, d1.g1, d2.g1, d3.g1), acc);
        put4(g2 + i0, make_float4(d0.g2, d1.g2, d2.g2, d3.g2), acc);
        put4(go + 2 * i0, make_float4(d0.gl, d0.gr, d1.gl, d1.gr), acc);
        put4(go + 2 * i0 + 4, make_float4(d2.gl, d2.gr, d3.gl, d3.gr), acc);
      }
    } else {
      // the shortest levels, the end of a row, or operands that are not 16-byte aligned: point by point
      for (int i = i0; i < min(i0 + 4, S); ++i) {
        const bool valid = mk[i] != 0;
        if (!GRAD && !valid) continue;
        const int li = level_of(p.rule, i);
        const LevelCtx c = level_ctx(p.rule, li, t0, t1);
        const float x1 = two && valid ? l1[i] : 0.f, x2 = valid ? l2[i] : 0.f;
        const float ol = valid ? of[2 * i] : 0.f, orr = valid ? of[2 * i + 1] : 0.f;
        if constexpr (VAL) objective_point(p, c, i - p.rule.off[li], t0, t1, valid, x1, x2, ol, orr, two, a);
        if constexpr (GRAD) {
          const PointGrad d = grad_point(p, s_cls, s_reg, c, i - p.rule.off[li], t0, t1, valid, x1, x2, ol, orr, two);
          if (two) put1(g1 + i, d.g1, acc);
          put1(g2 + i, d.g2, acc);
          put1(go + 2 * i, d.gl, acc);
          put1(go + 2 * i + 1, d.gr, acc);
        }
      }
    }
  }
  if constexpr (!VAL) return;
  const float f1 = wave_sum(a.f1), f2 = wave_sum(a.f2), io = wave_sum(a.iou);
  const float np = wave_sum((float)a.npos);                       // <= 2048 per workgroup: exact in fp32
  if ((threadIdx.x & 63) == 63) {
    float* s = s_part[threadIdx.x >> 6];
    s[0] = f1; s[1] = f2; s[2] = io; s[3] = np;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    float s = 0.f;
    for (int w = 0; w < OBJ_NT / 64; ++w) s += s_part[w][threadIdx.x];
    p.part[((size_t)b * p.bpr + blockIdx.x) * 4 + threadIdx.x] = s;
  }
}

// One workgroup.  Thread t adds the partials of rows t, t + NT, ... in workgroup order; then the rows are added in row order and
// the scalars of worker_v2.py:447-465 applied: x / loss_norm * world_size per term, (cls1 + cls2) / 2, cls + loss_weight * reg.
__global__ __launch_bounds__(OBJ_NT) void k_objective_final(const float* __restrict__ part, int nrows, int bpr, int two_heads,
                                                            const float* __restrict__ loss_norm, float world_size, float loss_weight,
                                                            float* __restrict__ rows, float* __restrict__ rows_out,
                                                            float* __restrict__ out4) {
  __shared__ float s_tot[4];
  for (int b = threadIdx.x; b < nrows; b += OBJ_NT) {
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < bpr; ++k)
      for (int q = 0; q < 4; ++q) s[q] += part[((size_t)b * bpr + k) * 4 + q];
    for (int q = 0; q < 4; ++q) {
      rows[(size_t)b * 4 + q] = s[q];
      if (rows_out) rows_out[(size_t)b * 4 + q] = s[q];
    }
  }
  __syncthreads();
  if (!out4) return;
  if (threadIdx.x < 4) {
    const int q = threadIdx.x;
    if (q < 3) {
      float s = 0.f;
      for (int b = 0; b < nrows; ++b) s += rows[(size_t)b * 4 + q];
      s_tot[q] = s;
    } else {
      long long n = 0;                                            // the reference's norm is an integer sum
      for (int b = 0; b < nrows; ++b) n += (long long)rows[(size_t)b * 4 + 3];
      s_tot[3] = (float)n;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float ln = *loss_norm;
    const float cls2 = s_tot[1] / ln * world_size;
    const float cls = two_heads ? (s_tot[0] / ln * world_size + cls2) / 2.f : cls2;
    const float reg = s_tot[2] / ln * world_size;
    out4[0] = cls;
    out4[1] = reg;
    out4[2] = cls + loss_weight * reg;
    out4[3] = s_tot[3];
  }
}

int launch_annotate(const AnnotateArgs& a, int nrows, hipStream_t st) {
  if (nrows <= 0) return 0;
  ProfScope prof("annotate_points", st, 0.0, 9.0 * (double)nrows * a.rule.S);
  hipLaunchKernelGGL(k_annotate, dim3((a.rule.S + OBJ_NT - 1) / OBJ_NT, nrows), dim3(OBJ_NT), 0, st, a);
  DCF_HIP(hipGetLastError());
  return 0;
}

int objective_blocks_per_row(int S) { return (S + OBJ_PER_BLOCK - 1) / OBJ_PER_BLOCK; }

size_t objective_scratch_bytes(int nrows, int S) {
  return ((size_t)nrows * objective_blocks_per_row(S) + (size_t)nrows) * 4 * sizeof(float);
}

int launch_objective(const ObjectiveArgs& a, int nrows, const float* loss_norm, float world_size, float loss_weight, float* rows_scratch,
                     float* rows_out, float* out4, hipStream_t st) {
  ProfScope prof("point_objective", st, 0.0, (a.logits1 ? 17.0 : 13.0) * (double)nrows * a.rule.S);
  if (nrows > 0) {
    hipLaunchKernelGGL((k_objective<true, false>), dim3(a.bpr, nrows), dim3(OBJ_NT), 0, st, a, ObjectiveGradArgs{});
    DCF_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(k_objective_final, dim3(1), dim3(OBJ_NT), 0, st, (const float*)a.part, nrows, a.bpr, a.logits1 ? 1 : 0, loss_norm,
                     world_size, loss_weight, rows_scratch, rows_out, out4);
  DCF_HIP(hipGetLastError());
  return 0;
}

// The gradient alone (rows_out and out4 NULL: one launch, a.part unused) or values and gradient from one pass over the inputs
int launch_objective_grad(const ObjectiveArgs& a, const ObjectiveGradArgs& g, int nrows, float* rows_scratch, float* rows_out, float* out4,
                          hipStream_t st) {
  const bool val = rows_out || out4;
  ProfScope prof(val ? "point_objective_value_grad" : "point_objective_grad", st, 0.0, (a.logits1 ? 33.0 : 25.0) * (double)nrows * a.rule.S);
  if (nrows > 0) {
    if (val) hipLaunchKernelGGL((k_objective<true, true>), dim3(a.bpr, nrows), dim3(OBJ_NT), 0, st, a, g);
    else hipLaunchKernelGGL((k_objective<false, true>), dim3(a.bpr, nrows), dim3(OBJ_NT), 0, st, a, g);
    DCF_HIP(hipGetLastError());
  }
  if (val) {
    hipLaunchKernelGGL(k_objective_final, dim3(1), dim3(OBJ_NT), 0, st, (const float*)a.part, nrows, a.bpr, a.logits1 ? 1 : 0, g.loss_norm,
                       g.world_size, g.loss_weight, rows_scratch, rows_out, out4);
    DCF_HIP(hipGetLastError());
  }
  return 0;
}

}  // namespace dcf

extern "C" {

int dcf_annotate_points(const float* targets, int32_t nrows, int64_t T, int32_t L, double regression_range, double sigma, int32_t use_offset,
                        int64_t max_seq_len, int32_t center_sampling, double radius, uint8_t* labels_out, float* offsets_out,
                        uint8_t* in_window_out, uint8_t* in_range_out, void* stream) {
  dcf::AnnotateArgs a{};
  DCF_CHECK(nrows >= 0 && (nrows == 0 || (targets && labels_out && offsets_out)), "dcf_annotate_points: bad arguments");
  DCF_CHECK(dcf::make_point_rule(a.rule, T, L, regression_range, sigma, use_offset, max_seq_len, center_sampling, radius),
            "dcf_annotate_points: (T = %lld, L = %d, regression_range = %g, sigma = %g, max_seq_len = %lld) is not a PtGenerator layout "
            "(1 <= L <= 16, T a multiple of 2^(L-1), T <= max_seq_len, T < 2^23, 0 < sigma <= 1)", (long long)T, L, regression_range, sigma,
            (long long)max_seq_len);
  DCF_CHECK(((uintptr_t)offsets_out & 7) == 0, "dcf_annotate_points: offsets_out must be 8-byte aligned");
  a.targets = targets;
  a.labels = labels_out;
  a.offsets = offsets_out;
  a.in_window = in_window_out;
  a.in_range = in_range_out;
  return dcf::launch_annotate(a, nrows, (hipStream_t)stream);
}

int dcf_point_objective(const float* logits1, const float* logits2, const float* offsets, const uint8_t* masks, const float* targets,
                        int32_t nrows, int64_t T, int32_t L, double regression_range, double sigma, int32_t use_offset, int64_t max_seq_len,
                        int32_t center_sampling, double radius, float alpha, double smoothing, int32_t iou_kind, float eps,
                        const float* loss_norm_dev, float world_size, float loss_weight, float* rows_out, float* out4, void* stream) {
  dcf::ObjectiveArgs a{};
  DCF_CHECK(nrows >= 0 && (nrows == 0 || (logits2 && offsets && masks && targets)) && (iou_kind == 0 || iou_kind == 1) &&
                (rows_out || out4) && (!out4 || loss_norm_dev),
            "dcf_point_objective: bad arguments");
  DCF_CHECK(dcf::make_point_rule(a.rule, T, L, regression_range, sigma, use_offset, max_seq_len, center_sampling, radius),
            "dcf_point_objective: (T = %lld, L = %d, regression_range = %g, sigma = %g, max_seq_len = %lld) is not a PtGenerator layout "
            "(1 <= L <= 16, T a multiple of 2^(L-1), T <= max_seq_len, T < 2^23, 0 < sigma <= 1)", (long long)T, L, regression_range, sigma,
            (long long)max_seq_len);
  hipStream_t st = (hipStream_t)stream;
  a.logits1 = logits1;
  a.logits2 = logits2;
  a.offsets = offsets;
  a.masks = masks;
  a.targets = targets;
  a.vec = a.rule.S % 4 == 0 && (((uintptr_t)logits1 | (uintptr_t)logits2 | (uintptr_t)offsets) & 15) == 0 && ((uintptr_t)masks & 3) == 0;
  a.alpha = alpha;
  // calc_focal_loss (worker_v2.py:85-87): labels.to(fp32) * (1.0 - smoothing) + smoothing / 2, the two Python doubles rounded to
  // fp32 where they meet the tensor; the label is 0 or 1, so the product is exact and one fp32 add remains
  a.t_neg = (float)(smoothing / 2);
  a.t_pos = (float)(1.0 - smoothing) + a.t_neg;
  a.eps = eps;
  a.kind = iou_kind;
  a.bpr = dcf::objective_blocks_per_row(a.rule.S);
  dcf::StreamScratch sc(st);
  char* scratch = nullptr;
  if (sc.take(&scratch, dcf::objective_scratch_bytes(nrows > 0 ? nrows : 1, a.rule.S))) return -1;   // sized from (B', S) alone
  a.part = reinterpret_cast<float*>(scratch);
  float* rows = a.part + (size_t)(nrows > 0 ? nrows : 1) * a.bpr * 4;
  return sc.end(dcf::launch_objective(a, nrows, loss_norm_dev, world_size, loss_weight, rows, rows_out, out4, st));
}

int dcf_point_objective_grad(const float* logits1, const float* logits2, const float* offsets, const uint8_t* masks, const float* targets,
                             int32_t nrows, int64_t T, int32_t L, double regression_range, double sigma, int32_t use_offset, int64_t max_seq_len,
                             int32_t center_sampling, double radius, float alpha, double smoothing, int32_t iou_kind, float eps,
                             const float* loss_norm_dev, float world_size, float loss_weight, const float* grad_total_dev,
                             const float* grad_parts_dev, float* g_logits1, float* g_logits2, float* g_offsets, int32_t accumulate,
                             float* rows_out, float* out4, void* stream) {
  dcf::ObjectiveArgs a{};
  DCF_CHECK(nrows >= 0 && (nrows == 0 || (logits2 && offsets && masks && targets && g_logits2 && g_offsets)) && (iou_kind == 0 || iou_kind == 1) &&
                loss_norm_dev && (nrows == 0 || (logits1 == nullptr) == (g_logits1 == nullptr)),
            "dcf_point_objective_grad: bad arguments (g_logits1 goes with logits1; loss_norm_dev is required)");
  DCF_CHECK(dcf::make_point_rule(a.rule, T, L, regression_range, sigma, use_offset, max_seq_len, center_sampling, radius),
            "dcf_point_objective_grad: (T = %lld, L = %d, regression_range = %g, sigma = %g, max_seq_len = %lld) is not a PtGenerator layout "
            "(1 <= L <= 16, T a multiple of 2^(L-1), T <= max_seq_len, T < 2^23, 0 < sigma <= 1)", (long long)T, L, regression_range, sigma,
            (long long)max_seq_len);
  hipStream_t st = (hipStream_t)stream;
  a.logits1 = logits1;
  a.logits2 = logits2;
  a.offsets = offsets;
  a.masks = masks;
  a.targets = targets;
  a.vec = a.rule.S % 4 == 0 && ((uintptr_t)masks & 3) == 0 &&
          (((uintptr_t)logits1 | (uintptr_t)logits2 | (uintptr_t)offsets | (uintptr_t)g_logits1 | (uintptr_t)g_logits2 | (uintptr_t)g_offsets) & 15) == 0;
  a.alpha = alpha;
  a.t_neg = (float)(smoothing / 2);                                // as dcf_point_objective
  a.t_pos = (float)(1.0 - smoothing) + a.t_neg;
  a.eps = eps;
  a.kind = iou_kind;
  a.bpr = dcf::objective_blocks_per_row(a.rule.S);
  dcf::ObjectiveGradArgs g{g_logits1, g_logits2, g_offsets, loss_norm_dev, grad_total_dev, grad_parts_dev, world_size, loss_weight, accumulate != 0};
  if (!rows_out && !out4) return dcf::launch_objective_grad(a, g, nrows, nullptr, nullptr, nullptr, st);
  dcf::StreamScratch sc(st);
  char* scratch = nullptr;
  if (sc.take(&scratch, dcf::objective_scratch_bytes(nrows > 0 ? nrows : 1, a.rule.S))) return -1;
  a.part = reinterpret_cast<float*>(scratch);
  float* rows = a.part + (size_t)(nrows > 0 ? nrows : 1) * a.bpr * 4;
  return sc.end(dcf::launch_objective_grad(a, g, nrows, rows, rows_out, out4, st));
}

}  // extern "C"
