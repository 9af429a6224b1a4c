// Per-element arithmetic of the point losses (libs/modeling/loss.py), shared by loss.hip (the reference's loss functions) and
// objective.hip (the Trainer's fused objective): one definition, so the two paths cannot drift apart.
#pragma once
#include "common.h"

namespace dcf {

// sigmoid_focal_loss, loss.py:5-57
__device__ __forceinline__ float focal_elem(float x, float t, float alpha, float gamma, bool smoothing) {
  const float mask = t >= 0.5f ? 1.f : 0.f;                       // positive mask (loss.py:38)
  const float p = 1.f / (1.f + expf(-x));                         // torch.sigmoid
  const float p_t = smoothing ? p * t + (1.f - p) * (1.f - t) : p * mask + (1.f - p) * (1.f - mask);
  // F.binary_cross_entropy_with_logits(x, t) = (1 - t) x + log(1 + exp(-x)), the log term formed without overflow
  const float ce = (1.f - t) * x + (fmaxf(-x, 0.f) + log1pf(expf(-fabsf(x))));
  const float m = 1.f - p_t;
  float loss = ce * (gamma == 2.f ? m * m : powf(m, gamma));
  if (alpha >= 0.f) loss = (alpha * mask + (1.f - alpha) * (1.f - mask)) * loss;
  return loss;
}

// ctr_giou_loss (kind 0, loss.py:60-109) / ctr_diou_loss (kind 1, loss.py:111-166) of one (left, right) offset pair
__device__ __forceinline__ float iou_elem(float lp, float rp, float lg, float rg, int kind, float eps) {
  const float lkis = fminf(lp, lg), rkis = fminf(rp, rg);
  const float intsctk = rkis + lkis;
  const float unionk = (lp + rp) + (lg + rg) - intsctk;
  const float iouk = intsctk / fmaxf(unionk, eps);
  float loss = 1.0f - iouk;
  if (kind == 1) {
    const float len_c = fmaxf(lp, lg) + fmaxf(rp, rg);             // smallest enclosing segment
    const float rho = 0.5f * (rp - lp - rg + lg);                  // offset between the centres
    const float q = rho / fmaxf(len_c, eps);
    loss = loss + q * q;
  }
  return loss;
}

// Gradients.  Convention at the non-smooth points: eager PyTorch autograd (derivatives.yaml), see include/decafnet_hip.h --
// minimum / maximum give each argument half the gradient at a == b, clamp(min=eps) passes the gradient where x >= eps and blocks
// it below, `targets >= 0.5` carries none.

// d focal_elem / d x.  With ce = BCE-with-logits and m = 1 - p_t:  d ce / d x = p - t,  d p_t / d x = p (1 - p) (2 s - 1) with s the
// (smoothed) target p_t was mixed with,  d loss / d x = alpha_t ((p - t) m^gamma - gamma ce m^(gamma - 1) d p_t / d x).
// p and 1 - p come from one exp(-|x|) each without cancellation, so |x| = 100 gives finite values.
__device__ __forceinline__ float focal_grad_elem(float x, float t, float alpha, float gamma, bool smoothing) {
  const float mask = t >= 0.5f ? 1.f : 0.f;
  const float e = expf(-fabsf(x));
  const float r = 1.f / (1.f + e);
  const float p = x >= 0.f ? r : e * r;                            // sigmoid(x)
  const float q = x >= 0.f ? e * r : r;                            // 1 - sigmoid(x)
  const float s = smoothing ? t : mask;
  const float m = p * (1.f - s) + q * s;                           // 1 - p_t
  const float ce = (1.f - t) * x + (fmaxf(-x, 0.f) + log1pf(e));
  const float dpt = p * q * (2.f * s - 1.f);
  float mg, mg1;                                                   // m^gamma, gamma m^(gamma - 1)
  if (gamma == 2.f) { mg = m * m; mg1 = 2.f * m; }
  else if (gamma == 0.f) { mg = 1.f; mg1 = 0.f; }
  else { mg = powf(m, gamma); mg1 = gamma * powf(m, gamma - 1.f); }
  float g = (p - t) * mg - ce * mg1 * dpt;
  if (alpha >= 0.f) g = (alpha * mask + (1.f - alpha) * (1.f - mask)) * g;
  return g;
}

// d iou_elem / d (lp, rp) -> (gl, gr)
__device__ __forceinline__ void iou_grad_elem(float lp, float rp, float lg, float rg, int kind, float eps, float& gl, float& gr) {
  const float al = lp < lg ? 1.f : (lp == lg ? 0.5f : 0.f);        // d min(lp, lg) / d lp;  d max(lp, lg) / d lp = 1 - al
  const float ar = rp < rg ? 1.f : (rp == rg ? 0.5f : 0.f);
  const float intsctk = fminf(rp, rg) + fminf(lp, lg);
  const float unionk = (lp + rp) + (lg + rg) - intsctk;
  const float inv_u = 1.f / fmaxf(unionk, eps);
  // -(d iou / d lp) = ((1 - al) I - al U) / U^2 where the clamp passes (one subtraction, exact 0 for pred == gt), -al / eps below
  if (unionk >= eps) {
    const float iu2 = inv_u * inv_u;
    gl = ((1.f - al) * intsctk - al * unionk) * iu2;
    gr = ((1.f - ar) * intsctk - ar * unionk) * iu2;
  } else {
    gl = -al * inv_u;
    gr = -ar * inv_u;
  }
  if (kind == 1) {
    const float len_c = fmaxf(lp, lg) + fmaxf(rp, rg);
    const float rho = 0.5f * (rp - lp - rg + lg);
    const float inv_c = 1.f / fmaxf(len_c, eps);
    const float q2 = 2.f * rho * inv_c;                            // 2 q, q = rho / len_c
    const float v = len_c >= eps ? rho * inv_c * inv_c : 0.f;      // q / len_c where the clamp passes
    gl += q2 * (-0.5f * inv_c - v * (1.f - al));
    gr += q2 * (0.5f * inv_c - v * (1.f - ar));
  }
}

}  // namespace dcf
