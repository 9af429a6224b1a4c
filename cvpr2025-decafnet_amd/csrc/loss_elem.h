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

}  // namespace dcf
