"""Restatements of the training extension's three operator pairs (include/decafnet_hip_train.h) in torch, fp64 or fp32, on the keep
bits of tests/philox_ref.py; the fp32 evaluation of the residual in the kernel's stated order; the project's gradient rule.

Token-major (B, T, C) tensors of a (B, C, T) tensor of the reference whose first sequence is sample b0 of its batch:
e = ((b0 + b) * C + c) * T + t, drop-path e = b0 + b."""
import numpy as np
import torch

import philox_ref as P

FLOOR = 2.0 ** -21


def keep_rows(seed, site, B, T, C, b0, p):
    """keep bits (B, T, C) bool of dropout at rate p (all True at p = 0)"""
    if p <= 0:
        return torch.ones(B, T, C, dtype=torch.bool)
    b, c, t = np.meshgrid(np.arange(B, dtype=np.uint64), np.arange(C, dtype=np.uint64), np.arange(T, dtype=np.uint64), indexing='ij')
    e = ((np.uint64(b0) + b) * np.uint64(C) + c) * np.uint64(T) + t              # (B, C, T), the reference's layout
    return torch.from_numpy(np.ascontiguousarray(P.keep(seed, site, e, p).transpose(0, 2, 1)))


def keep_paths(seed, site, B, b0, p):
    """per-sample keep bits (B,) bool of drop-path at rate p"""
    if p <= 0:
        return torch.ones(B, dtype=torch.bool)
    return torch.from_numpy(P.keep(seed, site, np.arange(b0, b0 + B, dtype=np.uint64), p))


def factor(keep, p, dtype):
    """kept ? 1 / (1 - p) : 0 with the fp32 scale of the kernels"""
    return keep.to(dtype) * float(P.scale(p))


# ---------------------------------------------------------------------------------- forwards (differentiable) and hand-written backwards
def dropout(x, k):
    return x * k


def dropout_bwd(gy, k):
    return gy * k


def gelu_dropout(x, k):
    return torch.nn.functional.gelu(x) * k


def gelu_dropout_bwd(x, gy, k):
    Phi = 0.5 * torch.erfc(-x / 2.0 ** 0.5)
    phi = torch.exp(-0.5 * x * x) / (2.0 * torch.pi) ** 0.5
    return (gy * k) * (Phi + x * phi)


def drop_residual(r, m_r, h, m_h, ls, k, dp):
    """Y = R m_R + ls dp(b) k (H m_H); masks (B, T) of the dtype or None, ls (C), k (B, T, C), dp (B,)"""
    r = r if m_r is None else r * m_r[..., None]
    h = h if m_h is None else h * m_h[..., None]
    return r + ls * dp[:, None, None] * (k * h)


def drop_residual_bwd(gy, h, m_r, m_h, ls, k, dp):
    """-> dR, dH, dls"""
    f = k * dp[:, None, None]
    one = torch.ones(gy.shape[:2], dtype=gy.dtype)
    m_r, m_h = one if m_r is None else m_r, one if m_h is None else m_h
    return gy * m_r[..., None], gy * ls * f * m_h[..., None], (gy * f * h * m_h[..., None]).sum((0, 1))


# ---------------------------------------------------------------------------------- the residual's fp32 evaluation, bit for bit
def fma32(a, b, c):
    """fp32 fused multiply-add on numpy float32 arrays: the product is exact in fp64, the sum is rounded to odd there (53 bits hold the
    24 of the result and two more), so the final rounding to fp32 is the single rounding of the fused operation"""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.broadcast_to(c.astype(np.float64), p.shape)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                                # TwoSum: p + c = s + err exactly
    even = (s.view(np.int64) & 1) == 0
    odd = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
    return np.where((err != 0) & even, odd, s).astype(np.float32)


def drop_residual_bits(r, m_r, h, m_h, ls, keep, p_drop, path_keep, p_path):
    """Y as the kernel evaluates it: v = H m_H; v = kept ? v * scale : +0; Y = fma(ls * v, dp, R m_R); a masked factor is a
    multiplication by 0.0f / 1.0f.  numpy float32 in and out; keep (B, T, C) and path_keep (B,) bool"""
    f32 = np.float32
    v = h if m_h is None else h * m_h.astype(f32)[..., None]
    v = np.where(keep, v * P.scale(p_drop), f32(0)) if p_drop > 0 else v * f32(1)
    dp = np.where(path_keep, P.scale(p_path), f32(0)).astype(f32) if p_path > 0 else np.ones(len(path_keep), f32)
    rm = r if m_r is None else r * m_r.astype(f32)[..., None]
    return fma32((ls * v).astype(f32), dp[:, None, None], rm)


# ---------------------------------------------------------------------------------- the gradient rule
def check(label, tag, got, g64, g32, top=None):
    """e_gpu <= max(4 e_ref, 2^-21 max |g_64|), e = max |g - g_64| (tests/test_gpu_step_grad.py); prints one `label` line;
    -> None or the miss"""
    got, g64, g32 = got.detach().cpu().double(), g64.detach().double(), g32.detach().double()
    assert got.shape == g64.shape == g32.shape, (tag, got.shape, g64.shape, g32.shape)
    assert bool(torch.isfinite(got).all()), tag
    top = float(g64.abs().max()) if top is None else top
    e_ref, e_gpu = float((g32 - g64).abs().max()), float((got - g64).abs().max())
    bound = max(4 * e_ref, FLOOR * top)
    ok = e_gpu <= bound
    print(f'{label} {tag}: max|g64| {top:.3e} e_ref {e_ref:.3e} e_gpu {e_gpu:.3e} bound {bound:.3e} ratio {e_gpu / bound if bound else 0.0:.3f}'
          f'{"" if ok else "  MISSED"}')
    return None if ok else (tag, e_gpu, bound)
