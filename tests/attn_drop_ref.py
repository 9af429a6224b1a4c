"""The attention cores with dropout on the map -- the sliding-window core and, at the end of the file, global self attention and cross
attention (``dense_*``) --, forward and hand-written backward, and channel dropout, restated in torch for any dtype on the Philox keep bits of tests/philox_ref.py (what csrc/attn_drop.hip computes; the contract is
include/decafnet_hip_attn_drop.h).

Element index of the map: the flat index of the reference's (bs, H, T, W) tensor (blocks.py:364-368), the sample offset by b0,

    e = (((b0 + b) H + h) T + t) W + j,        slot j of row t is key t - W // 2 + j

of the (bs, H, T, Lk) map of global (Lk = T) and cross attention  e = (((b0 + b) H + h) T + t) Lk + j, j the key, and of channel
dropout on a (B', Cin, T) tensor  e = (b0 + b) Cin + c.  With P the softmax map of tests/attn_grad_ref.py, k the keep
factor (scale = fp32(1 / (1 - p)) or 0) and Pd = k o P:

    O_t = sum_j Pd_tj v_j,   dV_j = sum_t Pd_tj dO_t,   dPd_tj = dO_t . v_j,   dP = k o dPd
    delta_t = sum_j Pd_tj dPd_tj,   dS = P o (dP - delta),   dQ, dK from dS as in attn_grad_ref."""
import numpy as np
import torch

import attn_grad_ref as G
import philox_ref as P

DROP_ATTN, DROP_CHANNEL = 6, 7
DROP_G_INPUT = 7


def window_keep(seed, site, B, heads, T, window, p, b0=0):
    """keep bits (B, heads, T, window) bool of a local map"""
    n = B * heads * T * window
    e = np.arange(n, dtype=np.uint64) + np.uint64(b0 * heads * T * window)
    return torch.from_numpy(P.keep(seed, site, e, p).reshape(B, heads, T, window))


def channel_keep(seed, site, B, C, p, b0=0):
    """keep bits (B, C) bool of channel dropout"""
    e = np.arange(B * C, dtype=np.uint64) + np.uint64(b0 * C)
    return torch.from_numpy(P.keep(seed, site, e, p).reshape(B, C))


def factor(keep, p, dtype):
    """the keep factor: the fp32 scale of the contract, exactly, in ``dtype``"""
    return keep.to(dtype) * float(P.scale(p))


def window_attention_drop(q, k, v, mask, heads, window, keep, p):
    """O (B, T, C); differentiable.  ``keep``: (B, heads, T, window) bool"""
    pm, _, idx, _ = G._probabilities(q, k, mask, heads, window)
    return G._merge(torch.einsum('bhtw,bhtwd->bhtd', pm * factor(keep, p, q.dtype), G._split(v, heads)[:, :, idx]))


def window_attention_drop_grads(q, k, v, mask, dO, heads, window, keep, p):
    """(dQ, dK, dV) by the closed forms above"""
    pm, kw, idx, scale = G._probabilities(q, k, mask, heads, window)
    kf = factor(keep, p, q.dtype)
    pd = pm * kf
    qh, gh = G._split(q, heads), G._split(dO, heads)
    dPd = torch.einsum('bhtd,bhtwd->bhtw', gh, G._split(v, heads)[:, :, idx])
    delta = (pd * dPd).sum(-1, keepdim=True)
    dS = pm * (kf * dPd - delta)
    dQ = scale * scale * torch.einsum('bhtw,bhtwd->bhtd', dS, kw)
    flat = idx.reshape(-1)
    dK = torch.zeros_like(qh).index_add_(2, flat, (dS[..., None] * qh[:, :, :, None, :]).flatten(2, 3)) * (scale * scale)
    dV = torch.zeros_like(qh).index_add_(2, flat, (pd[..., None] * gh[:, :, :, None, :]).flatten(2, 3))
    return G._merge(dQ), G._merge(dK), G._merge(dV)


def valid_slots(mask, window):
    """(B, T, window) bool: the slot's key exists, is valid, and the query row is valid"""
    B, T = mask.shape
    idx, exists = G._band(T, window)
    return exists[None] & mask[:, idx] & mask[:, :, None]


def masked_mha_drop(q_in, k_in, v_in, mask, sd, heads, window, keep, p):
    """MaskedMHA.forward, local branch with attn_drop (blocks.py:348-373, :391-392; no proj_drop), on token-major (B, T, C) inputs"""
    ctx = window_attention_drop(G.conv1(q_in, sd, 'query'), G.conv1(k_in, sd, 'key'), G.conv1(v_in, sd, 'value'), mask, heads, window, keep, p)
    return G.conv1(ctx, sd, 'proj')


def channel_dropout(x, keep, p):
    """x (B, T, C) token-major, keep (B, C): kept values times the fp32 scale rounded once in x's dtype, dropped ones +0"""
    scale = torch.tensor(float(P.scale(p)), dtype=x.dtype)
    return torch.where(keep[:, None, :], x * scale, torch.zeros((), dtype=x.dtype))


# ---------------------------------------------------------------------------------------------- global self attention and cross attention
def dense_keep(seed, site, B, heads, T, Lk, p, b0=0):
    """keep bits (B, heads, T, Lk) bool of a (bs, H, T, Lk) map: e = (((b0 + b) H + h) T + t) Lk + j (Lk = T for global self attention)"""
    e = np.arange(B * heads * T * Lk, dtype=np.uint64) + np.uint64(b0 * heads * T * Lk)
    return torch.from_numpy(P.keep(seed, site, e, p).reshape(B, heads, T, Lk))


def _dense_probabilities(q, k, kmask, heads):
    """P (B, h, T, Lk) over the valid keys (a masked key excluded exactly; a sequence without a valid key: zeros), the scale"""
    B, Lk, C = k.shape
    scale = (C // heads) ** -0.25
    kmask = torch.ones(B, Lk, dtype=torch.bool) if kmask is None else kmask.reshape(B, Lk).bool()
    s = torch.einsum('bhtd,bhjd->bhtj', G._split(q, heads) * scale, G._split(k, heads) * scale)
    s = s.masked_fill(~kmask[:, None, None, :], float('-inf'))
    pm = torch.softmax(s, dim=-1)
    return torch.where(kmask.any(1)[:, None, None, None], pm, torch.zeros((), dtype=q.dtype)), scale


def dense_attention_drop(q, k, v, kmask, heads, keep, p):
    """O (B, T, C) of q (B, T, C) on k / v (B, Lk, C); differentiable.  ``keep``: (B, heads, T, Lk) bool"""
    pm, _ = _dense_probabilities(q, k, kmask, heads)
    return G._merge(torch.einsum('bhtj,bhjd->bhtd', pm * factor(keep, p, q.dtype), G._split(v, heads)))


def dense_attention_drop_grads(q, k, v, kmask, dO, heads, keep, p):
    """(dQ, dK, dV) by the closed forms of the module docstring"""
    pm, scale = _dense_probabilities(q, k, kmask, heads)
    kf = factor(keep, p, q.dtype)
    pd = pm * kf
    qh, kh, vh, gh = (G._split(z, heads) for z in (q, k, v, dO))
    dPd = torch.einsum('bhtd,bhjd->bhtj', gh, vh)
    delta = (pd * dPd).sum(-1, keepdim=True)
    dS = pm * (kf * dPd - delta)
    dQ = scale * scale * torch.einsum('bhtj,bhjd->bhtd', dS, kh)
    dK = scale * scale * torch.einsum('bhtj,bhtd->bhjd', dS, qh)
    dV = torch.einsum('bhtj,bhtd->bhjd', pd, gh)
    return G._merge(dQ), G._merge(dK), G._merge(dV)
