"""Torch restatement of the closed forms csrc/enc_grad.hip implements (a helper module of tests/test_enc_grad_cpu.py and
tests/test_gpu_enc_grad.py), in the dtype of the operands, and the oracle's functions behind token-major adapters.

Tensors are token-major (B, T, C); masks are (B, T) bool or None (= all valid).

    depthwise convolution   Y_i[b,o,c] = sum_j W_i[c,j] m[b,s o+j-1] X[b,s o+j-1,c]
                            dX[b,t,c]  = m[b,t] sum_i sum_j dY_i[b,o,c] W_i[c,j]   over s o + j - 1 = t
                            dW_i[c,j]  = sum_{b,o} dY_i[b,o,c] m X[b,s o+j-1,c]
    max pooling (3, 2, 1)   f = m ? X : min_t X (detached);  Y[b,o,c] = mo[b,o] max_{t in window o} f[b,t,c]
                            dX[b,t,c] = m[b,t] sum of dY[b,o,c] mo[b,o] over the windows whose maximum sits at t (lowest position wins)
    GELU                    y = x Phi(x),  dx = dy (Phi(x) + x phi(x))
    LayerScale residual     Y = R m_R + ls (H m_H);  dR = dY m_R,  dH = ls dY m_H,  dls[c] = sum_rows dY H m_H
"""
import contextlib
import math
import sys

import torch
import torch.nn.functional as F

from conftest import ROOT

if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import decafnet_ref as O  # noqa: E402


def _m(mask, x):
    B, T, _ = x.shape
    return torch.ones(B, T, dtype=torch.bool) if mask is None else mask


# ------------------------------------------------------------------------------------------
# closed forms
# ------------------------------------------------------------------------------------------
def _taps(x, mask, stride):
    """[x masked and shifted to tap j, sampled at the stride] for j = 0, 1, 2: each (B, To, C); rows outside the sequence are zero"""
    B, T, C = x.shape
    xm = x * _m(mask, x)[..., None].to(x.dtype)
    xp = F.pad(xm, (0, 0, 1, 1))                              # xp[:, u + 1] = xm[:, u]
    return [xp[:, j:j + T:stride] for j in range(3)]


def dwconv3(x, mask, w, stride):
    """w (n, C, 3) -> Y (n, B, T / stride, C)"""
    taps = _taps(x, mask, stride)
    return torch.stack([sum(taps[j] * w[i, :, j] for j in range(3)) for i in range(w.size(0))])


def dwconv3_grads(x, mask, w, dy, stride):
    """dy (n, B, To, C) -> (dX (B, T, C), dW (n, C, 3))"""
    B, T, C = x.shape
    taps = _taps(x, mask, stride)
    dw = torch.stack([torch.stack([(dy[i] * taps[j]).sum((0, 1)) for j in range(3)], dim=-1) for i in range(w.size(0))])
    dxp = torch.zeros(B, T + 2, C, dtype=x.dtype)
    for i in range(w.size(0)):
        for j in range(3):
            dxp[:, j:j + T:stride] += dy[i] * w[i, :, j]
    return dxp[:, 1:T + 1] * _m(mask, x)[..., None].to(x.dtype), dw


def _pool_select(x, mask):
    """(filled values of the three slots (B, To, 3, C) with -inf outside the sequence, index of the lowest position holding the
    maximum (B, To, C), pooled mask (B, To))"""
    B, T, C = x.shape
    m = _m(mask, x)
    f = torch.where(m[..., None], x, x.amin(dim=1, keepdim=True).detach().expand_as(x))
    fp = F.pad(f, (0, 0, 1, 1), value=float('-inf'))
    mp = F.pad(m, (1, 1))
    slots = torch.stack([fp[:, j:j + T:2] for j in range(3)], dim=2)
    mo = torch.stack([mp[:, j:j + T:2] for j in range(3)], dim=2).any(dim=2)
    best = slots.amax(dim=2, keepdim=True)
    first = (slots == best).to(torch.int8).argmax(dim=2)     # argmax of a 0 / 1 tensor: the first 1
    return slots, first, mo


def masked_max_pool(x, mask):
    slots, _, mo = _pool_select(x, mask)
    return slots.amax(dim=2) * mo[..., None].to(x.dtype), mo


def masked_max_pool_grad(x, mask, dy):
    B, T, C = x.shape
    _, first, mo = _pool_select(x, mask)
    g = dy * mo[..., None].to(dy.dtype)
    dxp = torch.zeros(B, T + 2, C, dtype=dy.dtype)
    for j in range(3):
        dxp[:, j:j + T:2] += torch.where(first == j, g, torch.zeros_like(g))
    return dxp[:, 1:T + 1] * _m(mask, x)[..., None].to(dy.dtype)


def gelu(x):
    return x * 0.5 * torch.erfc(-x / math.sqrt(2.0))


def gelu_grad(x, dy):
    return dy * (0.5 * torch.erfc(-x / math.sqrt(2.0)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi))


def layerscale_residual(r, h, ls, r_mask=None, h_mask=None):
    return r * _m(r_mask, r)[..., None].to(r.dtype) + ls * (h * _m(h_mask, h)[..., None].to(h.dtype))


def layerscale_residual_grads(dy, h, ls, r_mask=None, h_mask=None):
    """(dR, dH, dls)"""
    mr, mh = _m(r_mask, dy)[..., None].to(dy.dtype), _m(h_mask, dy)[..., None].to(dy.dtype)
    return dy * mr, ls * dy * mh, (dy * h * mh).sum((0, 1))


# ------------------------------------------------------------------------------------------
# the oracle's functions on token-major tensors (they work on (B, C, T) and (B, 1, T))
# ------------------------------------------------------------------------------------------
@contextlib.contextmanager
def detached_fill():
    """The reference detaches the fill value of padded slots (`x.amin(dim=-1, keepdim=True).detach()`, blocks.py:38); the oracle's
    masked_max_pool1d takes the same minimum without the detach, so under autograd a padded slot that wins a window would hand its
    gradient to the row that holds the minimum.  Inside this context Tensor.amin returns detached values: the oracle's function then
    differentiates what the reference does (pinned by the `pool` case of tests/golden/enc_grad.npz, the reference's own backward)."""
    amin = torch.Tensor.amin
    torch.Tensor.amin = lambda self, *a, **k: amin(self, *a, **k).detach()
    try:
        yield
    finally:
        torch.Tensor.amin = amin


def cm(x):
    return x.transpose(1, 2)


def oracle_dwconv3(x, mask, w, stride):
    """the oracle's masked_conv1d with groups = C, once per convolution -> (n, B, To, C)"""
    C = x.size(-1)
    return torch.stack([cm(O.masked_conv1d(cm(x), _m(mask, x)[:, None], w[i][:, None, :], None, stride, 1, C)[0]) for i in range(w.size(0))])


def oracle_pool(x, mask):
    with detached_fill():
        y, mo = O.masked_max_pool1d(cm(x), _m(mask, x)[:, None], 3, 2)
    return cm(y), mo[:, 0]


def oracle_encoder(sd, x, mask, stride, heads, window):
    """the oracle's transformer_encoder (state dict without prefix) on token-major x -> (y token-major, mask_out (B, To))"""
    with detached_fill():
        y, mo = O.transformer_encoder({'blk.' + k: v for k, v in sd.items()}, 'blk', cm(x), _m(mask, x)[:, None], stride, heads, window)
    return cm(y), mo[:, 0]


def holes(B, T, gen):
    """tests/test_gpu_conv_grad.py holes(): single invalid rows inside every sequence, a fully padded tail in the odd sequences"""
    m = torch.rand(B, T, generator=gen) > 0.15
    for b in range(1, B, 2):
        m[b, T - T // 4:] = False
    return m


def set_block_parameters(block, gen):
    """the fixture's parameter recipe (make_golden_enc_grad.py) on a TransformerEncoder of any width"""
    with torch.no_grad():
        for k, p in block.named_parameters():
            r = torch.randn(p.shape, generator=gen)
            if k.endswith('drop_path_attn.scale') or k.endswith('drop_path_ffn.scale'):
                p.copy_(0.5 + 0.25 * r)
            elif k.endswith('bias') or 'norm' in k or k.startswith('ln_'):
                p.add_(0.1 * r)
