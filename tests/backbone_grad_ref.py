"""Torch restatement of the closed forms the k = 5 / stride-2 kernels of csrc/conv_grad.hip implement (a helper module of
tests/test_backbone_grad_cpu.py and tests/test_gpu_backbone_grad.py), in the dtype of the operands, the oracle's functions behind
token-major adapters, and the reader of the tests/golden/backbone_grad_*.npz fixtures (make_golden_backbone_grad.py).

Tensors are token-major: x (B, T, Cin), T even, To = T / 2, mask (B, T) bool or None, w PyTorch's (N, Cin, 5), dy (B, To, N).

    Y[b,u,n]   = sum_{j=0..4} sum_c W[n,c,j] m[b,2u+j-2] X[b,2u+j-2,c]      taps stay inside sequence b; Y is not masked
    dW[n,c,j]  = sum_{b,u} dY[b,u,n] m[b,2u+j-2] X[b,2u+j-2,c]
    dX[b,t,c]  = m[b,t] sum_{j = t (mod 2), 0 <= (t+2-j)/2 < To} sum_n dY[b,(t+2-j)/2,n] W[n,c,j]
"""
import sys

import torch

from conftest import Golden, ROOT
from enc_grad_ref import detached_fill

if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import decafnet_ref as O  # noqa: E402

CASES = ('s4', 's2', 'pool')
ZERO_BY_SYMMETRY = ('attn.attn.key.bias', 'attn.k_norm.bias')


def _masked_padded(x, mask):
    B, T, C = x.shape
    xm = x if mask is None else x * mask.reshape(B, T, 1).to(x.dtype)
    return torch.cat([xm.new_zeros(B, 2, C), xm, xm.new_zeros(B, 2, C)], 1)          # row i holds (x m)[i - 2]


def conv5s2(x, mask, w):
    T = x.size(1)
    xp = _masked_padded(x, mask)
    return sum(xp[:, j:j + T:2] @ w[:, :, j].t() for j in range(5))                   # output row u reads xp[2 u + j]


def conv5s2_bwd_weight(x, mask, dy):
    T = x.size(1)
    xp = _masked_padded(x, mask)
    return torch.stack([torch.einsum('bun,buc->nc', dy, xp[:, j:j + T:2]) for j in range(5)], -1)


def conv5s2_bwd_data(dy, mask, w):
    """even rows t = 2 u take taps 0, 2, 4 of the output rows u + 1, u, u - 1; odd rows t = 2 u + 1 taps 1, 3 of u + 1, u"""
    B, To, N = dy.shape
    dp = torch.cat([dy.new_zeros(B, 1, N), dy, dy.new_zeros(B, 1, N)], 1)             # row i holds dY[i - 1]
    even = sum(dp[:, 2 - j // 2:2 - j // 2 + To] @ w[:, :, j] for j in (0, 2, 4))     # dY[u + 1 - j / 2]
    odd = sum(dp[:, 2 - j // 2:2 - j // 2 + To] @ w[:, :, j] for j in (1, 3))         # dY[u + (3 - j) / 2]
    dx = torch.stack([even, odd], 2).reshape(B, 2 * To, -1)
    return dx if mask is None else dx * mask.reshape(B, 2 * To, 1).to(dx.dtype)


# ------------------------------------------------------------------------------------------
# the oracle's functions on token-major tensors (they work on (B, C, T) and (B, 1, T))
# ------------------------------------------------------------------------------------------
def cm(x):
    return x.transpose(1, 2)


def _m(mask, x):
    return torch.ones(x.shape[:2], dtype=torch.bool) if mask is None else mask


def oracle_conv5s2(x, mask, w):
    """the oracle's masked_conv1d(..., stride=2, padding=2) -> (Y (B, To, N), the mask that goes on (B, To))"""
    y, mo = O.masked_conv1d(cm(x), _m(mask, x)[:, None], w, None, 2, 2)
    return cm(y), mo[:, 0]


def conv5s2_autograd(x, mask, w, dy):
    """(Y, dX, dW) by autograd through the oracle, in the dtype of the operands"""
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = oracle_conv5s2(xr, mask, wr)[0]
    gx, gw = torch.autograd.grad((y * dy).sum(), (xr, wr))
    return y.detach(), gx, gw


def oracle_video(sd, cfg, x, mask):
    """the oracle's video_transformer (state dict without prefix) -> (levels (B, T_l, E), masks (B, T_l))"""
    with detached_fill():
        fpn, masks = O.video_transformer({'vid_net.' + k: v for k, v in sd.items()}, cfg, cm(x), mask)
    return tuple(cm(f) for f in fpn), tuple(m[:, 0] for m in masks)


def oracle_text(sd, cfg, tokens, mask):
    """the oracle's text_transformer (state dict without prefix) -> ((B, L [+ 1], TE), mask (B, L [+ 1]))"""
    y, mo = O.text_transformer({'text_net.' + k: v for k, v in sd.items()}, cfg, cm(tokens), mask)
    return cm(y), mo[:, 0]


def holes(B, T, lens, gen):
    """single invalid rows inside every sequence and a padded tail from lens[b] on"""
    m = torch.rand(B, T, generator=gen) > 0.15
    for b, n in enumerate(lens):
        m[b, n:] = False
    return m


# ------------------------------------------------------------------------------------------
# the fixtures
# ------------------------------------------------------------------------------------------
class Fixture:
    """case `name` ('s4', 's2', 'pool' or 'text') of tests/golden/backbone_grad_<name>*.npz on token-major tensors in `dtype`:
    x (B, T, in_dim), mask (B, T), up / out[tag] / mask_out (tuples over the levels; one level for the text), gx[tag], gp[tag]
    {parameter: gradient}, sd (the backbone's state dict), cfg (the oracle's configuration), kw (the module's constructor arguments)"""

    def __init__(self, name, dtype):
        g = Golden(f'backbone_grad_{name}.npz')
        self.name, self.meta, self.text = name, g.js('meta'), name == 'text'
        self.kw = self.meta['kw']
        self.cfg = dict(self.kw)
        tm = lambda z: z.transpose(1, 2).contiguous()
        self.n_levels = self.meta['n_levels']
        self.x, self.mask = tm(g.t('x')).to(dtype), g.t('mask')
        self.up = tuple(tm(g.t(f'up{l}')).to(dtype) for l in range(self.n_levels))
        self.mask_out = tuple(g.t(f'mask_out{l}') for l in range(self.n_levels))
        self.out = {t: tuple(tm(g.t(f'out{t}_{l}')) for l in range(self.n_levels)) for t in ('32', '64')}
        self.gx = {t: tm(g.t(f'gx{t}')) for t in ('32', '64')}
        self.sd = {k: v.to(dtype) if v.is_floating_point() else v for k, v in g.sub('param/').items()}
        self.gp = {t: Golden(f'backbone_grad_{name}_gp{t}.npz').sub('') for t in ('32', '64')}
        assert len(self.sd) == self.meta['n_params'] == len(self.gp['64']) == len(self.gp['32'])

    def oracle(self, x, sd):
        if self.text:
            y, mo = oracle_text(sd, self.cfg, x, self.mask)
            return (y,), (mo,)
        return oracle_video(sd, self.cfg, x, self.mask)

    def oracle_grads(self):
        """(levels, masks, d x, {parameter: gradient}) by autograd through the oracle, in the fixture's dtype"""
        x = self.x.clone().requires_grad_(True)
        sd = {k: v.clone().requires_grad_(True) for k, v in self.sd.items()}
        ys, masks = self.oracle(x, sd)
        sum((y * u).sum() for y, u in zip(ys, self.up)).backward()
        return tuple(y.detach() for y in ys), masks, x.grad, {k: v.grad for k, v in sd.items()}

    def top(self, tag, k=None):
        """max |g_64| of the gradient rule for parameter `k`.  A constant added to every key moves all scores of a row alike, so the
        gradients of attn.attn.key.bias (every block, the stride-0 ones of the text encoder included) and of attn.k_norm.bias (the video
        blocks) are zero in exact arithmetic and the fixture holds rounding noise: their scale is that of the same layer's key.weight /
        k_norm.weight, the terms that cancel (ZERO_BY_SYMMETRY of tests/test_enc_grad_cpu.py and tests/test_dec_grad_cpu.py)"""
        for z in ZERO_BY_SYMMETRY:
            if k is not None and k.endswith(z):
                k = k[:-len('bias')] + 'weight'
        return float((self.gp['64'][k] if k is not None else tag).double().abs().max())


def set_backbone_parameters(module, gen):
    """the fixtures' parameter recipe (make_golden_backbone_grad.py) on a VideoTransformer / TextTransformer of any width"""
    with torch.no_grad():
        for k, p in module.named_parameters():
            r = torch.randn(p.shape, generator=gen)
            if k.endswith('drop_path_attn.scale') or k.endswith('drop_path_ffn.scale'):
                p.copy_(0.5 + 0.25 * r)
            elif k.endswith('bias') or 'norm' in k or '.ln_' in k:
                p.add_(0.1 * r)
