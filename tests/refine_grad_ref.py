"""Torch restatement of the closed forms csrc/refine_grad.hip implements (a helper module of tests/test_refine_grad_cpu.py and
tests/test_gpu_refine_grad.py), in the dtype of the operands, the oracle's functions behind token-major adapters, and the reader of the
tests/golden/refine_grad*.npz fixtures (make_golden_refine_grad.py).

Tensors are token-major: x (B, T0, 32), mask (B, T0) bool or None, logits1 (B, S) with level l at offset sum_{j<l} T0 >> j.

    refine_in   u[b,t,0] = logits1[b,0,t],  u[b,t,l] = m0[b,t] logits1[b,l,t >> l];  H = u W_in^T + b_in
                dU = (dH W_in) * (1 | m0),  dlogits1[b,l,s] = sum_{t >> l == s} dU[b,t,l],  dW_in = dH^T u,  db_in = sum dH
    tcn_layer   X_j = X shifted by (j - 1) d inside the sequence;  h = relu(bd + sum_j X_j Wd[:,:,j]^T);  o = keep / (1 - p) (h Wp^T + bp)
                z = (X + o) m;  Y = zhat ln_w + ln_b,  zhat = (z - mean) rs
                g = dY ln_w,  dz = m rs (g - mean g - zhat mean(g zhat)),  do = dz keep / (1 - p),  dh = (h > 0) (do Wp)
                dX = dz + sum_j (dh Wd[:,:,j]) shifted by -(j - 1) d,  dWd[:,:,j] = dh^T X_j,  dbd = sum dh,  dWp = do^T h,  dbp = sum do,
                dln_w = sum dY zhat,  dln_b = sum dY
"""
import sys

import numpy as np
import torch

from conftest import Golden, ROOT
import philox_ref as PH

if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import decafnet_ref as O  # noqa: E402

EPS = 1e-5
C = 32
LAYER_PARAMS = ('conv_dilated.weight', 'conv_dilated.bias', 'conv_1x1.weight', 'conv_1x1.bias', 'norm.weight', 'norm.bias')
GRAD_NAMES = ('dX', 'dWd', 'dbd', 'dWp', 'dbp', 'dlnw', 'dlnb')


def sizes(T0, L):
    return [T0 >> l for l in range(L)]


def _mf(mask, like):
    return torch.ones(like.shape[:2], dtype=like.dtype) if mask is None else mask.to(like.dtype)


def stack(logits1, mask0, T0, L):
    """u (B, T0, L); differentiable"""
    m = _mf(mask0, logits1.new_zeros(logits1.size(0), T0))
    cols, off = [], 0
    idx = torch.arange(T0)
    for l in range(L):
        col = logits1[:, off + (idx >> l)]
        cols.append(col if l == 0 else col * m)
        off += T0 >> l
    return torch.stack(cols, dim=-1)


def refine_in(logits1, mask0, W, b, T0):
    W = W.reshape(C, -1)
    return stack(logits1, mask0, T0, W.size(1)) @ W.t() + b


def refine_in_grads(logits1, mask0, W, dH):
    """(dlogits1, dW_in, db_in)"""
    W = W.reshape(C, -1)
    B, T0, _ = dH.shape
    L = W.size(1)
    u = stack(logits1, mask0, T0, L)
    dU = dH @ W
    m = _mf(mask0, dH)
    parts = []
    for l in range(L):
        col = dU[..., l] if l == 0 else dU[..., l] * m
        parts.append(col.reshape(B, T0 >> l, 1 << l).sum(-1))
    return torch.cat(parts, dim=1), torch.einsum('btc,btl->cl', dH, u), dH.sum((0, 1))


def shift(x, s):
    """y[:, t] = x[:, t + s], zero outside the sequence"""
    B, T, _ = x.shape
    y = torch.zeros_like(x)
    if abs(s) < T:
        if s >= 0:
            y[:, :T - s] = x[:, s:]
        else:
            y[:, -s:] = x[:, :T + s]
    return y


def keep_scale(drop, layer, B, T0):
    """keep / (1 - p) of the training forward as a (B, T0, 32) float32 tensor, `drop` = (seed, p, b0) or None -> None"""
    if drop is None or drop[1] <= 0:
        return None
    seed, p, b0 = drop
    keep = PH.dropout_mask(seed, PH.site(PH.G_REFINE, layer, PH.TCN), (b0 + B, C, T0), p)[b0:]
    return torch.from_numpy(np.ascontiguousarray(keep.transpose(0, 2, 1)).astype(np.float32) * PH.scale(p))


def _layer_forward(x, mask, P, dil, ks):
    wd, bd, wp, bp, lnw, lnb = P
    wp = wp.reshape(C, C)
    taps = [shift(x, (j - 1) * dil) for j in range(3)]
    h = torch.relu(bd + sum(taps[j] @ wd[:, :, j].t() for j in range(3)))
    o = h @ wp.t() + bp
    if ks is not None:
        o = o * ks.to(x.dtype)
    z = (x + o) * _mf(mask, x)[..., None]
    zc = z - z.mean(-1, keepdim=True)
    rs = 1.0 / torch.sqrt((zc * zc).mean(-1, keepdim=True) + EPS)
    return taps, h, zc * rs, rs


def tcn_layer(x, mask, P, dil, ks=None):
    """Y (B, T0, 32); P = (Wd, bd, Wp, bp, ln_w, ln_b); ks = keep_scale(...) or None; differentiable"""
    _, _, zh, _ = _layer_forward(x, mask, P, dil, ks)
    return zh * P[4] + P[5]


def tcn_layer_grads(x, mask, P, dil, dY, ks=None):
    """(dX, dWd, dbd, dWp, dbp, dln_w, dln_b) by the closed forms above"""
    wd, wp, lnw = P[0], P[2].reshape(C, C), P[4]
    taps, h, zh, rs = _layer_forward(x, mask, P, dil, ks)
    g = dY * lnw
    dz = _mf(mask, x)[..., None] * rs * (g - g.mean(-1, keepdim=True) - zh * (g * zh).mean(-1, keepdim=True))
    do = dz if ks is None else dz * ks.to(x.dtype)
    dh = (do @ wp) * (h > 0).to(x.dtype)
    dX = dz + sum(shift(dh @ wd[:, :, j], -(j - 1) * dil) for j in range(3))
    dWd = torch.stack([torch.einsum('bto,bti->oi', dh, taps[j]) for j in range(3)], dim=-1)
    return (dX, dWd, dh.sum((0, 1)), torch.einsum('bto,bti->oi', do, h).reshape(P[2].shape), do.sum((0, 1)), (dY * zh).sum((0, 1)), dY.sum((0, 1)))


def layer_params(sd, i, p='refine'):
    return tuple(sd[f'{p}.layers.{i}.{k}'] for k in LAYER_PARAMS)


def tcn(logits1, mask0, sd, T0, L, drop=None, p='refine'):
    """the whole refinement TCN by the closed forms: (out (B, T0, 32), the input of every layer)"""
    x = refine_in(logits1, mask0, sd[p + '.conv_1x1.weight'], sd[p + '.conv_1x1.bias'], T0)
    xs = []
    for i in range(L):
        xs.append(x)
        x = tcn_layer(x, mask0, layer_params(sd, i, p), 2 ** i, keep_scale(drop, i, x.size(0), T0))
    xs.append(x)
    return (x @ sd[p + '.conv_out.weight'].reshape(C, C).t() + sd[p + '.conv_out.bias']) * _mf(mask0, x)[..., None], xs


def tcn_grads(logits1, mask0, sd, T0, L, dOut, drop=None, p='refine'):
    """(dlogits1, {parameter: gradient}) of the whole TCN, chained from the closed forms of its parts"""
    _, xs = tcn(logits1, mask0, sd, T0, L, drop, p)
    gm = dOut * _mf(mask0, dOut)[..., None]
    wo = sd[p + '.conv_out.weight']
    gp = {p + '.conv_out.weight': torch.einsum('bto,bti->oi', gm, xs[-1]).reshape(wo.shape), p + '.conv_out.bias': gm.sum((0, 1))}
    g = gm @ wo.reshape(C, C)
    for i in reversed(range(L)):
        out = tcn_layer_grads(xs[i], mask0, layer_params(sd, i, p), 2 ** i, g, keep_scale(drop, i, g.size(0), T0))
        g = out[0]
        for k, v in zip(LAYER_PARAMS, out[1:]):
            gp[f'{p}.layers.{i}.{k}'] = v
    dl, dW, db = refine_in_grads(logits1, mask0, sd[p + '.conv_1x1.weight'], g)
    gp[p + '.conv_1x1.weight'], gp[p + '.conv_1x1.bias'] = dW.reshape(sd[p + '.conv_1x1.weight'].shape), db
    return dl, gp


# ------------------------------------------------------------------------------------------
# the oracle's functions on token-major tensors (they work on (B, C, T) and (B, 1, T))
# ------------------------------------------------------------------------------------------
def cm(x):
    return x.transpose(1, 2)


def oracle_tcn(sd, u, mask0, L, p='refine'):
    """the oracle's tcn_refine on the stacked input u (B, T0, L) -> (B, T0, 32)"""
    m = torch.ones(u.shape[:2], dtype=torch.bool) if mask0 is None else mask0
    return cm(O.tcn_refine(sd, p, cm(u), m[:, None], L))


def oracle_layer(P, x, mask, dtype=None):
    """one DilatedResidualLayer of dilation 1 through the oracle's tcn_refine: a one-layer TCN whose conv_1x1 and conv_out are the
    identity -> Y * mask (tcn_refine masks its output)"""
    eye, zero = torch.eye(C, dtype=x.dtype)[:, :, None], torch.zeros(C, dtype=x.dtype)
    sd = {'r.conv_1x1.weight': eye, 'r.conv_1x1.bias': zero, 'r.conv_out.weight': eye, 'r.conv_out.bias': zero}
    sd.update({f'r.layers.0.{k}': v for k, v in zip(LAYER_PARAMS, P)})
    return oracle_tcn(sd, x, mask, 1, 'r')


def oracle_fuse_and_predict(sd, cfg, fpn, masks):
    """the oracle's fuse_and_predict (second_fusion off) on token-major levels -> (logits1, logits2, offsets) per level, (B, T_l[, 2])"""
    l1, l2, off, _ = O.fuse_and_predict(sd, cfg, [cm(x) for x in fpn], [m[:, None] for m in masks])
    return list(l1), list(l2), list(off)


def random_layer(gen, dtype=torch.float32):
    """(Wd, bd, Wp, bp, ln_w, ln_b) at the scale of PyTorch's initialisation, biases and LayerNorm weights off their initial values"""
    r = lambda *s: torch.randn(*s, generator=gen)
    P = (r(C, C, 3) / 96 ** 0.5, 0.1 * r(C), r(C, C, 1) / 32 ** 0.5, 0.1 * r(C), 1 + 0.1 * r(C), 0.1 * r(C))
    return tuple(t.to(dtype) for t in P)


def tail_mask(B, T0, gen):
    """padded tails: every sequence keeps at least one row, the first keeps all"""
    lens = torch.randint(1, T0 + 1, (B,), generator=gen)
    lens[0] = T0
    return torch.arange(T0)[None, :] < lens[:, None]


# ------------------------------------------------------------------------------------------
# the fixture
# ------------------------------------------------------------------------------------------
class Fixture:
    """tests/golden/refine_grad*.npz on token-major tensors in `dtype`: fpn[l] (B, T_l, E), masks[l] (B, T_l), up1 / up2 / up3 per level,
    sd (the parameters of cls_head, refine, cls_head2, reg_head), cfg for the oracle, and by precision tag '32' / '64' logits1 /
    logits2 / offsets / gfpn per level (token-major) and gp (parameter -> gradient), in the precision they were recorded in"""

    def __init__(self, dtype):
        g = Golden('refine_grad.npz')
        self.meta, self.opt_kwargs = g.js('meta'), g.js('opt_kwargs')
        self.L, self.T0 = self.meta['L'], self.meta['T0']
        lv = range(self.L)
        self.fpn = [cm(g.t(f'fpn/l{l}')).contiguous().to(dtype) for l in lv]
        self.masks = [g.t(f'mask/l{l}') for l in lv]
        self.up = {k: [g.t(f'{k}/l{l}').to(dtype) for l in lv] for k in ('up1', 'up2', 'up3')}
        self.sd = {k: v.to(dtype) for k, v in g.sub('param/').items()}
        self.cfg = {'vid_net': {'arch': (2, 0, self.L)}, 'cls_head': {'n_layers': 2}, 'reg_head': {'n_layers': 2}}
        self.out = {t: {k: [g.t(f'{k}_{t}/l{l}') for l in lv] for k in ('logits1', 'logits2', 'offsets')} for t in ('32', '64')}
        self.gfpn = {t: [cm(g.t(f'gfpn_{t}/l{l}')).contiguous() for l in lv] for t in ('32', '64')}
        self.gp = {t: Golden(f'refine_grad_gp{t}.npz').sub('') for t in ('32', '64')}
        assert len(self.sd) == self.meta['n_params'] == len(self.gp['64'])

    def scalar(self, l1, l2, off):
        return sum((a * u.to(a.device)).sum() for outs, k in ((l1, 'up1'), (l2, 'up2'), (off, 'up3')) for a, u in zip(outs, self.up[k]))

    def oracle_grads(self):
        """((logits1, logits2, offsets), d fpn, {parameter: gradient}) by autograd through the oracle, in the fixture's dtype"""
        fpn = [x.clone().requires_grad_(True) for x in self.fpn]
        sd = {k: v.clone().requires_grad_(True) for k, v in self.sd.items()}
        outs = oracle_fuse_and_predict(sd, self.cfg, fpn, self.masks)
        self.scalar(*outs).backward()
        return {k: [o.detach() for o in v] for k, v in zip(('logits1', 'logits2', 'offsets'), outs)}, [x.grad for x in fpn], {k: v.grad for k, v in sd.items()}
