"""Torch restatement of the closed forms csrc/xattn_grad.hip implements (a helper module of tests/test_dec_grad_cpu.py and
tests/test_gpu_dec_grad.py), in the dtype of the operands, the oracle's functions behind token-major adapters, and the reader of the
tests/golden/dec_grad*.npz fixtures (make_golden_dec_grad.py).

Tensors are token-major: q (B, T, C), k / v (B, Lk, C) with the heads concatenated along C, kv_mask (B, Lk) bool or None.

    cross attention   s_tj = (scale q_t) . (scale k_j), scale = d^-1/4, -inf at a masked key;  p = softmax_j s;  O_t = sum_j p_tj v_j
                      dP_tj = dO_t . v_j,  delta_t = sum_j p_tj dP_tj,  dS_tj = p_tj (dP_tj - delta_t)
                      dQ_t = scale^2 sum_j dS_tj k_j,  dK_j = scale^2 sum_t dS_tj q_t,  dV_j = sum_t p_tj dO_t
    AdaLN             Y = N(X m) * H[..., :C] + H[..., C:],  N = the affine-free channel LayerNorm (eps 1e-5) or the identity
                      dH[..., :C] = dY * N(X m),  dH[..., C:] = dY,  dX = m LN'(dY * H[..., :C])
"""
import sys

import torch

from conftest import Golden, ROOT

if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import decafnet_ref as O  # noqa: E402

EPS = 1e-5


def _split(z, heads):
    B, T, C = z.shape
    return z.reshape(B, T, heads, C // heads).permute(0, 2, 1, 3)              # (B, h, T, d)


def _merge(z):
    B, h, T, d = z.shape
    return z.permute(0, 2, 1, 3).reshape(B, T, h * d)


def _probabilities(q, k, kv_mask, heads):
    scale = (q.size(-1) // heads) ** -0.25
    s = torch.einsum('bhtd,bhjd->bhtj', _split(q, heads) * scale, _split(k, heads) * scale)
    if kv_mask is not None:
        s = s.masked_fill(~kv_mask[:, None, None, :], float('-inf'))
    return torch.softmax(s, dim=-1), scale


def cross_attention(q, k, v, kv_mask, heads):
    """O (B, T, C); differentiable"""
    p, _ = _probabilities(q, k, kv_mask, heads)
    return _merge(torch.einsum('bhtj,bhjd->bhtd', p, _split(v, heads)))


def cross_attention_grads(q, k, v, kv_mask, dO, heads):
    """(dQ, dK, dV) by the closed forms above"""
    p, scale = _probabilities(q, k, kv_mask, heads)
    qh, kh, vh, gh = (_split(z, heads) for z in (q, k, v, dO))
    dP = torch.einsum('bhtd,bhjd->bhtj', gh, vh)
    delta = (p * dP).sum(-1, keepdim=True)
    dS = p * (dP - delta)
    dQ = scale * scale * torch.einsum('bhtj,bhjd->bhtd', dS, kh)
    dK = scale * scale * torch.einsum('bhtj,bhtd->bhjd', dS, qh)
    dV = torch.einsum('bhtj,bhtd->bhjd', p, gh)
    return _merge(dQ), _merge(dK), _merge(dV)


def _m(mask, x):
    return torch.ones(x.shape[:2], dtype=torch.bool) if mask is None else mask


def _norm(xm, norm):
    """(N(xm), 1 / sqrt(var + eps) or None)"""
    if not norm:
        return xm, None
    xc = xm - xm.mean(-1, keepdim=True)
    rs = 1.0 / torch.sqrt((xc * xc).mean(-1, keepdim=True) + EPS)
    return xc * rs, rs


def adaln(x, mask, h, norm=True):
    C = x.size(-1)
    xh, _ = _norm(x * _m(mask, x)[..., None].to(x.dtype), norm)
    return xh * h[..., :C] + h[..., C:]


def adaln_grads(x, mask, h, dy, norm=True):
    """(dX, dH)"""
    C = x.size(-1)
    m = _m(mask, x)[..., None].to(x.dtype)
    xh, rs = _norm(x * m, norm)
    dh = torch.cat([dy * xh, dy], dim=-1)
    g = dy * h[..., :C]
    if norm:
        g = rs * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    return g * m, dh


# ------------------------------------------------------------------------------------------
# the oracle's functions on token-major tensors (they work on (B, C, T) and (B, 1, T))
# ------------------------------------------------------------------------------------------
def cm(x):
    return x.transpose(1, 2)


def identity_projections(C, dtype):
    """a state dict that makes the four projections of the oracle's MaskedMHA the identity: what is left is the attention core"""
    eye, zero = torch.eye(C, dtype=dtype)[:, :, None], torch.zeros(C, dtype=dtype)
    return {f'a.{n}.{w}': (eye if w == 'weight' else zero) for n in ('query', 'key', 'value', 'proj') for w in ('weight', 'bias')}


def oracle_cross_attention(q, k, v, kv_mask, heads):
    """the oracle's _mha_global_qkv with identity projections -> O (B, T, C)"""
    B, Lk, C = k.shape
    km = torch.ones(B, Lk, dtype=torch.bool) if kv_mask is None else kv_mask
    return cm(O._mha_global_qkv(identity_projections(C, q.dtype), 'a', cm(q), cm(k), cm(v), km[:, None], heads))


def oracle_adaln(x, mask, h, norm=True):
    """blocks.py:643-645 through the oracle's channel_layer_norm"""
    C = x.size(-1)
    xm = cm(x * _m(mask, x)[..., None].to(x.dtype))
    xh = O.channel_layer_norm(xm) if norm else xm
    return cm(xh) * h[..., :C] + h[..., C:]


def oracle_decoder(sd, vid, vid_mask, text, text_mask, heads, adaln_mode=True, kv_size=None):
    """the oracle's transformer_decoder (state dict without prefix) on token-major tensors -> y (B', T, E).  The oracle has no kv_size:
    everything it does to the query before the attention is per sequence, so repeating the video first is the same function."""
    if kv_size is not None:
        vid, vid_mask = vid.repeat_interleave(kv_size, dim=0), vid_mask.repeat_interleave(kv_size, dim=0)
    y, _ = O.transformer_decoder({'blk.' + k: v for k, v in sd.items()}, 'blk', cm(vid), vid_mask[:, None], cm(text), text_mask[:, None], heads, adaln_mode)
    return cm(y), vid_mask


def oracle_fusion(sd, vid, vid_mask, text, text_mask, heads, layers, adaln_mode=True, kv_size=None):
    """XAttNFusion._forward (fusion.py:56-66) through the oracle's transformer_decoder and channel_layer_norm"""
    for i in range(layers):
        p = f'layers.{i}.'
        vid, vid_mask = oracle_decoder({k[len(p):]: v for k, v in sd.items() if k.startswith(p)}, vid, vid_mask, text, text_mask, heads, adaln_mode,
                                       kv_size if vid.size(0) != text.size(0) else None)
    return cm(O.channel_layer_norm(cm(vid), sd['ln_out.weight'], sd['ln_out.bias'])), vid_mask


def holes(B, L, gen):
    """key masks with holes; every sequence keeps at least one valid key"""
    m = torch.rand(B, L, generator=gen) > 0.25
    m[torch.arange(B), torch.randint(0, L, (B,), generator=gen)] = True
    return m


# ------------------------------------------------------------------------------------------
# the fixture
# ------------------------------------------------------------------------------------------
class Fixture:
    """case `name` of tests/golden/dec_grad*.npz on token-major tensors in `dtype`: vid (B, T, E), vid_mask (B, T), text (B', Lk, TE),
    text_mask (B', Lk), up (B', T, E), kv_size (B,) or None, sd (the state dict: of the stack, or of layer 0 for `single`), and
    out / gvid / gtext / gp by precision tag '32' / '64' (token-major, in the precision they were recorded in)"""

    def __init__(self, name, dtype):
        g = Golden('dec_grad.npz')
        self.meta, self.name = g.js('meta'), name
        self.single = name == 'single'
        self.adaln = self.meta['cases'][name] == 'adaln'
        self.heads, self.layers = self.meta['heads'], self.meta['layers']
        tm = lambda z: z.transpose(1, 2).contiguous()
        self.vid, self.text, self.up = (tm(g.t(f'{name}/{k}')).to(dtype) for k in ('vid', 'text', 'up'))
        self.vid_mask, self.text_mask = g.t(f'{name}/vid_mask'), g.t(f'{name}/text_mask')
        self.kv_size = None if self.single else g.t(f'{name}/kv_size')
        self.mask_out = g.t(f'{name}/mask_out')
        sd = {k: v.to(dtype) for k, v in g.sub('param/').items()}
        self.sd = {k[len('layers.0.'):]: v for k, v in sd.items() if k.startswith('layers.0.')} if self.single else sd
        self.out = {t: tm(g.t(f'{name}/out{t}')) for t in ('32', '64')}
        self.gvid = {t: tm(g.t(f'{name}/gvid{t}')) for t in ('32', '64')}
        self.gtext = {t: tm(g.t(f'{name}/gtext{t}')) for t in ('32', '64')}
        self.gp = {t: Golden(f'dec_grad_{name}_gp{t}.npz').sub('') for t in ('32', '64')}
        assert len(self.sd) == (self.meta['n_layer_params'] if self.single else self.meta['n_params'])

    def oracle(self, vid, text, sd):
        if self.single:
            return oracle_decoder(sd, vid, self.vid_mask, text, self.text_mask, self.heads, self.adaln)[0]
        return oracle_fusion(sd, vid, self.vid_mask, text, self.text_mask, self.heads, self.layers, self.adaln, self.kv_size)[0]

    def oracle_grads(self):
        """(out, d vid, d text, {parameter: gradient}) by autograd through the oracle, in the fixture's dtype"""
        vid, text = self.vid.clone().requires_grad_(True), self.text.clone().requires_grad_(True)
        sd = {k: v.clone().requires_grad_(True) for k, v in self.sd.items()}
        y = self.oracle(vid, text, sd)
        (y * self.up).sum().backward()
        return y.detach(), vid.grad, text.grad, {k: v.grad for k, v in sd.items()}


def set_fusion_parameters(module, gen):
    """the fixture's parameter recipe (make_golden_dec_grad.py) on a TransformerDecoder / XAttNFusion of any width"""
    with torch.no_grad():
        for k, p in module.named_parameters():
            r = torch.randn(p.shape, generator=gen)
            if k.endswith('drop_path_ffn.scale'):
                p.copy_(0.5 + 0.25 * r)
            elif k.endswith('bias') or 'norm' in k or 'ln_' in k:
                p.add_(0.1 * r)
