"""The sliding-window attention core and its gradient restated in torch, for any dtype (what csrc/attn_grad.hip computes), and the
local-window MaskedMHA over a state dict.

Per sequence b, head h (head dimension d), query row t, half = window // 2, scale = d^-1/4 on q and on k:

    s_tj = (scale q_t) . (scale k_j) + pen_j     |j - t| <= half, 0 <= j < T;   pen_j = -1e4 at a padded key (blocks.py:279), else 0
    p_t. = softmax_j s_tj,  O_t = sum_j p_tj v_j;   p_t. = 0 and O_t = 0 at a padded QUERY row (blocks.py:293)
    dP_tj = dO_t . v_j,  delta_t = sum_j p_tj dP_tj,  dS_tj = p_tj (dP_tj - delta_t)
    dV_j = sum_t p_tj dO_t,  dQ_t = scale^2 sum_j dS_tj k_j,  dK_j = scale^2 sum_t dS_tj q_t

Tensors are token-major (B, T, C) with the heads concatenated along C; ``mask`` is (B, T) bool or None."""
import torch


def _split(z, heads):
    B, T, C = z.shape
    return z.reshape(B, T, heads, C // heads).permute(0, 2, 1, 3)              # (B, h, T, d)


def _merge(z):
    B, h, T, d = z.shape
    return z.permute(0, 2, 1, 3).reshape(B, T, h * d)


def _band(T, window):
    """(clamped key index (T, w), key exists (T, w))"""
    half = window // 2
    pos = torch.arange(T)[:, None] + torch.arange(-half, half + 1)[None, :]
    return pos.clamp(0, T - 1), (pos >= 0) & (pos < T)


def _probabilities(q, k, mask, heads, window):
    """p (B, h, T, w), the window's keys kw (B, h, T, w, d) unscaled, the band"""
    B, T, C = q.shape
    scale = (C // heads) ** -0.25
    idx, exists = _band(T, window)
    mask = torch.ones(B, T, dtype=torch.bool) if mask is None else mask.reshape(B, T).bool()
    kw = _split(k, heads)[:, :, idx]                                            # (B, h, T, w, d)
    s = torch.einsum('bhtd,bhtwd->bhtw', _split(q, heads) * scale, kw * scale)
    pen = torch.zeros(B, T, idx.size(1), dtype=q.dtype).masked_fill(~mask[:, idx], -1e4)
    s = (s + pen[:, None]).masked_fill(~exists, float('-inf'))
    p = torch.softmax(s, dim=-1).masked_fill(~mask[:, None, :, None], 0.0)
    return p, kw, idx, scale


def window_attention(q, k, v, mask, heads, window):
    """O (B, T, C); differentiable"""
    p, _, idx, _ = _probabilities(q, k, mask, heads, window)
    return _merge(torch.einsum('bhtw,bhtwd->bhtd', p, _split(v, heads)[:, :, idx]))


def window_attention_grads(q, k, v, mask, dO, heads, window):
    """(dQ, dK, dV) by the closed forms above"""
    B, T, C = q.shape
    p, kw, idx, scale = _probabilities(q, k, mask, heads, window)
    qh, gh = _split(q, heads), _split(dO, heads)
    dP = torch.einsum('bhtd,bhtwd->bhtw', gh, _split(v, heads)[:, :, idx])
    delta = (p * dP).sum(-1, keepdim=True)
    dS = p * (dP - delta)                                                       # 0 where the key does not exist: p = 0 there
    dQ = scale * scale * torch.einsum('bhtw,bhtwd->bhtd', dS, kw)
    flat = idx.reshape(-1)
    dK = torch.zeros_like(qh).index_add_(2, flat, (dS[..., None] * qh[:, :, :, None, :]).flatten(2, 3)) * (scale * scale)
    dV = torch.zeros_like(qh).index_add_(2, flat, (p[..., None] * gh[:, :, :, None, :]).flatten(2, 3))
    return _merge(dQ), _merge(dK), _merge(dV)


def conv1(x, sd, name):
    """nn.Conv1d(k = 1) on token-major rows: the reference's projections do not mask their input"""
    return x @ sd[name + '.weight'][:, :, 0].t() + sd[name + '.bias']


def masked_mha(q_in, k_in, v_in, mask, sd, heads, window):
    """MaskedMHA.forward, local branch without dropout (blocks.py:348-373, :391-392), on token-major (B, T, C) inputs"""
    ctx = window_attention(conv1(q_in, sd, 'query'), conv1(k_in, sd, 'key'), conv1(v_in, sd, 'value'), mask, heads, window)
    return conv1(ctx, sd, 'proj')
