"""fp64-capable torch-CPU restatement of what csrc/conv_grad.hip differentiates, written from the forward contract alone:

    Y[b,t,n] = bias[n] + sum_{j<k} sum_c W[n,c,j] m[b,t+j-p] X[b,t+j-p,c],   k in {1, 3}, p = (k - 1) / 2,

taps never leave sequence b and the output is not masked (libs/modeling/blocks.py:87-106), and the channel LayerNorm of
blocks.py:125-131 (two-pass, eps inside the square root) optionally followed by ReLU.  Tensors are token-major (B, T, C); the
functions run in the dtype of their inputs, so the same code is the fp64 yardstick and the fp32 CPU comparison.  Gradients come
from autograd through these expressions and, independently, from the closed forms below."""
import torch


def conv(x, mask, w, bias=None):
    B, T, C = x.shape
    N, Cw, k = w.shape
    assert Cw == C and k in (1, 3)
    p = (k - 1) // 2
    xm = x if mask is None else x * mask.reshape(B, T, 1).to(x.dtype)
    xp = torch.cat([xm.new_zeros(B, p, C), xm, xm.new_zeros(B, p, C)], 1)
    y = sum(xp[:, j:j + T] @ w[:, :, j].t() for j in range(k))
    return y if bias is None else y + bias


def layer_norm(x, w, b, relu=False, eps=1e-5):
    x = x - x.mean(-1, keepdim=True)
    x = x / torch.sqrt((x * x).mean(-1, keepdim=True) + eps)
    if w is not None:
        x = x * w.reshape(-1) + b.reshape(-1)
    return torch.relu(x) if relu else x


def head(x, mask, params, level=None):
    """ClsHead / RegHead of libs/modeling/head.py for one level; params: the head's state_dict"""
    n = len([k for k in params if k.startswith('norms.') and k.endswith('.weight')])
    for i in range(n):
        x = conv(x, mask, params[f'convs.{i}.conv.weight'])
        x = layer_norm(x, params[f'norms.{i}.weight'], params[f'norms.{i}.bias'], relu=True)
    if 'reg_head.conv.weight' in params:
        return torch.relu(params[f'scales.{level}.scale'] * conv(x, mask, params['reg_head.conv.weight'], params['reg_head.conv.bias']))
    return conv(x, mask, params['cls_head.conv.weight'], params['cls_head.conv.bias']).squeeze(-1)


# ---- closed forms (what the kernels compute), for the finite-difference check and the operator tests ----
def conv_bwd_data(dy, mask, w):
    B, T, N = dy.shape
    _, C, k = w.shape
    p = (k - 1) // 2
    dp = torch.cat([dy.new_zeros(B, p, N), dy, dy.new_zeros(B, p, N)], 1)
    dx = sum(dp[:, 2 * p - j:2 * p - j + T] @ w[:, :, j] for j in range(k))      # dY[t - j + p]
    return dx if mask is None else dx * mask.reshape(B, T, 1).to(dx.dtype)


def conv_bwd_weight(x, mask, dy, k):
    B, T, C = x.shape
    p = (k - 1) // 2
    xm = x if mask is None else x * mask.reshape(B, T, 1).to(x.dtype)
    xp = torch.cat([xm.new_zeros(B, p, C), xm, xm.new_zeros(B, p, C)], 1)
    dw = torch.stack([torch.einsum('btn,btc->nc', dy, xp[:, j:j + T]) for j in range(k)], -1)
    return dw, dy.sum((0, 1))


def conv_grads(x, mask, w, dy):
    """(dX, dW, db) of `conv` by the closed forms"""
    dw, db = conv_bwd_weight(x, mask, dy, w.shape[-1])
    return conv_bwd_data(dy, mask, w), dw, db


def layer_norm_grads(x, w, b, dout, relu=False, eps=1e-5):
    """(dX, dw, db) of `layer_norm` by the closed form; the ReLU passes the gradient where out > 0"""
    C = x.shape[-1]
    xc = x - x.mean(-1, keepdim=True)
    rs = 1.0 / torch.sqrt((xc * xc).mean(-1, keepdim=True) + eps)
    xh = xc * rs
    dy = dout
    if relu:
        dy = torch.where(xh * w.reshape(-1) + b.reshape(-1) > 0, dout, torch.zeros_like(dout))
    dh = dy * w.reshape(-1)
    dx = rs * (dh - dh.mean(-1, keepdim=True) - xh * (dh * xh).mean(-1, keepdim=True))
    return dx, (dy * xh).reshape(-1, C).sum(0), dy.reshape(-1, C).sum(0)
