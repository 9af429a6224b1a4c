"""Differentiable MaskedConv1D and channel LayerNorm on the MI355X, and a prediction head composed of them.

``masked_conv1d`` and ``channel_layer_norm`` are ``torch.autograd.Function``s over the library's single-operator entry points:
the forwards are the kernels the network's forward runs (dcf_op_conv3_split / dcf_op_linear_split / dcf_op_layernorm), the
backwards are dcf_op_conv_bwd_data / dcf_op_conv_bwd_weight / dcf_op_layernorm_bwd (csrc/conv_grad.hip), all on the current
stream and without a host wait.  Tensors are token-major ``(B, T, C)`` fp32 on the GPU; there is no CPU path.

``conv_head`` runs one pyramid level through a ClsHead / RegHead (libs/modeling/head.py:53-64, :95-108) built from the two, so a
head trains end to end with ``loss.PointObjective``.  It is a demonstration of the operators, not the training forward:
``forward(..., eval=False)`` still returns plain tensors and the gradient of the network stops at the pyramid features.
"""
import torch

from . import _lib

_F16X3 = 16
_PAD_N = 32        # the forward GEMMs need N % 32 == 0: the heads' 1- and 2-channel output convolutions run zero-padded to 32


def _rows(x, name):
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 3):
        raise RuntimeError(f'{name}: a (B, T, C) tensor on the GPU is required (there is no CPU path)')
    return x.detach().float().contiguous()


def _mask_rows(mask, B, T):
    if mask is None:
        return None
    m = mask.detach().reshape(B, T)
    return (m if m.dtype == torch.bool else m != 0).contiguous()


def _conv_forward(x, m, w, B, T):
    """Y (B, T, N) = conv(x * m) without the bias, through the forward's split-operand kernels"""
    N, Cin, k = w.shape
    wf = w
    if N % 32:
        wf = torch.zeros(_PAD_N, Cin, k, dtype=w.dtype, device=w.device)
        wf[:N] = w
    Np = wf.size(0)
    y = torch.empty(B, T, Np, dtype=torch.float32, device=x.device)
    L, st = _lib.lib(), _lib.current_stream()
    if k == 3:
        _lib.check(L.dcf_op_conv3_split(_lib.ptr(x), _lib.ptr(m), _lib.ptr(wf.contiguous()), _lib.ptr(y), B, T, Cin, Np, _F16X3, st),
                   'dcf_op_conv3_split')
    else:
        xm = x if m is None else x * m[..., None].to(x.dtype)
        _lib.check(L.dcf_op_linear_split(_lib.ptr(xm), _lib.ptr(wf.reshape(Np, Cin).contiguous()), None, _lib.ptr(y), B * T, Np, Cin, 0, _F16X3, st),
                   'dcf_op_linear_split')
    return y if Np == N else y[..., :N].contiguous()


class _MaskedConv1dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mask, weight, bias):
        B, T, Cin = x.shape
        N, Cw, k = weight.shape
        if Cw != Cin or k not in (1, 3):
            raise ValueError(f'masked_conv1d: weight {tuple(weight.shape)} on {Cin} channels (k = 1 or 3, groups = 1)')
        xd, wd = _rows(x, 'masked_conv1d'), weight.detach().float().contiguous()
        m = _mask_rows(mask, B, T)
        y = _conv_forward(xd, m, wd, B, T)
        if bias is not None:
            y = y + bias.detach().float()
        ctx.save_for_backward(xd, m, wd)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        x, m, w = ctx.saved_tensors
        B, T, Cin = x.shape
        N, _, k = w.shape
        gy = gy.float().contiguous()
        L, st = _lib.lib(), _lib.current_stream()
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x)
            _lib.check(L.dcf_op_conv_bwd_data(_lib.ptr(gy), _lib.ptr(m), _lib.ptr(w), _lib.ptr(gx), B, T, Cin, N, k, st), 'dcf_op_conv_bwd_data')
        want_b = ctx.has_bias and ctx.needs_input_grad[3]
        if ctx.needs_input_grad[2]:
            gw = torch.empty_like(w)
            gb = torch.empty(N, dtype=torch.float32, device=x.device) if want_b else None
            _lib.check(L.dcf_op_conv_bwd_weight(_lib.ptr(x), _lib.ptr(m), _lib.ptr(gy), _lib.ptr(gw), _lib.ptr(gb), B, T, Cin, N, k, 0, st),
                       'dcf_op_conv_bwd_weight')
        elif want_b:
            gb = gy.sum((0, 1))
        return gx, None, gw, gb


class _ChannelLayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, relu):
        B, T, C = x.shape
        xd = _rows(x, 'channel_layer_norm')
        w = weight.detach().float().reshape(C).contiguous()
        b = bias.detach().float().reshape(C).contiguous()
        y = torch.empty_like(xd)
        _lib.check(_lib.lib().dcf_op_layernorm(_lib.ptr(xd), _lib.ptr(w), _lib.ptr(b), _lib.ptr(y), B * T, C, int(relu), _lib.current_stream()),
                   'dcf_op_layernorm')
        ctx.save_for_backward(xd, w, b)
        ctx.relu, ctx.shapes = bool(relu), (weight.shape, bias.shape)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w, b = ctx.saved_tensors
        B, T, C = x.shape
        gy = gy.float().contiguous()
        gx = torch.empty_like(x)
        gw = torch.empty_like(w) if ctx.needs_input_grad[1] else None
        gb = torch.empty_like(b) if ctx.needs_input_grad[2] else None
        _lib.check(_lib.lib().dcf_op_layernorm_bwd(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(gy), _lib.ptr(gx), _lib.ptr(gw), _lib.ptr(gb),
                                                   B * T, C, int(ctx.relu), 0, _lib.current_stream()), 'dcf_op_layernorm_bwd')
        return (gx if ctx.needs_input_grad[0] else None, gw.reshape(ctx.shapes[0]) if gw is not None else None,
                gb.reshape(ctx.shapes[1]) if gb is not None else None, None)


def masked_conv1d(x, mask, weight, bias=None):
    """MaskedConv1D.forward (blocks.py:87-106; stride 1, groups 1, k = 1 or 3, padding (k - 1) / 2) on token-major ``x`` (B, T, Cin):
    ``conv(x * mask) + bias`` -> (B, T, N).  ``mask``: (B, T) or (B, 1, T) bool, None = all valid; ``weight``: (N, Cin, k)."""
    return _MaskedConv1dFn.apply(x, mask, weight, bias)


def channel_layer_norm(x, weight, bias, relu=False):
    """LayerNorm.forward (blocks.py:125-131) over the channels of token-major ``x`` (B, T, C), optionally followed by ReLU;
    ``weight`` / ``bias``: C elements of any shape (the reference keeps (C, 1))."""
    return _ChannelLayerNormFn.apply(x, weight, bias, relu)


def conv_head(x, mask, head, level=None):
    """ClsHead.forward / RegHead.forward (head.py:53-64 / :95-108) for ONE pyramid level on token-major ``x`` (B, T, E), with
    ``head`` a modeling.ConvHead: (B, T) logits, or -- for a head with ``scales`` -- (B, T, 2) offsets of level ``level``."""
    for conv, norm in zip(head.convs, head.norms):
        x = masked_conv1d(x, mask, conv.conv.weight, conv.conv.bias)
        x = channel_layer_norm(x, norm.weight, norm.bias, relu=True)
    if hasattr(head, 'scales'):
        if level is None:
            raise ValueError('conv_head: a regression head needs the pyramid level (its Scale)')
        out = head.reg_head.conv
        return torch.relu(head.scales[level].scale * masked_conv1d(x, mask, out.weight, out.bias))
    out = head.cls_head.conv
    return masked_conv1d(x, mask, out.weight, out.bias).squeeze(-1)
