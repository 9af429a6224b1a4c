"""Differentiable MaskedConv1D, channel LayerNorm and sliding-window attention on the MI355X, and blocks composed of them.

``masked_conv1d``, ``channel_layer_norm`` and ``window_attention`` are ``torch.autograd.Function``s over the library's
single-operator entry points: the forwards are the kernels the network's forward runs (dcf_op_conv3_split / dcf_op_linear_split /
dcf_op_layernorm / dcf_op_local_attn), the backwards are dcf_op_conv_bwd_data / dcf_op_conv_bwd_weight / dcf_op_layernorm_bwd
(csrc/conv_grad.hip) and dcf_op_local_attn_bwd (csrc/attn_grad.hip), all on the current stream and without a host wait.  Tensors
are token-major ``(B, T, C)`` fp32 on the GPU; there is no CPU path.

``conv_head`` runs one pyramid level through a ClsHead / RegHead (libs/modeling/head.py:53-64, :95-108) and ``masked_mha`` runs the
local-window MaskedMHA of an encoder block (blocks.py:348-373, :391-392), so a head -- and the attention in front of it -- trains end
to end with ``loss.PointObjective``.  Both demonstrate the operators, they are not the training forward: ``forward(..., eval=False)``
still returns plain tensors.  Of a TransformerEncoder block the depthwise q / k / v convolutions, the stride-2 pooling skip and the
attention-map dropout have no backward yet, and neither has the cross attention of the fusion blocks.
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


class _WindowAttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, mask, n_heads, window):
        qd, kd, vd = (_rows(z, 'window_attention') for z in (q, k, v))
        B, T, C = qd.shape
        if kd.shape != qd.shape or vd.shape != qd.shape:
            raise ValueError(f'window_attention: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)} must agree (self attention)')
        if window <= 0 or window % 2 == 0:
            raise ValueError(f'window_attention: window = {window} must be odd and positive (global attention has no backward)')
        m = _mask_rows(mask, B, T)
        if m is None:
            m = torch.ones(B, T, dtype=torch.bool, device=qd.device)       # the forward core reads its mask unconditionally
        o = torch.empty_like(qd)
        _lib.check(_lib.lib().dcf_op_local_attn(_lib.ptr(qd), _lib.ptr(kd), _lib.ptr(vd), _lib.ptr(m), _lib.ptr(o), B, T, C, int(n_heads), int(window),
                                                _lib.current_stream()), 'dcf_op_local_attn')
        ctx.save_for_backward(qd, kd, vd, m)
        ctx.n_heads, ctx.window = int(n_heads), int(window)
        return o

    @staticmethod
    def backward(ctx, go):
        q, k, v, m = ctx.saved_tensors
        B, T, C = q.shape
        go = go.float().contiguous()
        gq, gk, gv = (torch.empty_like(q) if need else None for need in ctx.needs_input_grad[:3])
        if gq is not None or gk is not None or gv is not None:
            _lib.check(_lib.lib().dcf_op_local_attn_bwd(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(m), _lib.ptr(go), _lib.ptr(gq), _lib.ptr(gk),
                                                        _lib.ptr(gv), B, T, C, ctx.n_heads, ctx.window, _lib.current_stream()),
                       'dcf_op_local_attn_bwd')
        return gq, gk, gv, None, None, None


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


def window_attention(q, k, v, mask, n_heads, window):
    """The sliding-window attention core of MaskedMHA (blocks.py:204-325, :357-373) on token-major ``q`` / ``k`` / ``v`` (B, T, C), heads
    concatenated along C: softmax over the keys |j - t| <= window // 2 of the sequence, d^-1/4 on q and on k, -1e4 on padded keys,
    zero rows at padded queries -> (B, T, C).  ``mask``: (B, T) or (B, 1, T) bool, None = all valid; ``window`` odd and positive."""
    return _WindowAttentionFn.apply(q, k, v, mask, n_heads, window)


def masked_mha(q_in, k_in, v_in, mask, mha):
    """MaskedMHA.forward (blocks.py:327-373, :391-393; local branch, no dropout) on token-major inputs (B, T, C), with ``mha`` a
    modeling.MaskedMHA of ``window_size > 0``: proj(window_attention(query(q_in), key(k_in), value(v_in))).  The four projections are
    k = 1 convolutions that do not mask their input (the reference's are plain nn.Conv1d)."""
    if mha.window_size <= 0:
        raise ValueError('masked_mha: a MaskedMHA with window_size > 0 is required (global attention has no backward)')
    q = masked_conv1d(q_in, None, mha.query.weight, mha.query.bias)
    k = masked_conv1d(k_in, None, mha.key.weight, mha.key.bias)
    v = masked_conv1d(v_in, None, mha.value.weight, mha.value.bias)
    ctx = window_attention(q, k, v, mask, mha.n_heads, mha.window_size)
    return masked_conv1d(ctx, None, mha.proj.weight, mha.proj.bias)
