"""Differentiable operators of the video encoder, of the fusion decoder and of the refinement stage on the MI355X, and blocks composed
of them, up to a whole TransformerEncoder block, a whole XAttNFusion stack and ``fuse_and_predict`` of PtTransformerEarlyFusionIterative.

``masked_conv1d``, ``channel_layer_norm``, ``window_attention``, ``cross_attention``, ``depthwise_conv1d``, ``masked_max_pool1d``,
``gelu``, ``layer_scale_residual`` and ``adaln_modulate`` are ``torch.autograd.Function``s over the library's single-operator entry
points.  The forwards of the first four are the kernels the network's forward runs (dcf_op_conv3_split / dcf_op_linear_split /
dcf_op_layernorm / dcf_op_local_attn / dcf_op_xattn), their backwards are dcf_op_conv_bwd_data / dcf_op_conv_bwd_weight /
dcf_op_layernorm_bwd (csrc/conv_grad.hip), dcf_op_local_attn_bwd (csrc/attn_grad.hip) and dcf_op_xattn_bwd (csrc/xattn_grad.hip); the
other five are the forward / backward pairs of csrc/enc_grad.hip (dcf_op_dwconv3, dcf_op_masked_maxpool, dcf_op_gelu,
dcf_op_layerscale_residual and their ``_bwd``) and of csrc/xattn_grad.hip (dcf_op_adaln, dcf_op_adaln_bwd).  Everything runs on the
current stream and without a host wait.  Tensors are token-major ``(B, T, C)`` fp32 on the GPU; there is no CPU path.

``global_attention`` is the global self-attention core (``mha_win_size = 0``): the forward is dcf_op_local_attn with window = 0, the
backward dcf_op_global_attn_bwd (csrc/global_attn_grad.hip, include/decafnet_hip_attn.h).

``conv_head`` runs one pyramid level through a ClsHead / RegHead (libs/modeling/head.py:53-64, :95-108), ``masked_mha`` the
self-attention MaskedMHA, local window or global (blocks.py:348-393), ``ffn`` the FFN (blocks.py:535-538), ``conv_attn_layer`` a
ConvAttNLayer (blocks.py:462-473) and ``transformer_encoder`` a whole TransformerEncoder block (blocks.py:578-591): a block of the
video encoder (stride 1 or 2, local window or global) or of the text encoder (stride 0, global self-attention through ``xattn_mha``
with q = k = v; more than 64 positions need heads of 32 or 64 channels); ``xattn_mha`` is MaskedMHA in its global cross-attention
branch (blocks.py:327-356, :374-393), ``conv_xattn_layer`` a ConvXAttNLayer (blocks.py:513-520), ``transformer_decoder`` a whole TransformerDecoder layer (blocks.py:632-650, 'adaln' or 'affine')
and ``xattn_fusion`` the XAttNFusion stack (fusion.py:56-66).  So the stem, every pyramid level, the text-conditioned fusion and the
heads behind them train end to end with ``loss.PointObjective``.

``masked_conv1d(..., stride=2)`` / ``strided_masked_conv1d`` is the k = 5 / stride-2 embedding convolution of ``vid_net.stride > 1``
(video_net.py:62-70): the forward's own path (dcf_op_conv5s2_split) and dcf_op_conv5s2_bwd_data / dcf_op_conv5s2_bwd_weight
(csrc/conv_grad.hip).  ``video_transformer`` is VideoTransformer.forward (video_net.py:123-164: embd_fc, the embedding convolutions,
the position encoding, the stem and the branch, ``pool_only`` included) and ``text_transformer`` TextTransformer.forward
(text_net.py:158-188: embd_fc, the position encoding, the background token, the stride-0 blocks), both in their training branch.  With
them every trainable parameter of the default model lies in a module that has a differentiable function here.

Dropout and drop-path.  ``layer_scale_residual``, ``ffn``, ``transformer_encoder`` (stride 1 / 2), ``transformer_decoder``,
``xattn_fusion`` and ``video_transformer`` take ``drop``, a ``DropSpec``: the 64-bit key, the first sample's index ``b0`` in the
reference's batch, ``proj_pdrop`` and ``path_pdrop``, and the site group / layer of the block (``DropSpec.at``; a stack numbers its
layers itself).  The keep bits are those of the training forward (``model.enable_dropout``; csrc/dropout.h: Philox4x32-10 on
(key, site, element)), so nothing is saved for the backward: it recomputes them (csrc/drop_grad.hip, include/decafnet_hip_train.h --
``dropout``, ``gelu_dropout`` and the residual with both of its dropouts, dcf_op_dropout / dcf_op_gelu_dropout / dcf_op_drop_residual
and their ``_bwd``).  ``drop=None``, or a spec whose probabilities are 0, is the code path without dropout: the same operators, the
same bits.  ``DropSpec.attn_p`` is the rate of the dropout on the attention map (blocks.py:368): ``window_attention``, ``masked_mha``,
``conv_attn_layer`` and ``transformer_encoder`` hand it to kernels that draw the keep bits where the map element is formed, forward and
backward (csrc/attn_drop.hip, include/decafnet_hip_attn_drop.h: dcf_op_local_attn_drop and its ``_bwd``); ``channel_dropout`` is
nn.Dropout1d on the clip features (dcf_op_channel_dropout).  ``global_attention`` and ``cross_attention`` take the same ``drop``
(dcf_op_local_attn_drop with window = 0, dcf_op_global_attn_drop_bwd, dcf_op_xattn_drop and its ``_bwd``), stride-0 blocks take
``drop`` under group DROP_G_TEXT (``text_transformer``), and ``fuse_and_predict`` takes ``fusion_drop`` for the second fusion
(DROP_G_FUSION2).  ``forward(..., eval=False)`` still returns plain tensors: the training forward with a graph is
``train.training_forward``.

``refine_in`` and ``tcn_layer`` are the forward / backward pairs of csrc/refine_grad.hip (dcf_op_refine_in, dcf_op_tcn_layer and their
``_bwd``): the stacking of the nearest-upsampled first-pass logits fused with refine.conv_1x1 (model.py:449-455) and one
DilatedResidualLayer (tcn.py:21-38).  ``tcn`` is the whole refinement TCN (tcn.py:66-84) and ``fuse_and_predict`` is model.py:442-471:
the three outputs ``loss.PointObjective`` consumes, with a graph.  The refinement is the one place where the reference hard-wires a
dropout in training (tcn.py:5,13: 0.5), so these three take ``dropout = (seed, p, b0)``: the keep bits are those of the training
forward (``model.enable_dropout``; csrc/dropout.h), recomputed in the backward.

``vid_map`` is ``masked_conv1d`` (k = 1) on the gated, concatenated input under the mask after the gate, and composed that way --
gate, ``vid_map``, ``text_transformer``, the first ``xattn_fusion``, ``video_transformer``, ``fuse_and_predict``,
``loss.PointObjective`` -- the whole training step reproduces the reference's ``backward()`` on every parameter
(tests/step_grad_ref.py ``run_step``, tests/test_gpu_step_grad.py).  ``gated_vid_map`` is the same stage without that input tensor:
dcf_op_vidmap_shared / dcf_op_vidmap_shared_bwd (csrc/front_grad.hip, include/decafnet_hip_front.h) compute ``W[:, :D] . vid`` and
``W[:, D:2D] . shallow`` once per video, skip the 64-clip tiles that no query's gate keeps, combine them per query row, and form the
weight gradient from per-video row sums of the upstream gradient against the channel-major features; the raw-score channel of
``opt.model.scat`` is a rank-1 term.  It saves only its inputs and meets the same rule against the same reference
(tests/test_gpu_front_grad.py); ``train.training_forward(front_end='shared')`` composes the step with it.  ``selected_vid_map`` is its
counterpart on the expert features of the selected clips alone: packed (n_rows, D) rows with ``row_first`` and ``pos`` as
``model.select_clips_videos`` returns them (dcf_op_vidmap_selected / dcf_op_vidmap_selected_bwd, csrc/front_select.hip,
include/decafnet_hip_front_select.h); its backward saves the rows as stored and no dense expert tensor
(tests/test_gpu_front_select.py); ``train.training_forward(expert='selected')`` composes the step with it.

Without a backward yet: the gate (it has no parameters: its inputs are features the caller supplies, so it does not stand between these
functions and a training step), TextIdentity's attention pool (``text_transformer`` refuses a TextIdentity), cross-attention over more
than 64 keys, and global self-attention on head dimensions other than 32 / 64 (over more than 64 positions in the text encoder).
"""
from collections import namedtuple

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


def _byte_mask(mask, B, T, name):
    """(B, T) bool on the GPU or None, from (B, T) / (B, 1, T) of any integer type"""
    m = _mask_rows(mask, B, T)
    if m is not None and not m.is_cuda:
        raise RuntimeError(f'{name}: the mask must be on the GPU (there is no CPU path)')
    return m


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
        if ctx.needs_input_grad[2] or want_b:
            # a bias whose weight is frozen still takes its sum from the weight kernel (db rides along with dW there): the same bits
            # whether or not the weight asks for a gradient
            gw = torch.empty_like(w)
            gb = torch.empty(N, dtype=torch.float32, device=x.device) if want_b else None
            _lib.check(L.dcf_op_conv_bwd_weight(_lib.ptr(x), _lib.ptr(m), _lib.ptr(gy), _lib.ptr(gw), _lib.ptr(gb), B, T, Cin, N, k, 0, st),
                       'dcf_op_conv_bwd_weight')
            if not ctx.needs_input_grad[2]:
                gw = None
        return gx, None, gw, gb


class _MaskedConv5s2Fn(torch.autograd.Function):
    """the k = 5 / stride 2 / padding 2 MaskedConv1D without bias (video_net.py:62-70)"""

    @staticmethod
    def forward(ctx, x, mask, weight):
        B, T, Cin = x.shape
        N, Cw, k = weight.shape
        if Cw != Cin or k != 5:
            raise ValueError(f'masked_conv1d: stride = 2 admits exactly k = 5 (padding 2, groups = 1): weight {tuple(weight.shape)} on {Cin} channels')
        if T % 2:
            raise ValueError(f'masked_conv1d: T = {T} must be a multiple of the stride 2')
        xd, wd = _rows(x, 'masked_conv1d'), weight.detach().float().contiguous()
        m = _mask_rows(mask, B, T)
        y = torch.empty(B, T // 2, N, dtype=torch.float32, device=xd.device)
        _lib.check(_lib.lib().dcf_op_conv5s2_split(_lib.ptr(xd), _lib.ptr(m), _lib.ptr(wd), _lib.ptr(y), B, T, Cin, N, _F16X3, _lib.current_stream()),
                   'dcf_op_conv5s2_split')
        ctx.save_for_backward(xd, m, wd)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, m, w = ctx.saved_tensors
        B, T, Cin = x.shape
        N = w.size(0)
        gy = gy.float().contiguous()
        L, st = _lib.lib(), _lib.current_stream()
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x)
            _lib.check(L.dcf_op_conv5s2_bwd_data(_lib.ptr(gy), _lib.ptr(m), _lib.ptr(w), _lib.ptr(gx), B, T, Cin, N, st), 'dcf_op_conv5s2_bwd_data')
        if ctx.needs_input_grad[2]:
            gw = torch.empty_like(w)
            _lib.check(L.dcf_op_conv5s2_bwd_weight(_lib.ptr(x), _lib.ptr(m), _lib.ptr(gy), _lib.ptr(gw), B, T, Cin, N, 0, st),
                       'dcf_op_conv5s2_bwd_weight')
        return gx, None, gw


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


def _attn_operands(name, q, k, v, mask, cross=False):
    """What every attention core starts from: q (B, T, C) and k / v (B, Lk, C) as fp32 rows whose shapes agree (self attention:
    Lk = T), the key mask as (B, Lk) bool on the GPU -- ones for None: the forward cores read their mask unconditionally -- and an
    empty output."""
    qd, kd, vd = (_rows(z, name) for z in (q, k, v))
    B, T, C = qd.shape
    if cross:
        if kd.shape != (B, kd.size(1), C) or vd.shape != kd.shape:
            raise ValueError(f'{name}: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)} do not agree ((B, T, C) and (B, Lk, C))')
    elif kd.shape != qd.shape or vd.shape != qd.shape:
        raise ValueError(f'{name}: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)} must agree (self attention)')
    m = _byte_mask(mask, B, kd.size(1), name)
    if m is None:
        m = torch.ones(B, kd.size(1), dtype=torch.bool, device=qd.device)
    return qd, kd, vd, m, torch.empty_like(qd)


def _map_drop(drop):
    """the ``drop`` argument of an attention Function -- None, or (key, site, p, b0) of the dropout on its map -- as the exports take it"""
    if drop is None:
        return None
    key, site, p, b0 = drop
    return int(b0), int(key), int(site), float(p)


def _attn_launch(plain, dropped, tensors, geom, drop):
    """the export ``plain``; with dropout on the map ``dropped``, which takes the same arguments and then ``drop``"""
    name, tail = (plain, ()) if drop is None else (dropped, drop)
    _lib.check(getattr(_lib.lib(), name)(*(_lib.ptr(t) for t in tensors), *geom, *tail, _lib.current_stream()), name)


def _attn_backward(ctx, go, plain, dropped, geom):
    """dQ, dK, dV of an attention Function that saved (q, k, v, mask) and ``ctx.drop``.  With dropout nothing else was saved: the
    backward draws the keep bits again from (key, site, b0)."""
    q, k, v, m = ctx.saved_tensors
    go = go.float().contiguous()
    gq, gk, gv = (torch.empty_like(z) if need else None for z, need in zip((q, k, v), ctx.needs_input_grad[:3]))
    if gq is not None or gk is not None or gv is not None:
        _attn_launch(plain, dropped, (q, k, v, m, go, gq, gk, gv), geom, ctx.drop)
    return gq, gk, gv


class _WindowAttentionFn(torch.autograd.Function):
    """``drop``: None, or (key, site, p, b0) of the dropout on the map (dcf_op_local_attn_drop / dcf_op_local_attn_drop_bwd)"""

    @staticmethod
    def forward(ctx, q, k, v, mask, n_heads, window, drop):
        if window <= 0 or window % 2 == 0:
            raise ValueError(f'window_attention: window = {window} must be odd and positive (global attention is global_attention)')
        qd, kd, vd, m, o = _attn_operands('window_attention', q, k, v, mask)
        ctx.geom, ctx.drop = (*qd.shape, int(n_heads), int(window)), _map_drop(drop)
        _attn_launch('dcf_op_local_attn', 'dcf_op_local_attn_drop', (qd, kd, vd, m, o), ctx.geom, ctx.drop)
        ctx.save_for_backward(qd, kd, vd, m)
        return o

    @staticmethod
    def backward(ctx, go):
        return _attn_backward(ctx, go, 'dcf_op_local_attn_bwd', 'dcf_op_local_attn_drop_bwd', ctx.geom) + (None,) * 4


_GLOBAL_HEAD_DIMS = (32, 64)     # the head dimensions of k_global_attn and of its backward


def _global_head_limit(C, n_heads):
    """the message of the head-dimension limit of ``global_attention`` that (C channels on n_heads heads) breaks, or None"""
    if n_heads <= 0 or C % n_heads or C // n_heads not in _GLOBAL_HEAD_DIMS:
        return f'global attention: C = {C} on {n_heads} heads: the head dimension must be 32 or 64'
    return None


class _GlobalAttentionFn(torch.autograd.Function):
    """``drop``: None, or (key, site, p, b0) of the dropout on the map (dcf_op_local_attn_drop with window = 0 /
    dcf_op_global_attn_drop_bwd)"""

    @staticmethod
    def forward(ctx, q, k, v, mask, n_heads, drop):
        limit = _global_head_limit(q.size(-1), int(n_heads))
        if limit:
            raise ValueError(f'global_attention: {limit}')
        if q.size(-1) > 1024:
            raise ValueError(f'global_attention: C = {q.size(-1)} (at most 1024)')
        qd, kd, vd, m, o = _attn_operands('global_attention', q, k, v, mask)
        ctx.geom, ctx.drop = (*qd.shape, int(n_heads)), _map_drop(drop)
        _attn_launch('dcf_op_local_attn', 'dcf_op_local_attn_drop', (qd, kd, vd, m, o), ctx.geom + (0,), ctx.drop)
        ctx.save_for_backward(qd, kd, vd, m)
        return o

    @staticmethod
    def backward(ctx, go):
        return _attn_backward(ctx, go, 'dcf_op_global_attn_bwd', 'dcf_op_global_attn_drop_bwd', ctx.geom) + (None,) * 3


def masked_conv1d(x, mask, weight, bias=None, stride=1):
    """MaskedConv1D.forward (blocks.py:87-106; stride 1, groups 1, k = 1 or 3, padding (k - 1) / 2) on token-major ``x`` (B, T, Cin):
    ``conv(x * mask) + bias`` -> (B, T, N).  ``mask``: (B, T) or (B, 1, T) bool, None = all valid; ``weight``: (N, Cin, k).
    ``stride=2`` admits exactly k = 5 (padding 2) without bias, T even -> (B, T / 2, N); the mask that goes with the result is
    ``mask[:, ::2]`` (``strided_masked_conv1d`` returns it)."""
    if stride == 1:
        return _MaskedConv1dFn.apply(x, mask, weight, bias)
    if stride != 2:
        raise ValueError(f'masked_conv1d: stride = {stride} (1, or 2 with k = 5)')
    if bias is not None:
        raise ValueError('masked_conv1d: stride = 2 is the k = 5 embedding convolution, which has no bias')
    return _MaskedConv5s2Fn.apply(x, mask, weight)


class _GatedVidMapFn(torch.autograd.Function):
    """dcf_op_vidmap_shared / dcf_op_vidmap_shared_bwd (csrc/front_grad.hip), or their ``_h`` forms on float16 features
    (include/decafnet_hip_front_half.h).  Saves its inputs -- the features as they are stored -- and nothing else."""

    @staticmethod
    def forward(ctx, vid, shallow, gate, mask, correl, sizes, weight, bias, skip):
        nvid, D, T = vid.shape
        E = weight.size(0)
        nq = sum(sizes)
        flags = 0 if skip else _lib.FRONT_NO_SKIP
        y = torch.empty(nq, T, E, dtype=torch.float32, device=vid.device)
        host_nq = torch.tensor(sizes, dtype=torch.int32)
        w, b = weight.detach().float().reshape(E, -1).contiguous(), bias.detach().float().contiguous()
        name = 'dcf_op_vidmap_shared_h' if vid.dtype == torch.float16 else 'dcf_op_vidmap_shared'
        _lib.check(getattr(_lib.lib(), name)(_lib.ptr(vid), _lib.ptr(shallow), _lib.ptr(w), _lib.ptr(b), _lib.ptr(gate), _lib.ptr(mask),
                                             _lib.ptr(correl), _lib.ptr(host_nq), _lib.ptr(y), nvid, D, T, E, flags, _lib.current_stream()), name)
        ctx.save_for_backward(vid, gate, mask, *(z for z in (shallow, correl) if z is not None))
        ctx.msf, ctx.scat, ctx.sizes, ctx.flags, ctx.wshape = shallow is not None, correl is not None, sizes, flags, tuple(weight.shape)
        return y

    @staticmethod
    def backward(ctx, gy):
        vid, gate, mask, *rest = ctx.saved_tensors
        shallow = rest.pop(0) if ctx.msf else None
        correl = rest.pop(0) if ctx.scat else None
        nvid, D, T = vid.shape
        E = ctx.wshape[0]
        want_w, want_b = ctx.needs_input_grad[6], ctx.needs_input_grad[7]
        if not (want_w or want_b):
            return (None,) * 9
        # a bias whose weight is frozen still takes its sum from the same call: the same bits whether or not the weight asks
        gy = gy.float().contiguous()
        gw = torch.empty(ctx.wshape, dtype=torch.float32, device=vid.device)
        gb = torch.empty(E, dtype=torch.float32, device=vid.device) if want_b else None
        host_nq = torch.tensor(ctx.sizes, dtype=torch.int32)
        name = 'dcf_op_vidmap_shared_bwd_h' if vid.dtype == torch.float16 else 'dcf_op_vidmap_shared_bwd'
        _lib.check(getattr(_lib.lib(), name)(_lib.ptr(vid), _lib.ptr(shallow), _lib.ptr(gate), _lib.ptr(mask), _lib.ptr(correl),
                                             _lib.ptr(host_nq), _lib.ptr(gy), _lib.ptr(gw), _lib.ptr(gb), nvid, D, T, E, ctx.flags, 0,
                                             _lib.current_stream()), name)
        return None, None, None, None, None, None, (gw if want_w else None), gb, None


def gated_vid_map(vid, shallow, gate, mask, correl, text_size, weight, bias, skip=True):
    """``vid_map`` of the training forward (model.py:567-583) on shared products: ``MaskedConv1D`` (k = 1) on the gated,
    concatenated input without building it.  ``vid`` / ``shallow`` (nvid, D, T) channel-major as the batch holds them (``shallow``
    None: no msf), ``gate`` (B', T) fp32 0 / 1 and ``mask`` (B', T) bool as dcf_op_gate returns them, ``correl`` (B', T) the raw
    sidekick scores of dcf_op_sidekick (None: no scat), ``text_size`` the queries per video (B' = their sum, rows in (video, query)
    order; None: one each), ``weight`` (E, Cin, 1) with Cin = D [+ D] [+ 1], ``bias`` (E,) -> (B', T, E).
    ``W[:, :D] . vid`` and ``W[:, D:2D] . shallow`` are computed once per video, 64-clip tiles that no query of the video keeps not
    at all (``skip=False`` computes them: a test switch, the same bits); the backward gives the weight and the bias their gradients
    (include/decafnet_hip_front.h) and saves only its inputs.  The features, the gate and the scores are data: a feature tensor
    that requires a gradient is refused.
    ``vid`` / ``shallow`` may be ``torch.float16``, both or neither (one of the two is a ValueError): a float16 pair goes to
    dcf_op_vidmap_shared_h / dcf_op_vidmap_shared_bwd_h (include/decafnet_hip_front_half.h) as it is stored -- no fp32 copy is made or
    saved -- and the result and the gradients are those of the same values passed as fp32, bit for bit."""
    for name, z in (('vid', vid), ('shallow', shallow), ('gate', gate), ('correl', correl)):
        if z is not None and z.requires_grad:
            raise ValueError(f'gated_vid_map: `{name}` requires a gradient; the features, the gate and the scores are data (no gradient reaches them)')
    if torch.is_tensor(vid) and torch.is_tensor(shallow):
        from .modeling import _check_feature_dtypes
        _check_feature_dtypes(vid, shallow)
    if not (torch.is_tensor(vid) and vid.is_cuda and vid.dim() == 3):
        raise RuntimeError('gated_vid_map: (nvid, D, T) features on the GPU are required (there is no CPU path)')
    nvid, D, T = vid.shape
    sizes = tuple([1] * nvid if text_size is None else [int(k) for k in text_size])
    nq = sum(sizes)
    cin = D * (2 if shallow is not None else 1) + (1 if correl is not None else 0)
    if len(sizes) != nvid or min(sizes) < 1:
        raise ValueError(f'gated_vid_map: text_size {list(sizes)} does not match {nvid} videos (one entry >= 1 per video)')
    if weight.dim() != 3 or weight.size(1) != cin or weight.size(2) != 1 or bias is None or tuple(bias.shape) != (weight.size(0),):
        raise ValueError(f'gated_vid_map: weight {tuple(weight.shape)} / bias on {cin} input channels (k = 1, with bias)')
    if shallow is not None and tuple(shallow.shape) != (nvid, D, T):
        raise ValueError(f'gated_vid_map: shallow {tuple(shallow.shape)} against vid {(nvid, D, T)}')
    for name, z in (('gate', gate), ('mask', mask), ('correl', correl)):
        if z is not None and tuple(z.shape) != (nq, T):
            raise ValueError(f'gated_vid_map: {name} {tuple(z.shape)} is not ({nq}, {T})')
    f = lambda z: None if z is None else z.detach().float().contiguous()
    m = mask.detach()
    m = (m if m.dtype == torch.bool else m != 0).contiguous()
    x = (lambda z: None if z is None else z.detach().contiguous()) if vid.dtype == torch.float16 else f      # float16: as stored
    return _GatedVidMapFn.apply(x(vid), x(shallow), f(gate), m, f(correl), sizes, weight, bias, bool(skip))


class _SelectedVidMapFn(torch.autograd.Function):
    """dcf_op_vidmap_selected / dcf_op_vidmap_selected_bwd (csrc/front_select.hip), or their ``_h`` forms on float16 features
    (include/decafnet_hip_front_select.h).  Saves its inputs -- the packed rows as they are stored -- and no dense expert tensor."""

    @staticmethod
    def forward(ctx, rows, row_first, pos, shallow, gate, mask, correl, sizes, weight, bias):
        nvid, T = pos.shape
        D, E = rows.size(1), weight.size(0)
        y = torch.empty(sum(sizes), T, E, dtype=torch.float32, device=rows.device)
        host_first, host_nq = torch.tensor(row_first, dtype=torch.int32), torch.tensor(sizes, dtype=torch.int32)
        w, b = weight.detach().float().reshape(E, -1).contiguous(), bias.detach().float().contiguous()
        name = 'dcf_op_vidmap_selected_h' if rows.dtype == torch.float16 else 'dcf_op_vidmap_selected'
        _lib.check(getattr(_lib.lib(), name)(_lib.ptr(rows), _lib.ptr(host_first), _lib.ptr(pos), _lib.ptr(shallow), _lib.ptr(w), _lib.ptr(b),
                                             _lib.ptr(gate), _lib.ptr(mask), _lib.ptr(correl), _lib.ptr(host_nq), _lib.ptr(y), nvid, D, T, E,
                                             _lib.current_stream()), name)
        ctx.save_for_backward(rows, pos, gate, mask, *(z for z in (shallow, correl) if z is not None))
        ctx.msf, ctx.scat, ctx.sizes, ctx.row_first, ctx.wshape = shallow is not None, correl is not None, sizes, row_first, tuple(weight.shape)
        return y

    @staticmethod
    def backward(ctx, gy):
        rows, pos, gate, mask, *rest = ctx.saved_tensors
        shallow = rest.pop(0) if ctx.msf else None
        correl = rest.pop(0) if ctx.scat else None
        nvid, T = pos.shape
        D, E = rows.size(1), ctx.wshape[0]
        want_w, want_b = ctx.needs_input_grad[8], ctx.needs_input_grad[9]
        if not (want_w or want_b):
            return (None,) * 10
        # a bias whose weight is frozen still takes its sum from the same call: the same bits whether or not the weight asks
        gy = gy.float().contiguous()
        gw = torch.empty(ctx.wshape, dtype=torch.float32, device=rows.device)
        gb = torch.empty(E, dtype=torch.float32, device=rows.device) if want_b else None
        host_first, host_nq = torch.tensor(ctx.row_first, dtype=torch.int32), torch.tensor(ctx.sizes, dtype=torch.int32)
        name = 'dcf_op_vidmap_selected_bwd_h' if rows.dtype == torch.float16 else 'dcf_op_vidmap_selected_bwd'
        _lib.check(getattr(_lib.lib(), name)(_lib.ptr(rows), _lib.ptr(host_first), _lib.ptr(pos), _lib.ptr(shallow), _lib.ptr(gate),
                                             _lib.ptr(mask), _lib.ptr(correl), _lib.ptr(host_nq), _lib.ptr(gy), _lib.ptr(gw), _lib.ptr(gb), nvid,
                                             D, T, E, 0, _lib.current_stream()), name)
        return None, None, None, None, None, None, None, None, (gw if want_w else None), gb


def selected_vid_map(rows, row_first, pos, shallow, gate, mask, correl, text_size, weight, bias):
    """``gated_vid_map`` on the expert features of the selected clips alone: ``rows`` (>= row_first[-1], D) clip-major and packed, video
    v's rows from ``row_first[v]`` on (more rows are allowed: a capacity buffer that is never read); ``row_first`` nvid + 1 ints on the
    host, strictly increasing from 0; ``pos`` (nvid, T) int32 video-local as ``model.select_clips_videos`` returns it (-1: the clip has
    no expert half, whatever its gate says: documented, not detected).  ``shallow`` (nvid, D, T) channel-major or None, ``gate`` /
    ``mask`` / ``correl`` (B', T), ``text_size``, ``weight`` (E, Cin, 1) and ``bias`` as ``gated_vid_map`` takes them -> (B', T, E).
    With ``pos`` a bijection between the clips some query of a video keeps and its rows, the result and the gradients of the weight
    and the bias are those of ``gated_vid_map`` on the dense features up to the summation order of the expert half
    (include/decafnet_hip_front_select.h).  The backward saves ``rows`` as stored, plus its other inputs: no dense expert tensor.
    ``rows`` / ``shallow`` may be ``torch.float16``, both or neither; at most 16 videos per call."""
    for name, z in (('rows', rows), ('shallow', shallow), ('gate', gate), ('correl', correl)):
        if z is not None and z.requires_grad:
            raise ValueError(f'selected_vid_map: `{name}` requires a gradient; the features, the gate and the scores are data (no gradient reaches them)')
    if torch.is_tensor(rows) and torch.is_tensor(shallow):
        from .modeling import _check_feature_dtypes
        _check_feature_dtypes(rows, shallow)
    if not (torch.is_tensor(rows) and rows.is_cuda and rows.dim() == 2):
        raise RuntimeError('selected_vid_map: (n_rows, D) expert rows on the GPU are required (there is no CPU path)')
    if not (torch.is_tensor(pos) and pos.dim() == 2 and pos.dtype == torch.int32 and pos.is_cuda):
        raise ValueError('selected_vid_map: pos is a (nvid, T) int32 tensor on the GPU')
    nvid, T = pos.shape
    D = rows.size(1)
    first = tuple(int(k) for k in row_first)
    sizes = tuple([1] * nvid if text_size is None else [int(k) for k in text_size])
    nq = sum(sizes)
    cin = D * (2 if shallow is not None else 1) + (1 if correl is not None else 0)
    if len(sizes) != nvid or min(sizes) < 1:
        raise ValueError(f'selected_vid_map: text_size {list(sizes)} does not match {nvid} videos (one entry >= 1 per video)')
    if len(first) != nvid + 1 or first[0] != 0 or any(not 0 < b - a <= T for a, b in zip(first, first[1:])) or rows.size(0) < first[-1]:
        raise ValueError(f'selected_vid_map: row_first {list(first)} for {nvid} videos and {rows.size(0)} rows (nvid + 1 entries, strictly '
                         f'increasing from 0, at most T = {T} rows per video, within rows)')
    if weight.dim() != 3 or weight.size(1) != cin or weight.size(2) != 1 or bias is None or tuple(bias.shape) != (weight.size(0),):
        raise ValueError(f'selected_vid_map: weight {tuple(weight.shape)} / bias on {cin} input channels (k = 1, with bias)')
    if shallow is not None and tuple(shallow.shape) != (nvid, D, T):
        raise ValueError(f'selected_vid_map: shallow {tuple(shallow.shape)} against {(nvid, D, T)}')
    for name, z in (('gate', gate), ('mask', mask), ('correl', correl)):
        if z is not None and tuple(z.shape) != (nq, T):
            raise ValueError(f'selected_vid_map: {name} {tuple(z.shape)} is not ({nq}, {T})')
    f = lambda z: None if z is None else z.detach().float().contiguous()
    m = mask.detach()
    m = (m if m.dtype == torch.bool else m != 0).contiguous()
    x = (lambda z: None if z is None else z.detach().contiguous()) if rows.dtype == torch.float16 else f      # float16: as stored
    return _SelectedVidMapFn.apply(x(rows), first, pos.detach().contiguous(), x(shallow), f(gate), m, f(correl), sizes, weight, bias)


def strided_masked_conv1d(x, mask, weight):
    """``masked_conv1d(x, mask, weight, stride=2)`` with the mask the reference hands on (blocks.py:101-105, nearest = every other
    position) -> ((B, T / 2, N), ``mask[:, ::2]``; None stays None)."""
    B, T, _ = x.shape
    y = masked_conv1d(x, mask, weight, None, 2)
    m = _mask_rows(mask, B, T)
    return y, (None if m is None else m[:, ::2].contiguous())


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


def window_attention(q, k, v, mask, n_heads, window, drop=None, sub=None):
    """The sliding-window attention core of MaskedMHA (blocks.py:204-325, :357-373) on token-major ``q`` / ``k`` / ``v`` (B, T, C), heads
    concatenated along C: softmax over the keys |j - t| <= window // 2 of the sequence, d^-1/4 on q and on k, -1e4 on padded keys,
    zero rows at padded queries -> (B, T, C).  ``mask``: (B, T) or (B, 1, T) bool, None = all valid; ``window`` odd and positive.
    ``drop`` with ``attn_p > 0``: nn.Dropout(attn_p) on the (B, H, T, window) softmax map (blocks.py:368) at site ``sub`` (DROP_ATTN) of
    the block ``drop`` names, drawn inside the kernels, forward and backward; with ``attn_p = 0`` the launches are those without it."""
    drop = _active(drop, 'window_attention')
    return _WindowAttentionFn.apply(q, k, v, mask, n_heads, window, _map_site(drop, sub))


def global_attention(q, k, v, mask, n_heads, drop=None, sub=None):
    """The global self-attention core of MaskedMHA (blocks.py:374-389 with q, k and v of one sequence) on token-major ``q`` / ``k`` / ``v``
    (B, T, C), heads concatenated along C: softmax over the valid keys of the sequence, d^-1/4 on q and on k, masked keys filled with
    -inf -> (B, T, C).  ``mask``: (B, T) or (B, 1, T), None = all valid.  It masks keys only: a padded query row has an output and takes
    a gradient like any other; a padded key takes none.  A sequence without a valid key gives zeros (the reference: NaN) and zero
    gradients.  Any T, head dimension 32 or 64, C <= 1024 (dcf_op_local_attn with window = 0, dcf_op_global_attn_bwd).  ``drop`` with
    ``attn_p > 0``: nn.Dropout(attn_p) on the (B, H, T, T) map (blocks.py:388) at site ``sub`` (DROP_ATTN), drawn inside the kernels."""
    drop = _active(drop, 'global_attention')
    return _GlobalAttentionFn.apply(q, k, v, mask, n_heads, _map_site(drop, sub))


def masked_mha(q_in, k_in, v_in, mask, mha, drop=None):
    """MaskedMHA.forward (blocks.py:327-393; self-attention, no proj_drop) on token-major inputs (B, T, C), with ``mha`` a
    modeling.MaskedMHA: proj(window_attention(query(q_in), key(k_in), value(v_in))) for ``window_size > 0``, and
    proj(global_attention(...)) for ``window_size = 0`` (head dimension 32 or 64).  The four projections are k = 1 convolutions that
    do not mask their input (the reference's are plain nn.Conv1d).  ``drop``: its ``attn_p`` is the rate of attn_drop (:368, :388) on the
    map of either core."""
    if mha.window_size < 0:
        raise ValueError(f'masked_mha: window_size = {mha.window_size} (odd and positive, or 0 for global attention)')
    if mha.window_size == 0:
        limit = _global_head_limit(mha.query.weight.size(0), mha.n_heads)
        if limit:
            raise ValueError(f'masked_mha: window_size = 0: {limit}')
    q = masked_conv1d(q_in, None, mha.query.weight, mha.query.bias)
    k = masked_conv1d(k_in, None, mha.key.weight, mha.key.bias)
    v = masked_conv1d(v_in, None, mha.value.weight, mha.value.bias)
    if mha.window_size == 0:
        ctx = global_attention(q, k, v, mask, mha.n_heads, **_drop_kw(drop))
    else:
        ctx = window_attention(q, k, v, mask, mha.n_heads, mha.window_size, **_drop_kw(drop))
    return masked_conv1d(ctx, None, mha.proj.weight, mha.proj.bias)


class _DepthwiseConv1dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mask, stride, *weights):
        B, T, C = x.shape
        n = len(weights)
        if stride not in (1, 2) or T % stride:
            raise ValueError(f'depthwise_conv1d: stride = {stride} must be 1 or 2 and divide T = {T}')
        if not 1 <= n <= 3 or any(tuple(w.shape) != (C, 1, 3) for w in weights):
            raise ValueError(f'depthwise_conv1d: one to three (C, 1, 3) weights on {C} channels are required (k = 3, groups = C), got '
                             f'{[tuple(w.shape) for w in weights]}')
        xd = _rows(x, 'depthwise_conv1d')
        m = _byte_mask(mask, B, T, 'depthwise_conv1d')
        w = torch.stack([z.detach().float().reshape(C, 3) for z in weights]).contiguous()
        y = torch.empty(n, B, T // stride, C, dtype=torch.float32, device=xd.device)
        _lib.check(_lib.lib().dcf_op_dwconv3(_lib.ptr(xd), _lib.ptr(m), _lib.ptr(w), _lib.ptr(y), B, T, C, n, stride, _lib.current_stream()),
                   'dcf_op_dwconv3')
        ctx.save_for_backward(xd, m, w)
        ctx.stride = stride
        return tuple(y.unbind(0))

    @staticmethod
    def backward(ctx, *gys):
        x, m, w = ctx.saved_tensors
        B, T, C = x.shape
        n = w.size(0)
        gy = torch.stack([g.float() for g in gys]).contiguous()
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gw = torch.empty_like(w) if any(ctx.needs_input_grad[3:]) else None
        if gx is not None or gw is not None:
            _lib.check(_lib.lib().dcf_op_dwconv3_bwd(_lib.ptr(x), _lib.ptr(m), _lib.ptr(w), _lib.ptr(gy), _lib.ptr(gx), _lib.ptr(gw), B, T, C, n,
                                                     ctx.stride, 0, _lib.current_stream()), 'dcf_op_dwconv3_bwd')
        gws = tuple(gw[i].reshape(C, 1, 3) if need else None for i, need in enumerate(ctx.needs_input_grad[3:]))
        return (gx, None, None) + gws


class _MaskedMaxPool1dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mask):
        B, T, C = x.shape
        if T % 2:
            raise ValueError(f'masked_max_pool1d: T = {T} must be a multiple of the stride 2')
        xd = _rows(x, 'masked_max_pool1d')
        m = _byte_mask(mask, B, T, 'masked_max_pool1d')
        y = torch.empty(B, T // 2, C, dtype=torch.float32, device=xd.device)
        mo = torch.empty(B, T // 2, dtype=torch.bool, device=xd.device)
        _lib.check(_lib.lib().dcf_op_masked_maxpool(_lib.ptr(xd), _lib.ptr(m), _lib.ptr(y), _lib.ptr(mo), B, T, C, _lib.current_stream()),
                   'dcf_op_masked_maxpool')
        ctx.save_for_backward(xd, m)
        ctx.mark_non_differentiable(mo)
        return y, mo

    @staticmethod
    def backward(ctx, gy, _):
        x, m = ctx.saved_tensors
        B, T, C = x.shape
        if not ctx.needs_input_grad[0]:
            return None, None
        gx = torch.empty_like(x)
        _lib.check(_lib.lib().dcf_op_masked_maxpool_bwd(_lib.ptr(x), _lib.ptr(m), _lib.ptr(gy.float().contiguous()), _lib.ptr(gx), B, T, C,
                                                        _lib.current_stream()), 'dcf_op_masked_maxpool_bwd')
        return gx, None


class _GeluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        if not (torch.is_tensor(x) and x.is_cuda):
            raise RuntimeError('gelu: a tensor on the GPU is required (there is no CPU path)')
        xd = x.detach().float().contiguous()
        y = torch.empty_like(xd)
        if xd.numel():
            _lib.check(_lib.lib().dcf_op_gelu(_lib.ptr(xd), _lib.ptr(y), xd.numel(), _lib.current_stream()), 'dcf_op_gelu')
        ctx.save_for_backward(xd)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, = ctx.saved_tensors
        gx = torch.empty_like(x)
        if x.numel():
            _lib.check(_lib.lib().dcf_op_gelu_bwd(_lib.ptr(x), _lib.ptr(gy.float().contiguous()), _lib.ptr(gx), x.numel(), _lib.current_stream()),
                       'dcf_op_gelu_bwd')
        return gx


class _LayerScaleResidualFn(torch.autograd.Function):
    """h None: y = r * r_mask (how transformer_encoder masks its input, blocks.py:581)"""

    @staticmethod
    def forward(ctx, r, h, scale, r_mask, h_mask):
        B, T, C = r.shape
        rd = _rows(r, 'layer_scale_residual')
        hd = ls = None
        if h is not None:
            hd = _rows(h, 'layer_scale_residual')
            if hd.shape != rd.shape or scale.numel() != C:
                raise ValueError(f'layer_scale_residual: r {tuple(r.shape)}, h {tuple(h.shape)}, scale {tuple(scale.shape)} do not agree')
            ls = scale.detach().float().reshape(C).contiguous()
        mr, mh = _byte_mask(r_mask, B, T, 'layer_scale_residual'), _byte_mask(h_mask, B, T, 'layer_scale_residual')
        y = torch.empty_like(rd)
        _lib.check(_lib.lib().dcf_op_layerscale_residual(_lib.ptr(rd), _lib.ptr(mr), _lib.ptr(hd), _lib.ptr(mh), _lib.ptr(ls), _lib.ptr(y), B * T, C,
                                                         _lib.current_stream()), 'dcf_op_layerscale_residual')
        ctx.save_for_backward(hd, ls, mr, mh)
        ctx.scale_shape = None if scale is None else scale.shape
        return y

    @staticmethod
    def backward(ctx, gy):
        h, ls, mr, mh = ctx.saved_tensors
        B, T, C = gy.shape
        gy = gy.float().contiguous()
        need_r, need_h, need_s = ctx.needs_input_grad[:3]
        need_h, need_s = need_h and h is not None, need_s and h is not None
        gr = torch.empty_like(gy) if need_r else None
        gh = torch.empty_like(gy) if need_h else None
        gs = torch.empty(C, dtype=torch.float32, device=gy.device) if need_s else None
        if need_r or need_h or need_s:
            _lib.check(_lib.lib().dcf_op_layerscale_residual_bwd(_lib.ptr(gy), _lib.ptr(h), _lib.ptr(mr), _lib.ptr(mh), _lib.ptr(ls), _lib.ptr(gr),
                                                                 _lib.ptr(gh), _lib.ptr(gs), B * T, C, 0, _lib.current_stream()),
                       'dcf_op_layerscale_residual_bwd')
        return gr, gh, gs.reshape(ctx.scale_shape) if gs is not None else None, None, None


# site groups and subs of csrc/dropout.h (site = group << 16 | layer << 4 | sub)
DROP_G_FUSION, DROP_G_STEM, DROP_G_BRANCH, DROP_G_REFINE = 1, 2, 3, 4
DROP_PROJ, DROP_FFN_HID, DROP_FFN_OUT, DROP_PATH_ATTN, DROP_PATH_FFN, DROP_TCN = 0, 1, 2, 3, 4, 5
# the sites of include/decafnet_hip_attn_drop.h: the attention map of a block, and channel dropout on the clip features
DROP_G_TEXT, DROP_G_FUSION2, DROP_G_INPUT = 5, 6, 7       # the text encoder's blocks; the fusion applied again per pyramid level; the clips
DROP_ATTN, DROP_CHANNEL = 6, 7


class DropSpec(namedtuple('DropSpec', 'seed b0 proj_p path_p group layer attn_p', defaults=(0, 0.0, 0.0, 0, 0, 0.0))):
    """Dropout of one block: the 64-bit key ``seed`` (``model.last_dropout_seed``), ``b0`` the index of the first sequence in the
    reference's batch, ``proj_p`` (proj_drop and the FFN's two dropouts) and ``path_p`` (drop-path), each in [0, 1), the block's
    site ``group`` (DROP_G_*) and ``layer``, and last ``attn_p``, the rate of the dropout on the attention map (sub DROP_ATTN), in
    [0, 1) too.  Immutable; ``at(group, layer)`` is the same spec at another block."""
    __slots__ = ()

    def __new__(cls, seed, b0=0, proj_p=0.0, path_p=0.0, group=0, layer=0, attn_p=0.0):
        proj_p, path_p, attn_p = float(proj_p), float(path_p), float(attn_p)
        for name, p in (('proj_p', proj_p), ('path_p', path_p), ('attn_p', attn_p)):
            if not 0.0 <= p < 1.0:
                raise ValueError(f'DropSpec: {name} = {p} must lie in [0, 1)')
        if int(b0) < 0 or not 0 <= int(group) < 1 << 15 or not 0 <= int(layer) < 1 << 12:
            raise ValueError(f'DropSpec: b0 = {b0}, group = {group}, layer = {layer} out of range')
        return super().__new__(cls, int(seed) & ((1 << 64) - 1), int(b0), proj_p, path_p, int(group), int(layer), attn_p)

    @property
    def active(self):
        return self.proj_p > 0.0 or self.path_p > 0.0 or self.attn_p > 0.0

    def at(self, group, layer):
        return self._replace(group=int(group), layer=int(layer))

    def site(self, sub):
        return self.group << 16 | self.layer << 4 | sub

    @property
    def key(self):
        """the key's 64 bits as the int64 the C ABI takes"""
        return self.seed - (1 << 64) if self.seed >= 1 << 63 else self.seed


def _drop_kw(drop):
    """the ``drop`` keyword of an inner call, passed on only where there is one: without dropout the calls are what they were"""
    return {} if drop is None else {'drop': drop}


def _map_site(drop, sub):
    """the ``drop`` argument of an attention Function: (key, site, p, b0) of the dropout on its map at site ``sub`` (DROP_ATTN) of the
    block ``drop`` names, or None where there is none (``attn_p = 0`` included: the launches are then those without it)"""
    if drop is None or drop.attn_p == 0.0:
        return None
    return drop.key, drop.site(DROP_ATTN if sub is None else sub), drop.attn_p, drop.b0


def _active(drop, name):
    """``drop`` if it drops anything, else None"""
    if drop is None:
        return None
    if not isinstance(drop, DropSpec):
        raise TypeError(f'{name}: drop must be an autograd.DropSpec or None, got {type(drop).__name__}')
    return drop if drop.active else None


class _DropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, key, site, p, b0):
        xd = _rows(x, 'dropout')
        B, T, C = xd.shape
        y = torch.empty_like(xd)
        ctx.geom = (B, T, C, b0, key, site, p)
        _lib.check(_lib.lib().dcf_op_dropout(_lib.ptr(xd), _lib.ptr(y), *ctx.geom, _lib.current_stream()), 'dcf_op_dropout')
        return y

    @staticmethod
    def backward(ctx, gy):
        gy = gy.float().contiguous()
        gx = torch.empty_like(gy)
        _lib.check(_lib.lib().dcf_op_dropout(_lib.ptr(gy), _lib.ptr(gx), *ctx.geom, _lib.current_stream()), 'dcf_op_dropout')
        return gx, None, None, None, None


class _GeluDropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, key, site, p, b0):
        xd = _rows(x, 'gelu_dropout')
        B, T, C = xd.shape
        y = torch.empty_like(xd)
        ctx.geom = (B, T, C, b0, key, site, p)
        _lib.check(_lib.lib().dcf_op_gelu_dropout(_lib.ptr(xd), _lib.ptr(y), *ctx.geom, _lib.current_stream()), 'dcf_op_gelu_dropout')
        ctx.save_for_backward(xd)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, = ctx.saved_tensors
        gx = torch.empty_like(x)
        _lib.check(_lib.lib().dcf_op_gelu_dropout_bwd(_lib.ptr(x), _lib.ptr(gy.float().contiguous()), _lib.ptr(gx), *ctx.geom, _lib.current_stream()),
                   'dcf_op_gelu_dropout_bwd')
        return gx, None, None, None, None


class _DropResidualFn(torch.autograd.Function):
    """_LayerScaleResidualFn with the dropout of ``h`` and the drop-path of the branch"""

    @staticmethod
    def forward(ctx, r, h, scale, r_mask, h_mask, key, b0, drop_site, drop_p, path_site, path_p):
        B, T, C = r.shape
        rd, hd = _rows(r, 'layer_scale_residual'), _rows(h, 'layer_scale_residual')
        if hd.shape != rd.shape or scale.numel() != C:
            raise ValueError(f'layer_scale_residual: r {tuple(r.shape)}, h {tuple(h.shape)}, scale {tuple(scale.shape)} do not agree')
        ls = scale.detach().float().reshape(C).contiguous()
        mr, mh = _byte_mask(r_mask, B, T, 'layer_scale_residual'), _byte_mask(h_mask, B, T, 'layer_scale_residual')
        if mr is not None and mh is not None:
            if r_mask is not h_mask:
                raise ValueError('layer_scale_residual: with dropout r_mask and h_mask, where both are given, are one tensor (a block has one mask)')
            mh = mr
        y = torch.empty_like(rd)
        ctx.geom = (B, T, C, b0, key, drop_site, drop_p, path_site, path_p)
        _lib.check(_lib.lib().dcf_op_drop_residual(_lib.ptr(rd), _lib.ptr(mr), _lib.ptr(hd), _lib.ptr(mh), _lib.ptr(ls), _lib.ptr(y), *ctx.geom,
                                                   _lib.current_stream()), 'dcf_op_drop_residual')
        ctx.save_for_backward(hd, ls, mr, mh)
        ctx.scale_shape = scale.shape
        return y

    @staticmethod
    def backward(ctx, gy):
        h, ls, mr, mh = ctx.saved_tensors
        C = gy.size(2)
        gy = gy.float().contiguous()
        need_r, need_h, need_s = ctx.needs_input_grad[:3]
        gr = torch.empty_like(gy) if need_r else None
        gh = torch.empty_like(gy) if need_h else None
        gs = torch.empty(C, dtype=torch.float32, device=gy.device) if need_s else None
        if need_r or need_h or need_s:
            _lib.check(_lib.lib().dcf_op_drop_residual_bwd(_lib.ptr(gy), _lib.ptr(h), _lib.ptr(mr), _lib.ptr(mh), _lib.ptr(ls), _lib.ptr(gr), _lib.ptr(gh),
                                                           _lib.ptr(gs), *ctx.geom, 0, _lib.current_stream()), 'dcf_op_drop_residual_bwd')
        return (gr, gh, gs.reshape(ctx.scale_shape) if gs is not None else None) + (None,) * 8


def depthwise_conv1d(x, mask, weights, stride=1):
    """One to three depthwise MaskedConv1D (blocks.py:87-106 with groups = C: k = 3, padding 1, no bias, stride 1 or 2) sharing the
    token-major input ``x`` (B, T, C): ``conv_i(x * mask)``, not masked afterwards -> (tuple of (B, T / stride, C), ``mask[:, ::stride]``).
    ``weights``: a sequence of PyTorch's (C, 1, 3) weights (q / k / v_conv of a ConvAttNLayer); ``mask``: (B, T) or (B, 1, T), None = all
    valid (then the returned mask is None)."""
    B, T, _ = x.shape
    ys = _DepthwiseConv1dFn.apply(x, mask, int(stride), *weights)
    m = _mask_rows(mask, B, T)
    return ys, (None if m is None else m[:, ::int(stride)].contiguous())


def masked_max_pool1d(x, mask):
    """masked_max_pool1d (blocks.py:31-47) with kernel 3, stride 2, padding 1 on token-major ``x`` (B, T, C), T even: padded slots take the
    (detached) minimum of their channel over the sequence, windows stay inside the sequence, the result is multiplied by the pooled mask
    -> ((B, T / 2, C), pooled mask (B, T / 2)).  The gradient goes to the lowest position that holds a window's maximum."""
    return _MaskedMaxPool1dFn.apply(x, mask)


def gelu(x):
    """nn.GELU() of FFN.actv (blocks.py:531): ``x * Phi(x)`` elementwise, any shape."""
    return _GeluFn.apply(x)


def dropout(x, drop, sub):
    """nn.Dropout(drop.proj_p) at site ``sub`` of the block ``drop`` names, on token-major ``x`` (B, T, C) of the reference's (B, C, T)
    tensor: kept values times 1 / (1 - p), dropped ones 0.  The backward is the same operator on the gradient."""
    drop = _active(drop, 'dropout')
    if drop is None or drop.proj_p == 0.0:
        return x
    return _DropoutFn.apply(x, drop.key, drop.site(sub), drop.proj_p, drop.b0)


class _ChannelDropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, key, site, p, b0):
        xd = _rows(x, 'channel_dropout')
        B, T, C = xd.shape
        y = torch.empty_like(xd)
        ctx.geom = (B, T, C, b0, key, site, p)
        _lib.check(_lib.lib().dcf_op_channel_dropout(_lib.ptr(xd), _lib.ptr(y), *ctx.geom, _lib.current_stream()), 'dcf_op_channel_dropout')
        return y

    @staticmethod
    def backward(ctx, gy):
        gy = gy.float().contiguous()
        gx = torch.empty_like(gy)
        _lib.check(_lib.lib().dcf_op_channel_dropout(_lib.ptr(gy), _lib.ptr(gx), *ctx.geom, _lib.current_stream()), 'dcf_op_channel_dropout')
        return gx, None, None, None, None


def channel_dropout(x, drop):
    """nn.Dropout1d(drop.proj_p) (model.py:614) on token-major ``x`` (B, T, C) of the reference's (B, C, T) tensor: one keep decision
    per (sample, channel), element index ``(b0 + b) * C + c``, at sub DROP_CHANNEL of the group / layer ``drop`` names (the clip
    features before vid_map: ``DropSpec(seed, b0, proj_p=cdrop, group=DROP_G_INPUT)``).  The backward is the same operator on the
    gradient."""
    drop = _active(drop, 'channel_dropout')
    if drop is None or drop.proj_p == 0.0:
        return x
    return _ChannelDropoutFn.apply(x, drop.key, drop.site(DROP_CHANNEL), drop.proj_p, drop.b0)


def gelu_dropout(x, drop, sub=DROP_FFN_HID):
    """``dropout(gelu(x))`` of FFN.forward (blocks.py:535-536) in one pass, forward and backward, with the bits of the two operators in
    a row; without an active ``drop`` it is ``gelu``."""
    drop = _active(drop, 'gelu_dropout')
    if drop is None or drop.proj_p == 0.0:
        return gelu(x)
    return _GeluDropoutFn.apply(x, drop.key, drop.site(sub), drop.proj_p, drop.b0)


def layer_scale_residual(r, h, scale, r_mask=None, h_mask=None, drop=None, subs=(DROP_FFN_OUT, DROP_PATH_FFN)):
    """A residual through LayerScale (blocks.py:670-682): ``r * r_mask + scale * (h * h_mask)`` on token-major (B, T, C),
    ``scale`` of C elements in any shape (the reference keeps (1, C, 1)); blocks.py:586 is ``r_mask = mask``, :589-590 ``h_mask = mask``.
    With ``drop``: ``r * r_mask + drop_path(scale * dropout(h * h_mask))``, the dropout of ``h`` at rate ``drop.proj_p`` and site
    ``subs[0]``, the drop-path at rate ``drop.path_p`` and site ``subs[1]`` -- (DROP_PROJ, DROP_PATH_ATTN) for the attention branch,
    (DROP_FFN_OUT, DROP_PATH_FFN), the FFN's last dropout, for the FFN branch."""
    drop = _active(drop, 'layer_scale_residual')
    if drop is None or h is None:
        return _LayerScaleResidualFn.apply(r, h, scale, r_mask, h_mask)
    return _DropResidualFn.apply(r, h, scale, r_mask, h_mask, drop.key, drop.b0, drop.site(subs[0]), drop.proj_p, drop.site(subs[1]), drop.path_p)


def ffn(x, ffn_module, drop=None):
    """FFN.forward (blocks.py:535-538) on token-major ``x`` (B, T, C), with ``ffn_module`` a modeling.FFN:
    proj(gelu(fc(x))), the two k = 1 convolutions unmasked (the reference's are plain nn.Conv1d).  Saved for the backward: ``x`` (by fc),
    the pre-activation fc(x) (by gelu, which recomputes Phi and phi from it) and gelu(fc(x)) (by proj, as the operand of its weight
    gradient) -- two (B, T, 4 C) tensors per call.  With ``drop`` the hidden tensor is ``gelu_dropout`` (site DROP_FFN_HID); the
    dropout behind ``proj`` (:538, site DROP_FFN_OUT) is NOT applied here: it is part of the ``layer_scale_residual`` that follows."""
    h = masked_conv1d(x, None, ffn_module.fc.weight, ffn_module.fc.bias)
    return masked_conv1d(gelu_dropout(h, drop), None, ffn_module.proj.weight, ffn_module.proj.bias)


def conv_attn_layer(x, mask, layer, drop=None):
    """ConvAttNLayer.forward (blocks.py:462-473) on token-major ``x`` (B, T, C), with ``layer`` a modeling.ConvAttNLayer of stride 1 or 2;
    of ``drop`` the layer takes the map dropout of ``masked_mha`` alone: q / k / v = {q,k,v}_norm({q,k,v}_conv(x, mask)), then the MaskedMHA under the strided mask, local (``window_size > 0``)
    or global (``window_size = 0``, head dimension 32 or 64) -> ((B, T / stride, C), ``mask[:, ::stride]``)."""
    if not hasattr(layer, 'q_conv'):
        raise ValueError('conv_attn_layer: stride 0 (no depthwise convolutions: the text encoder) has no backward here')
    if layer.attn.window_size == 0:
        limit = _global_head_limit(x.size(-1), layer.attn.n_heads)
        if limit:
            raise ValueError(f'conv_attn_layer: window_size = 0: {limit}')
    B, T, _ = x.shape
    if mask is None:
        mask = torch.ones(B, T, dtype=torch.bool, device=x.device)
    (q, k, v), mask = depthwise_conv1d(x, mask, [layer.q_conv.conv.weight, layer.k_conv.conv.weight, layer.v_conv.conv.weight], layer.q_conv.stride)
    q = channel_layer_norm(q, layer.q_norm.weight, layer.q_norm.bias)
    k = channel_layer_norm(k, layer.k_norm.weight, layer.k_norm.bias)
    v = channel_layer_norm(v, layer.v_norm.weight, layer.v_norm.bias)
    return masked_mha(q, k, v, mask, layer.attn, **_drop_kw(drop)), mask


def transformer_encoder(x, mask, block, drop=None, narrow_heads=False):
    """TransformerEncoder.forward (blocks.py:578-591) on token-major ``x`` (B, T, C), with ``block`` a modeling.TransformerEncoder of
    stride 1 or 2 (a stem or pyramid block of the video encoder; local window, or ``window_size = 0``: global self-attention over the
    clips, head dimension 32 or 64) -> (y (B, T / stride, C), ``mask[:, ::stride]``), or of stride 0 and ``window_size = 0`` (a block of
    the text encoder: no depthwise convolutions, q = k = v = ln_attn(x * mask) through the global branch of MaskedMHA, ``xattn_mha``).  A
    stride-0 block of at most 64 positions runs on ``cross_attention`` (head dimension 16 / 32 / 64 / 128; ``narrow_heads=True``, which
    ``text_transformer`` passes, also admits heads of 8 channels, which ``xattn_mha`` runs as zero-padded heads of 16); a longer one runs
    on ``global_attention`` and needs a head dimension of 32 or 64.  A limit is raised with its own message before anything runs
    -> (y (B, T, C), mask).
    To the letter: the input is multiplied by the mask (:581); at stride 2 the skip is masked_max_pool1d of that (:584) but is masked
    with the convolution's mask ``mask[:, ::2]``, not with the pooled one (:586); the output is not masked, so padded rows hold
    ``drop_path_attn.scale * attn.proj.bias``.  ``drop`` (stride 1 / 2 only; group DROP_G_STEM or DROP_G_BRANCH): proj_drop
    (blocks.py:392, sub 0) and drop_path_attn (3) in the first residual, the FFN's dropouts (1, 2) and drop_path_ffn (4), on the
    (B, C, T / stride) tensors of the reference, and with ``drop.attn_p`` attn_drop on the attention map (blocks.py:368 / :388, sub 6).
    A stride-0 block takes the same sites (group DROP_G_TEXT)."""
    if block.stride not in (0, 1, 2):
        raise ValueError(f'transformer_encoder: stride = {block.stride} (0: the text encoder, 1 or 2: the video encoder)')
    if block.stride == 0 and block.window_size != 0:
        raise ValueError(f'transformer_encoder: stride = 0 with window_size = {block.window_size}: the stride-0 blocks of the text encoder have '
                         f'no local window')
    B, T, C = x.shape
    if block.stride and block.window_size == 0:
        # known to be unsupported before the device check and before anything is launched
        limit = _global_head_limit(C, block.attn.attn.n_heads)
        if limit:
            raise ValueError(f'transformer_encoder: stride = {block.stride} with window_size = 0: {limit}')
    if block.stride and T % block.stride:
        raise ValueError(f'transformer_encoder: T = {T} must be a multiple of the stride {block.stride}')
    if block.stride == 0:
        # the block is known to be unsupported before anything is launched: cross_attention's own message, with the block named
        limit = (_global_attention_limit if narrow_heads else _cross_attention_limit)(T, C, block.attn.attn.n_heads)
        if limit and T > 64 and _global_head_limit(C, block.attn.attn.n_heads) is None:
            limit = None                                 # more than 64 positions on heads of 32 / 64 channels: global_attention
        if limit:
            raise ValueError(f'transformer_encoder: stride = 0 (global self-attention of the text encoder): {limit}')
    drop = _active(drop, 'transformer_encoder')
    if mask is None:
        mask = torch.ones(B, T, dtype=torch.bool, device=x.device)
    x = _LayerScaleResidualFn.apply(x, None, None, mask, None)
    if block.stride == 0:
        mask = _mask_rows(mask, B, T)
        q = channel_layer_norm(x, block.ln_attn.weight, block.ln_attn.bias)
        skip, h = x, xattn_mha(q, q, mask, block.attn.attn, **_drop_kw(drop))
    else:
        skip = masked_max_pool1d(x, mask)[0] if block.stride == 2 else x
        h, mask = conv_attn_layer(channel_layer_norm(x, block.ln_attn.weight, block.ln_attn.bias), mask, block.attn, **_drop_kw(drop))
    x = layer_scale_residual(skip, h, block.drop_path_attn.scale, r_mask=mask, drop=drop, subs=(DROP_PROJ, DROP_PATH_ATTN))
    h = ffn(channel_layer_norm(x, block.ln_ffn.weight, block.ln_ffn.bias), block.ffn, drop)
    return layer_scale_residual(x, h, block.drop_path_ffn.scale, h_mask=mask, drop=drop), mask


def _cross_attention_limit(Lk, C, n_heads):
    """the message of the limit of ``cross_attention`` that (Lk keys, C channels on n_heads heads) breaks, or None"""
    if not 1 <= Lk <= 64:
        return f'cross_attention: Lk = {Lk} keys (1 to 64 have a backward)'
    if C % n_heads or C // n_heads not in (16, 32, 64, 128):
        return f'cross_attention: C = {C} on {n_heads} heads: the head dimension must be 16, 32, 64 or 128'
    return None


_WIDE_HEAD = 16    # the narrowest head of cross_attention


def _global_attention_limit(Lk, C, n_heads):
    """``_cross_attention_limit`` for ``xattn_mha``, which also admits heads of 8 channels (run as heads of 16: ``_narrow_head_attention``)"""
    if C % n_heads == 0 and C // n_heads == 8:
        return _cross_attention_limit(Lk, n_heads * _WIDE_HEAD, n_heads)
    return _cross_attention_limit(Lk, C, n_heads)


def _narrow_head_attention(q, k, v, kv_mask, n_heads, drop=None):
    """``cross_attention`` for heads of d = 8 channels, narrower than the kernels' narrowest (16): every head is laid into the first d of
    16 channels, the rest zero, which leaves q . k and the values untouched; the kernels scale q and k by 16^-1/4 each where the
    reference has d^-1/4, so q and k are multiplied by (16 / d)^1/4 first.  The layout steps are torch's and differentiable; the
    attention and its backward are the same HIP kernels.  The text encoder of a model with text_net heads of 8 channels is where
    this occurs: at most 64 keys.  The channels are padded, not the keys: the element index of the map's dropout is unchanged."""
    B, T, C = q.shape
    d = C // n_heads
    gain = (_WIDE_HEAD / d) ** 0.25

    def widen(z, g):
        z = z.reshape(z.size(0), z.size(1), n_heads, d)
        return torch.nn.functional.pad(z if g is None else z * g, (0, _WIDE_HEAD - d)).reshape(z.size(0), z.size(1), n_heads * _WIDE_HEAD)

    o = cross_attention(widen(q, gain), widen(k, gain), widen(v, None), kv_mask, n_heads, **_drop_kw(drop))
    return o.reshape(B, T, n_heads, _WIDE_HEAD)[..., :d].reshape(B, T, C)


class _CrossAttentionFn(torch.autograd.Function):
    """``drop``: None, or (key, site, p, b0) of the dropout on the map (dcf_op_xattn_drop / dcf_op_xattn_drop_bwd)"""

    @staticmethod
    def forward(ctx, q, k, v, kv_mask, n_heads, drop):
        qd, kd, vd, m, o = _attn_operands('cross_attention', q, k, v, kv_mask, cross=True)
        B, T, C = qd.shape
        limit = _cross_attention_limit(kd.size(1), C, n_heads)
        if limit:
            raise ValueError(limit)
        ctx.geom, ctx.drop = (B, T, kd.size(1), C, int(n_heads)), _map_drop(drop)
        _attn_launch('dcf_op_xattn', 'dcf_op_xattn_drop', (qd, kd, vd, m, o), ctx.geom, ctx.drop)
        ctx.save_for_backward(qd, kd, vd, m)
        return o

    @staticmethod
    def backward(ctx, go):
        return _attn_backward(ctx, go, 'dcf_op_xattn_bwd', 'dcf_op_xattn_drop_bwd', ctx.geom) + (None,) * 3


class _AdaLnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mask, h, norm):
        B, T, C = x.shape
        xd, hd = _rows(x, 'adaln_modulate'), _rows(h, 'adaln_modulate')
        if hd.shape != (B, T, 2 * C):
            raise ValueError(f'adaln_modulate: x {tuple(x.shape)} needs h (B, T, 2 C), got {tuple(h.shape)}')
        m = _byte_mask(mask, B, T, 'adaln_modulate')
        y = torch.empty_like(xd)
        _lib.check(_lib.lib().dcf_op_adaln(_lib.ptr(xd), _lib.ptr(m), _lib.ptr(hd), _lib.ptr(y), B * T, C, int(bool(norm)), _lib.current_stream()),
                   'dcf_op_adaln')
        ctx.save_for_backward(xd, m, hd)
        ctx.norm = int(bool(norm))
        return y

    @staticmethod
    def backward(ctx, gy):
        x, m, h = ctx.saved_tensors
        B, T, C = x.shape
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gh = torch.empty_like(h) if ctx.needs_input_grad[2] else None
        gy = gy.float().contiguous()
        if gx is not None or gh is not None:
            _lib.check(_lib.lib().dcf_op_adaln_bwd(_lib.ptr(x), _lib.ptr(m), _lib.ptr(h), _lib.ptr(gy), _lib.ptr(gx), _lib.ptr(gh),
                                                   B * T, C, ctx.norm, _lib.current_stream()), 'dcf_op_adaln_bwd')
        return gx, None, gh, None


def cross_attention(q, k, v, kv_mask, n_heads, drop=None, sub=None):
    """The global cross-attention core of MaskedMHA (blocks.py:374-389) on token-major ``q`` (B, T, C) and ``k`` / ``v`` (B, Lk, C), heads
    concatenated along C: softmax over the valid keys of the sequence, d^-1/4 on q and on k, masked keys filled with -inf -> (B, T, C).
    ``kv_mask``: (B, Lk) or (B, 1, Lk), None = all valid; every sequence needs a valid key.  There is no query mask.  Lk from 1 to 64,
    head dimension 16, 32, 64 or 128.  ``drop`` with ``attn_p > 0``: nn.Dropout(attn_p) on the (B, H, T, Lk) map (blocks.py:388) at site
    ``sub`` (DROP_ATTN), drawn inside the kernels, forward and backward."""
    drop = _active(drop, 'cross_attention')
    return _CrossAttentionFn.apply(q, k, v, kv_mask, n_heads, _map_site(drop, sub))


def adaln_modulate(x, mask, h, norm=True):
    """blocks.py:643-645 on token-major ``x`` (B, T, C) and the cross-attention output ``h`` (B, T, 2 C):
    ``adaln(x * mask) * h[..., :C] + h[..., C:]`` with adaln the channel LayerNorm without affine parameters (``norm``, xattn_mode
    'adaln') or the identity (xattn_mode 'affine').  ``mask``: (B, T) or (B, 1, T), None = all valid."""
    return _AdaLnFn.apply(x, mask, h, norm)


def _repeat(x, kv_size, n):
    """``x.repeat_interleave(kv_size, dim=0)`` with the known result size ``n`` (no host wait for the sum of the counts)"""
    return x.repeat_interleave(torch.as_tensor(kv_size, device=x.device), dim=0, output_size=n)


def xattn_mha(q_in, kv_in, kv_mask, mha, kv_size=None, drop=None):
    """MaskedMHA.forward in its global branch as the fusion calls it (blocks.py:327-356, :374-393; k = v = kv, no dropout) on token-major
    ``q_in`` (B, T, Cq) and ``kv_in`` (B', Lk, Ckv), with ``mha`` a modeling.MaskedMHA of ``window_size = 0``:
    proj(cross_attention(query(q_in), key(kv_in), value(kv_in))) -> (B', T, out_dim).  ``kv_size`` (B,): how many of the B' key
    sequences belong to each query sequence; the PROJECTED query is repeated to match (:352-355).  Heads of 8 channels, narrower than
    ``cross_attention`` admits, run as zero-padded heads of 16 (``_narrow_head_attention``).  Self-attention (``q_in is kv_in``, no
    ``kv_size``) over more than 64 positions on heads of 32 or 64 channels runs on ``global_attention``, which has no limit on the
    length; up to 64 positions nothing changes.  ``drop``: its ``attn_p`` is the rate of attn_drop (:388) on the map."""
    if mha.window_size != 0:
        raise ValueError('xattn_mha: a MaskedMHA with window_size = 0 is required (the local branch is masked_mha)')
    q = masked_conv1d(q_in, None, mha.query.weight, mha.query.bias)
    k = masked_conv1d(kv_in, None, mha.key.weight, mha.key.bias)
    v = masked_conv1d(kv_in, None, mha.value.weight, mha.value.bias)
    if kv_size is not None and k.size(0) != q.size(0):
        q = _repeat(q, kv_size, k.size(0))
    narrow = q.size(2) % mha.n_heads == 0 and q.size(2) // mha.n_heads == 8
    if q_in is kv_in and kv_size is None and k.size(1) > 64 and _global_head_limit(q.size(2), mha.n_heads) is None:
        ctx = global_attention(q, k, v, kv_mask, mha.n_heads, **_drop_kw(drop))
    else:
        ctx = (_narrow_head_attention if narrow else cross_attention)(q, k, v, kv_mask, mha.n_heads, **_drop_kw(drop))
    return masked_conv1d(ctx, None, mha.proj.weight, mha.proj.bias)


def conv_xattn_layer(q, q_mask, kv, kv_mask, layer, kv_size=None, drop=None):
    """ConvXAttNLayer.forward (blocks.py:513-520; stride 1; of ``drop`` the map dropout of ``xattn_mha`` alone) on token-major ``q`` (B, T, C) and ``kv`` (B', Lk, Ckv), with
    ``layer`` a modeling.ConvXAttNLayer: xattn(q_norm(q_conv(q, q_mask)), kv) -> ((B', T, out_dim), the mask repeated like the batch)."""
    B, T, _ = q.shape
    (qc,), _ = depthwise_conv1d(q, q_mask, [layer.q_conv.conv.weight], 1)
    qc = channel_layer_norm(qc, layer.q_norm.weight, layer.q_norm.bias)
    out = xattn_mha(qc, kv, kv_mask, layer.xattn, kv_size, **_drop_kw(drop))
    q_mask = _mask_rows(q_mask, B, T)
    if kv_size is not None and q_mask is not None and out.size(0) != q_mask.size(0):
        q_mask = _repeat(q_mask, kv_size, out.size(0))
    return out, q_mask


def transformer_decoder(q, q_mask, kv, kv_mask, block, kv_size=None, drop=None):
    """TransformerDecoder.forward (blocks.py:632-650) on token-major ``q`` (B, T, E) and ``kv`` (B', Lk, TE), with ``block`` a
    modeling.TransformerDecoder -> (y (B', T, E), the query mask (B', T)).  To the letter: the input is multiplied by the mask (:635);
    the cross attention sees ln_xattn_q of that and ln_xattn_kv(kv); with ``kv_size`` the query residual is repeated to the B' text
    queries (:641-642); the residual is masked again, normalised without affine parameters ('adaln') or left as it is ('affine'), and
    modulated by the two halves of the cross-attention output (:643-645); the FFN branch is masked, the output is not, so padded rows
    hold the shift.  ``drop`` (group DROP_G_FUSION): proj_drop on the (B', 2E, T) scale / shift tensor before the modulation (sub 0),
    the FFN's dropouts (1, 2) and drop_path_ffn (4), and with ``drop.attn_p`` attn_drop on the cross-attention map (6); the decoder has no
    drop_path_attn."""
    B, T, _ = q.shape
    q_mask = torch.ones(B, T, dtype=torch.bool, device=q.device) if q_mask is None else _mask_rows(q_mask, B, T)
    q = _LayerScaleResidualFn.apply(q, None, None, q_mask, None)
    h, mask = conv_xattn_layer(channel_layer_norm(q, block.ln_xattn_q.weight, block.ln_xattn_q.bias), q_mask,
                               channel_layer_norm(kv, block.ln_xattn_kv.weight, block.ln_xattn_kv.bias), kv_mask, block.xattn, kv_size,
                               **_drop_kw(_active(drop, 'transformer_decoder')))
    if kv_size is not None and q.size(0) != h.size(0):
        q = _repeat(q, kv_size, h.size(0))
    drop = _active(drop, 'transformer_decoder')
    q = adaln_modulate(q, mask, dropout(h, drop, DROP_PROJ), norm=block.xattn_mode == 'adaln')
    h = ffn(channel_layer_norm(q, block.ln_ffn.weight, block.ln_ffn.bias), block.ffn, drop)
    return layer_scale_residual(q, h, block.drop_path_ffn.scale, h_mask=mask, drop=drop), mask


def xattn_fusion(vid, vid_mask, text, text_mask, fusion, kv_size=None, drop=None, group=DROP_G_FUSION, layer0=0):
    """XAttNFusion._forward (fusion.py:56-66) on token-major ``vid`` (B, T, E) and ``text`` (B', Lk, TE), with ``fusion`` a
    modeling.XAttNFusion: its decoder layers, ln_out, and the repeat by ``kv_size`` when no layer expanded the batch
    -> (fused (B', T, E), mask (B', T)).  ``drop``: decoder layer i is layer ``layer0 + i`` of ``group`` (DROP_G_FUSION, layer0 = 0; the
    fusion applied again to pyramid level l is DROP_G_FUSION2 with layer0 = l * n_layers: ``fuse_and_predict``)."""
    B, T, _ = vid.shape
    vid_mask = torch.ones(B, T, dtype=torch.bool, device=vid.device) if vid_mask is None else _mask_rows(vid_mask, B, T)
    drop = _active(drop, 'xattn_fusion')
    for i, layer in enumerate(fusion.layers):
        if drop is None:
            vid, vid_mask = transformer_decoder(vid, vid_mask, text, text_mask, layer, kv_size)
        else:
            vid, vid_mask = transformer_decoder(vid, vid_mask, text, text_mask, layer, kv_size, drop=drop.at(group, layer0 + i))
    vid = channel_layer_norm(vid, fusion.ln_out.weight, fusion.ln_out.bias)
    if kv_size is not None and vid.size(0) != text.size(0):
        vid, vid_mask = _repeat(vid, kv_size, text.size(0)), _repeat(vid_mask, kv_size, text.size(0))
    return vid, vid_mask


_TCN_C = 32        # channels of the refinement TCN (model.py:424)


def _drop_args(dropout, name):
    """(seed, p, b0) of ``dropout`` = None or (seed, p, b0)"""
    if dropout is None:
        return 0, 0.0, 0
    seed, p, b0 = dropout
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f'{name}: dropout p = {p} must lie in [0, 1)')
    if int(b0) < 0:
        raise ValueError(f'{name}: dropout b0 = {b0} must not be negative')
    return int(seed), p, int(b0)


def _vec(t, n, name, what):
    if t.numel() != n:
        raise ValueError(f'{name}: {what} {tuple(t.shape)} must hold {n} elements')
    return t.detach().float().reshape(n).contiguous()


class _RefineInFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits1, mask0, weight, bias):
        if not (torch.is_tensor(logits1) and logits1.is_cuda and logits1.dim() == 2):
            raise RuntimeError('refine_in: (B, S) logits on the GPU are required (there is no CPU path)')
        B, S = logits1.shape
        if weight.dim() not in (2, 3) or weight.size(0) != _TCN_C or weight[0].numel() != weight.size(1):
            raise ValueError(f'refine_in: weight {tuple(weight.shape)} must be ({_TCN_C}, L) or ({_TCN_C}, L, 1)')
        L = weight.size(1)
        if not 1 <= L <= 16:
            raise ValueError(f'refine_in: L = {L} pyramid levels (1 to 16)')
        T0, rem = divmod(S << (L - 1), (1 << L) - 1)                   # S = sum_l T0 >> l = T0 (2^L - 1) / 2^(L-1)
        if rem or T0 == 0 or T0 % (1 << (L - 1)):
            raise ValueError(f'refine_in: S = {S} is not the length of a pyramid of {L} levels (T0 must be a multiple of {1 << (L - 1)})')
        m = _byte_mask(mask0, B, T0, 'refine_in')
        lg = logits1.detach().float().contiguous()
        w, b = weight.detach().float().reshape(_TCN_C, L).contiguous(), _vec(bias, _TCN_C, 'refine_in', 'bias')
        h = torch.empty(B, T0, _TCN_C, dtype=torch.float32, device=lg.device)
        _lib.check(_lib.lib().dcf_op_refine_in(_lib.ptr(lg), _lib.ptr(m), _lib.ptr(w), _lib.ptr(b), _lib.ptr(h), B, T0, L, _lib.current_stream()),
                   'dcf_op_refine_in')
        ctx.save_for_backward(lg, m, w)
        ctx.shapes = (weight.shape, bias.shape)
        return h

    @staticmethod
    def backward(ctx, gh):
        lg, m, w = ctx.saved_tensors
        (B, S), L = lg.shape, w.size(1)
        gh = gh.float().contiguous()
        T0 = gh.size(1)
        gl = torch.empty_like(lg) if ctx.needs_input_grad[0] else None
        gw = torch.empty_like(w) if ctx.needs_input_grad[2] else None
        gb = torch.empty(_TCN_C, dtype=torch.float32, device=lg.device) if ctx.needs_input_grad[3] else None
        if gl is not None or gw is not None or gb is not None:
            _lib.check(_lib.lib().dcf_op_refine_in_bwd(_lib.ptr(lg), _lib.ptr(m), _lib.ptr(w), _lib.ptr(gh), _lib.ptr(gl), _lib.ptr(gw), _lib.ptr(gb),
                                                       B, T0, L, 0, _lib.current_stream()), 'dcf_op_refine_in_bwd')
        return (gl, None, gw.reshape(ctx.shapes[0]) if gw is not None else None, gb.reshape(ctx.shapes[1]) if gb is not None else None)


class _TcnLayerFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mask, wd, bd, wp, bp, lnw, lnb, dilation, site_layer, seed, p, b0):
        xd = _rows(x, 'tcn_layer')
        B, T0, C = xd.shape
        if C != _TCN_C or tuple(wd.shape) != (C, C, 3) or wp.numel() != C * C or wp.size(0) != C:
            raise ValueError(f'tcn_layer: x {tuple(x.shape)}, conv_dilated {tuple(wd.shape)}, conv_1x1 {tuple(wp.shape)}: the refinement TCN '
                             f'has {_TCN_C} channels, a ({_TCN_C}, {_TCN_C}, 3) and a ({_TCN_C}, {_TCN_C}[, 1]) weight')
        if dilation < 1:
            raise ValueError(f'tcn_layer: dilation = {dilation} must be at least 1')
        m = _byte_mask(mask, B, T0, 'tcn_layer')
        params = (wd.detach().float().contiguous(), _vec(bd, C, 'tcn_layer', 'conv_dilated.bias'), wp.detach().float().reshape(C, C).contiguous(),
                  _vec(bp, C, 'tcn_layer', 'conv_1x1.bias'), _vec(lnw, C, 'tcn_layer', 'norm.weight'), _vec(lnb, C, 'tcn_layer', 'norm.bias'))
        y = torch.empty_like(xd)
        _lib.check(_lib.lib().dcf_op_tcn_layer(_lib.ptr(xd), _lib.ptr(m), *(_lib.ptr(t) for t in params), _lib.ptr(y), B, T0, dilation, seed, p,
                                               site_layer, b0, _lib.current_stream()), 'dcf_op_tcn_layer')
        ctx.save_for_backward(xd, m, *params)
        ctx.geom = (dilation, site_layer, seed, p, b0)
        ctx.shapes = tuple(t.shape for t in (wd, bd, wp, bp, lnw, lnb))
        return y

    @staticmethod
    def backward(ctx, gy):
        x, m, *params = ctx.saved_tensors
        B, T0, C = x.shape
        dilation, site_layer, seed, p, b0 = ctx.geom
        gy = gy.float().contiguous()
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gp = [torch.empty_like(t) if need else None for t, need in zip(params, ctx.needs_input_grad[2:8])]
        if gx is not None or any(g is not None for g in gp):
            _lib.check(_lib.lib().dcf_op_tcn_layer_bwd(_lib.ptr(x), _lib.ptr(m), *(_lib.ptr(t) for t in params), _lib.ptr(gy), _lib.ptr(gx),
                                                       *(_lib.ptr(g) for g in gp), B, T0, dilation, seed, p, site_layer, b0, 0,
                                                       _lib.current_stream()), 'dcf_op_tcn_layer_bwd')
        gp = [g.reshape(shape) if g is not None else None for g, shape in zip(gp, ctx.shapes)]
        return (gx, None, *gp, None, None, None, None, None)


def refine_in(logits1, mask0, tcn_module):
    """model.py:449-455 fused with TCN.conv_1x1 (tcn.py:69-70), with ``tcn_module`` a modeling.TCN of L input channels: ``logits1`` (B, S),
    the first-pass logits of the L pyramid levels side by side (level l: T0 >> l entries), each level nearest-upsampled to T0, levels
    l > 0 multiplied by ``mask0`` (B, T0) or (B, 1, T0) (level 0 is not masked, to the letter), then mapped to 32 channels -> (B, T0, 32)."""
    return _RefineInFn.apply(logits1, mask0, tcn_module.conv_1x1.weight, tcn_module.conv_1x1.bias)


def tcn_layer(x, mask, layer, dilation, dropout=None, site_layer=None):
    """DilatedResidualLayer.forward (tcn.py:21-38) on token-major ``x`` (B, T0, 32), with ``layer`` a modeling.DilatedResidualLayer:
    ``LayerNorm((x + drop(conv_1x1(relu(conv_dilated(x))))) * mask)``; the dilated convolution does not mask its input.  ``dropout``:
    None or (seed, p, b0) -- the keep bits of the training forward for sequence b0 + b of its batch at the site of TCN layer
    ``site_layer`` (default: log2 of a power-of-two ``dilation``, as modeling.TCN numbers its layers).  The backward saves ``x`` alone."""
    dilation = int(dilation)
    seed, p, b0 = _drop_args(dropout, 'tcn_layer')
    if site_layer is None:
        if p > 0.0 and (dilation < 1 or dilation & (dilation - 1)):
            raise ValueError(f'tcn_layer: dropout on a layer of dilation {dilation} needs site_layer (the layer\'s index in its TCN)')
        site_layer = max(dilation, 1).bit_length() - 1 if not dilation & (dilation - 1) else 0
    return _TcnLayerFn.apply(x, mask, layer.conv_dilated.weight, layer.conv_dilated.bias, layer.conv_1x1.weight, layer.conv_1x1.bias,
                             layer.norm.weight, layer.norm.bias, dilation, int(site_layer), seed, p, b0)


def tcn(logits1, mask0, tcn_module, dropout=None):
    """TCN.forward (tcn.py:66-84) behind the stacking of model.py:449-455: ``refine_in``, the layers of dilation 2^i, then
    ``conv_out(x) * mask0`` -> (B, T0, 32).  ``dropout``: None or (seed, p, b0) for every layer's Dropout (tcn.py:27)."""
    x = refine_in(logits1, mask0, tcn_module)
    B, T0, _ = x.shape
    for i, layer in enumerate(tcn_module.layers):
        x = tcn_layer(x, mask0, layer, layer.conv_dilated.dilation[0], dropout, site_layer=i)
    x = masked_conv1d(x, None, tcn_module.conv_out.weight, tcn_module.conv_out.bias)
    return x if mask0 is None else _LayerScaleResidualFn.apply(x, None, None, _mask_rows(mask0, B, T0), None)


def fuse_and_predict(fpn, fpn_masks, model, dropout=None, text=None, text_mask=None, kv_size=None, fusion_drop=None):
    """PtTransformerEarlyFusionIterative.fuse_and_predict (model.py:442-471) on token-major pyramid levels ``fpn[l]`` (B, T0 >> l, E) with
    masks ``fpn_masks[l]`` (B, T0 >> l) or (B, 1, T0 >> l), ``model`` a modeling.PtTransformerEarlyFusionIterative -> (logits1, logits2,
    offsets, masks), tuples over the levels of (B', T_l), (B', T_l), (B', T_l, 2) and (B', T_l) bool: what ``loss.PointObjective`` takes.
    With ``model.second_fusion`` every level first goes through ``xattn_fusion`` against ``text`` (B', Lk, TE) / ``text_mask`` /
    ``kv_size``.  To the letter: the refined map is pooled down the pyramid with ``fpn_masks[i - 1]``, the pooled mask is discarded, and
    the heads see ``fpn_masks[i]``.  ``dropout``: None or (seed, p, b0) for the refinement TCN, the seed as ``model.enable_dropout``
    hands it out (``model.last_dropout_seed``).  ``fusion_drop`` (with ``model.second_fusion``): the fusion's dropouts at level l under
    group DROP_G_FUSION2, layer ``l * n_layers + i`` -- the modules are the first fusion's, called again, so the call is part of the site."""
    n_levels = len(model.refine.layers)
    if len(fpn) != n_levels or len(fpn_masks) != n_levels:
        raise ValueError(f'fuse_and_predict: {len(fpn)} levels and {len(fpn_masks)} masks for a model of {n_levels} pyramid levels')
    E = model.cls_head.convs[0].conv.weight.size(1) if len(model.cls_head.convs) else model.cls_head.cls_head.conv.weight.size(1)
    T0 = fpn[0].size(1) if torch.is_tensor(fpn[0]) and fpn[0].dim() == 3 else 0
    for l, x in enumerate(fpn):
        x = _rows(x, 'fuse_and_predict')
        if x.size(2) != E:
            raise ValueError(f'fuse_and_predict: level {l} has {x.size(2)} channels, the heads take {E}')
        if x.size(1) != T0 >> l or (l + 1 < n_levels and x.size(1) % 2):
            raise ValueError(f'fuse_and_predict: level {l} has length {x.size(1)}: the levels must be T0 >> l = {T0 >> l}, even above the last')
    masks = [_mask_rows(m, x.size(0), x.size(1)) for m, x in zip(fpn_masks, fpn)]
    if any(m is None for m in masks):
        raise ValueError('fuse_and_predict: every level needs its mask')
    if model.second_fusion:
        if text is None:
            raise ValueError('fuse_and_predict: a model with second_fusion needs the text')
        n_layers = len(model.fusion.layers)
        fusion_drop = _active(fusion_drop, 'fuse_and_predict')
        if fusion_drop is not None and n_levels * n_layers > 1 << 12:
            raise ValueError(f'fuse_and_predict: {n_levels} levels x {n_layers} fusion layers do not fit the 4096 layers of a site group')
        second = lambda l: {} if fusion_drop is None else dict(drop=fusion_drop, group=DROP_G_FUSION2, layer0=l * n_layers)
        fused = [xattn_fusion(x, m, text, text_mask, model.fusion, kv_size, **second(l)) for l, (x, m) in enumerate(zip(fpn, masks))]
        fpn, masks = [f[0] for f in fused], [f[1] for f in fused]
    logits1 = [conv_head(x, m, model.cls_head) for x, m in zip(fpn, masks)]
    refined = tcn(torch.cat(logits1, dim=1), masks[0], model.refine, dropout)
    new_fpn = []
    for i, x in enumerate(fpn):
        if i:
            refined = masked_max_pool1d(refined, masks[i - 1])[0]
        new_fpn.append(torch.cat([x, refined], dim=2))
    logits2 = [conv_head(x, m, model.cls_head2) for x, m in zip(new_fpn, masks)]
    offsets = [conv_head(x, m, model.reg_head, level=l) for l, (x, m) in enumerate(zip(new_fpn, masks))]
    return tuple(logits1), tuple(logits2), tuple(offsets), tuple(masks)


def _position_term(module, t, mask, name):
    """``pe[:t] * mask`` of a backbone (video_net.py:75-78, :141-151 / text_net.py:121-124, :166-176; the training branch), token-major
    (B, t, E), or None without ``use_abs_pe``"""
    if not module.use_abs_pe:
        return None
    if t > module.max_seq_len:
        raise ValueError(f'{name}: {t} positions exceed max_seq_len = {module.max_seq_len} (the training branch does not resample the '
                         f'position encoding)')
    pe = getattr(module, 'pe', None)
    if pe is None:
        from .modeling import sinusoid_encoding
        pe = sinusoid_encoding(module.max_seq_len, module.embd_dim // 2) / module.embd_dim ** 0.5
    pe = pe[:, :t].t().to(device=mask.device, dtype=torch.float32)
    return pe[None] * mask[..., None].to(torch.float32)


def video_transformer(x, mask, vid_net, drop=None):
    """VideoTransformer.forward (video_net.py:123-164, the training branch) on token-major ``x`` (B, T, in_dim), with ``vid_net`` a
    modeling.VideoTransformer -> (fpn, fpn_masks), tuples over the pyramid levels of (B, T_l, E) and (B, T_l) bool.  To the letter:
    the output of embd_fc is not masked (:133; the convolution behind it masks its input); each embedding convolution, k = 3 or
    k = 5 / stride 2, is followed by LayerNorm + ReLU; ``pe[:t] * mask`` is added under the mask of the shortened sequence; a
    ``pool_only`` branch layer is one depthwise k = 3 convolution, stride 1 at the first level and 2 after it.  ``drop``: stem layer i
    is layer i of group DROP_G_STEM, the block of pyramid level l layer l of group DROP_G_BRANCH (a ``pool_only`` layer has none)."""
    B, T, _ = x.shape
    mask = torch.ones(B, T, dtype=torch.bool, device=x.device) if mask is None else _byte_mask(mask, B, T, 'video_transformer')
    x = masked_conv1d(x, mask, vid_net.embd_fc.conv.weight, vid_net.embd_fc.conv.bias)
    for conv, norm in zip(vid_net.embd_convs, vid_net.embd_norms):
        if conv.stride == 2:
            x, mask = strided_masked_conv1d(x, mask, conv.conv.weight)
        else:
            x = masked_conv1d(x, mask, conv.conv.weight, conv.conv.bias)
        x = channel_layer_norm(x, norm.weight, norm.bias, relu=True)
    pe = _position_term(vid_net, x.size(1), mask, 'video_transformer')
    if pe is not None:
        x = x + pe
    drop = _active(drop, 'video_transformer')
    for i, block in enumerate(vid_net.stem):
        x, mask = transformer_encoder(x, mask, block) if drop is None else transformer_encoder(x, mask, block, drop=drop.at(DROP_G_STEM, i))
    fpn, fpn_masks = [], []
    for l, block in enumerate(vid_net.branch):
        if vid_net.pool_only:
            (x,), mask = depthwise_conv1d(x, mask, [block.conv.weight], block.stride)
        else:
            x, mask = transformer_encoder(x, mask, block) if drop is None else transformer_encoder(x, mask, block, drop=drop.at(DROP_G_BRANCH, l))
        fpn.append(x)
        fpn_masks.append(mask)
    return tuple(fpn), tuple(fpn_masks)


def text_transformer(tokens, mask, text_net, drop=None):
    """TextTransformer.forward (text_net.py:158-188, the training branch) on token-major ``tokens`` (B, L, in_dim), with ``text_net`` a
    modeling.TextTransformer -> ((B, L [+ 1], TE), mask (B, L [+ 1])).  To the letter: the background token is prepended to every
    sequence and the mask is extended by its own first column (:179-182); the gradient of ``bkgd_token`` is the sum over the batch.
    The blocks are global self-attention: with L [+ 1] <= 64 positions heads of 16, 32, 64 or 128 channels, or of 8 (``xattn_mha``); longer
    texts need heads of 32 or 64 channels (``global_attention``).  ``drop``: block i is layer i of group DROP_G_TEXT, with the sites of a
    video-encoder block."""
    if not hasattr(text_net, 'bkgd_token') or not hasattr(text_net, 'transformer') or hasattr(text_net, 'attn_pool'):
        raise ValueError(f'text_transformer: {type(text_net).__name__} is not differentiable yet (TextIdentity\'s attention pool has no '
                         f'backward); a modeling.TextTransformer is required')
    B, L, _ = tokens.shape
    mask = torch.ones(B, L, dtype=torch.bool, device=tokens.device) if mask is None else _byte_mask(mask, B, L, 'text_transformer')
    x = masked_conv1d(tokens, mask, text_net.embd_fc.conv.weight, text_net.embd_fc.conv.bias)
    pe = _position_term(text_net, L, mask, 'text_transformer')
    if pe is not None:
        x = x + pe
    if text_net.bkgd_token is not None:
        x = torch.cat((text_net.bkgd_token.t()[None].expand(B, -1, -1).to(x.dtype), x), dim=1)
        mask = torch.cat((mask[:, :1], mask), dim=1)
    drop = _active(drop, 'text_transformer')
    for i, block in enumerate(text_net.transformer):
        x, _ = transformer_encoder(x, mask, block, narrow_heads=True, **_drop_kw(None if drop is None else drop.at(DROP_G_TEXT, i)))
    return x, mask
