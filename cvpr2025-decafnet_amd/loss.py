"""Point losses of the training objective on the MI355X (csrc/loss.hip) with the reference's signatures
(libs/modeling/loss.py): ``sigmoid_focal_loss`` (:5-57), ``ctr_giou_loss`` (:60-109), ``ctr_diou_loss`` (:111-166), and the
two helpers the reference's Trainer wraps them in (libs/worker_v2.py:85-91).

The reference indexes with boolean masks before calling (``logits[fpn_masks]``, ``offsets[pos_masks]``,
worker_v2.py:446-458), which compacts on the device and synchronises the host for the output size; ``select=`` takes the mask
instead and leaves everything on the device.

The label side of the objective lives here too (csrc/objective.hip): ``annotate_points_per_video`` / ``annotate_points``
(worker_v2.py:93-133, :575-637) and ``PointObjective``, the fused pass over the training forward's packed outputs that returns the
Trainer's loss dict (worker_v2.py:441-476) without materialising labels or ground-truth offsets and without a host wait.

Backward (``total_loss.backward()``, worker_v2.py:467-468), cut at the forward's outputs: when the first argument of a loss
function requires grad, the result carries a ``grad_fn`` (a ``torch.autograd.Function`` around the value kernel and
``dcf_sigmoid_focal_loss_grad`` / ``dcf_ctr_iou_loss_grad``); so do ``'cls'``, ``'reg'`` and ``'total'`` of ``PointObjective`` when
any part of ``outputs`` does (``dcf_point_objective_grad``), and ``PointObjective.grad`` is the same gradient without autograd,
for a hand-written backward of the heads.  Targets, masks and loss_norm get no gradient; nothing below the forward's outputs is
differentiated.  Without ``requires_grad`` every function returns what it always did, bit for bit.  At the non-smooth points
(``min`` / ``max`` ties, the ``clamp(min=eps)`` edge) the gradient is eager PyTorch autograd's, not the scripted reference's,
which is not a stable function there (include/decafnet_hip.h).
"""
from __future__ import annotations

import torch

from . import _lib


def _flat_f32(x, name):
    if not x.is_cuda:
        raise RuntimeError(f'{name} must live on the MI355X: the losses have no CPU path')
    return x.float().contiguous()


def _reduce(elem, total, count, reduction, shape):
    if reduction == 'none':
        return elem.view(shape)
    if reduction == 'sum':
        return total[0]
    if reduction == 'mean':
        return total[0] / count[0].to(torch.float32)
    raise ValueError(f'reduction {reduction!r}')


def _selection(select, n, device):
    """the boolean mask the kernels index with: one byte per element, on the device of the operands (no broadcasting -- the
    kernel reads select[i] for every i < n)"""
    if select is None:
        return None
    if not select.is_cuda or select.device != device:
        raise ValueError(f'select must live on {device} (got {select.device})')
    if select.numel() != n:
        raise ValueError(f'select has {select.numel()} elements, the loss has {n}')
    return select.to(torch.bool).contiguous()


def _wants_grad(x):
    return torch.is_grad_enabled() and torch.is_tensor(x) and x.requires_grad


def _upstream(grad, reduction):
    """(grad_elem, grad_scalar) of a loss function's backward: one of them None"""
    g = grad.float().contiguous()
    return (g.view(-1), None) if reduction == 'none' else (None, g.reshape(1))


def _focal_values(inputs, targets, alpha, gamma, smoothing, reduction, select):
    x, t = _flat_f32(inputs, 'inputs'), _flat_f32(targets, 'targets')
    assert x.shape == t.shape
    n = x.numel()
    lib = _lib.lib()
    sel = _selection(select, n, x.device)
    elem = torch.empty_like(x) if reduction == 'none' else None
    total = torch.zeros(1, device=x.device) if reduction != 'none' else None
    count = torch.zeros(1, device=x.device, dtype=torch.int32) if reduction == 'mean' else None
    _lib.check(lib.dcf_sigmoid_focal_loss(_lib.ptr(x), _lib.ptr(t), _lib.ptr(sel), n, float(alpha), float(gamma), int(bool(smoothing)),
                                          _lib.ptr(elem), _lib.ptr(total), _lib.ptr(count), _lib.current_stream()), 'dcf_sigmoid_focal_loss')
    return _reduce(elem, total, count, reduction, inputs.shape), (x, t, sel, count)


class _FocalFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, inputs, targets, alpha, gamma, smoothing, reduction, select):
        out, (x, t, sel, count) = _focal_values(inputs.detach(), targets.detach(), alpha, gamma, smoothing, reduction, select)
        ctx.saved = (x, t, sel, count)
        ctx.conf = (float(alpha), float(gamma), int(bool(smoothing)), reduction, inputs.shape, inputs.dtype)
        return out

    @staticmethod
    def backward(ctx, grad):
        x, t, sel, count = ctx.saved
        alpha, gamma, smoothing, reduction, shape, dtype = ctx.conf
        g_elem, g_scalar = _upstream(grad, reduction)
        g = torch.empty_like(x)
        _lib.check(_lib.lib().dcf_sigmoid_focal_loss_grad(_lib.ptr(x), _lib.ptr(t), _lib.ptr(sel), x.numel(), alpha, gamma, smoothing,
                                                          _lib.ptr(g_elem), _lib.ptr(g_scalar), _lib.ptr(count), _lib.ptr(g),
                                                          _lib.current_stream()), 'dcf_sigmoid_focal_loss_grad')
        return g.view(shape).to(dtype), None, None, None, None, None, None


def sigmoid_focal_loss(inputs, targets, alpha: float = -1, gamma: float = 2.0, smoothing: bool = True, reduction: str = 'none',
                       select=None):
    """loss.py:5-57.  ``select`` (optional bool tensor of the same shape): only these elements count ('sum' / 'mean'); with
    reduction 'none' the unselected elements are 0.  Differentiable with respect to ``inputs``."""
    if _wants_grad(inputs):
        return _FocalFn.apply(inputs, targets, alpha, gamma, smoothing, reduction, select)
    return _focal_values(inputs, targets, alpha, gamma, smoothing, reduction, select)[0]


def _ctr_iou_values(input_offsets, target_offsets, reduction, eps, kind, select):
    a, b = _flat_f32(input_offsets, 'input_offsets'), _flat_f32(target_offsets, 'target_offsets')
    assert a.shape == b.shape and a.shape[-1] == 2
    n = a.numel() // 2
    lib = _lib.lib()
    sel = _selection(select, n, a.device)
    elem = torch.empty(a.shape[:-1], device=a.device) if reduction == 'none' else None
    total = torch.zeros(1, device=a.device) if reduction != 'none' else None
    count = torch.zeros(1, device=a.device, dtype=torch.int32) if reduction == 'mean' else None
    _lib.check(lib.dcf_ctr_iou_loss(_lib.ptr(a), _lib.ptr(b), _lib.ptr(sel), n, kind, float(eps), _lib.ptr(elem), _lib.ptr(total),
                                    _lib.ptr(count), _lib.current_stream()), 'dcf_ctr_iou_loss')
    saved = (a, b, sel, count)
    if reduction == 'mean':                                              # empty selection: `0.0 * loss.sum()` (loss.py:106,163)
        if n == 0:
            return torch.zeros((), device=a.device), saved
        return torch.where(count[0] > 0, total[0] / count[0].clamp(min=1).to(torch.float32), total.new_zeros(())), saved
    return _reduce(elem, total, count, reduction, a.shape[:-1]), saved


class _CtrIouFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input_offsets, target_offsets, reduction, eps, kind, select):
        out, ctx.saved = _ctr_iou_values(input_offsets.detach(), target_offsets.detach(), reduction, eps, kind, select)
        ctx.conf = (reduction, float(eps), int(kind), input_offsets.shape, input_offsets.dtype)
        return out

    @staticmethod
    def backward(ctx, grad):
        a, b, sel, count = ctx.saved
        reduction, eps, kind, shape, dtype = ctx.conf
        g_elem, g_scalar = _upstream(grad, reduction)
        g = torch.empty_like(a)
        _lib.check(_lib.lib().dcf_ctr_iou_loss_grad(_lib.ptr(a), _lib.ptr(b), _lib.ptr(sel), a.numel() // 2, kind, eps, _lib.ptr(g_elem),
                                                    _lib.ptr(g_scalar), _lib.ptr(count), _lib.ptr(g), _lib.current_stream()),
                   'dcf_ctr_iou_loss_grad')
        return g.view(shape).to(dtype), None, None, None, None, None


def _ctr_iou(input_offsets, target_offsets, reduction, eps, kind, select):
    if _wants_grad(input_offsets):
        return _CtrIouFn.apply(input_offsets, target_offsets, reduction, eps, kind, select)
    return _ctr_iou_values(input_offsets, target_offsets, reduction, eps, kind, select)[0]


def ctr_giou_loss(input_offsets, target_offsets, reduction: str = 'none', eps: float = 1e-8, select=None):
    """loss.py:60-109 (the generalised IoU reduces to the IoU for segments sharing a centre point).  The reference asserts
    non-negative offsets on the host (loss.py:87-88); RegHead ends with a ReLU (head.py:104), targets are distances."""
    return _ctr_iou(input_offsets, target_offsets, reduction, eps, 0, select)


def ctr_diou_loss(input_offsets, target_offsets, reduction: str = 'none', eps: float = 1e-8, select=None):
    """loss.py:111-166."""
    return _ctr_iou(input_offsets, target_offsets, reduction, eps, 1, select)


def calc_focal_loss(logits, labels, smoothing=0.2, alpha=0.5, reduction='sum', select=None):
    """worker_v2.py:85-87: label smoothing, then the focal loss."""
    labels = labels.to(logits.dtype) * (1.0 - smoothing) + smoothing / 2
    return sigmoid_focal_loss(logits, labels, alpha=alpha, reduction=reduction, select=select)


def calc_iou_loss(pred_offsets, gt_offsets, reg_loss='diou', reduction='sum', select=None):
    """worker_v2.py:89-91."""
    fn = ctr_diou_loss if reg_loss == 'diou' else ctr_giou_loss
    return fn(pred_offsets, gt_offsets, reduction=reduction, select=select)


# ---------------------------------------------------------------------------------------------------------------------------
# Point annotation and the Trainer's objective (csrc/objective.hip).  The kernels derive the candidate points from their index
# in the packed pyramid layout; the point table the reference passes around is used only to recover that layout's parameters.

def _pt_gen_params(ranges, max_seq_len):
    """(regression_range, sigma, max_seq_len) that make PtGenerator.__init__ (model.py:686-696) produce `ranges`, or None"""
    ranges = [(float(a), float(b)) for a, b in ranges]
    rr = ranges[0][1]
    if ranges[0][0] != 0.0 or not rr > 0:
        return None
    sigma = ranges[1][0] / rr if len(ranges) > 1 else 1.0
    if not 0 < sigma <= 1:
        return None
    msl = int(ranges[-1][1]) - 1 if max_seq_len is None else int(max_seq_len)
    want, cur = [(0.0, rr)], rr
    for l in range(1, len(ranges)):
        lo, hi = cur * sigma, cur * 2
        if l == len(ranges) - 1:
            hi = max(hi, msl + 1)
        want.append((lo, hi))
        cur = hi
    f32 = lambda r: torch.tensor(r, dtype=torch.float64).to(torch.float32)            # noqa: E731  (the buffer's rounding)
    if not torch.equal(f32(want), f32(ranges)):
        return None
    return rr, sigma, msl


def _point_layout(points):
    """T, L, (regression_range, sigma, max_seq_len), use_offset of a PtGenerator point table (a tuple of levels or their cat);
    ValueError when the table is anything else"""
    def bad(why):
        return ValueError(f'points is not a PtGenerator table ({why}): the kernels derive the candidate points from their index')

    if isinstance(points, (tuple, list)):
        levels = [p.detach().cpu().float() for p in points]
    else:
        p = points.detach().cpu().float()
        if p.dim() != 2 or p.size(-1) != 4 or p.size(0) == 0:
            raise bad(f'shape {tuple(p.shape)}')
        stride = p[:, 3]
        cuts = (torch.nonzero(stride[1:] != stride[:-1]).flatten() + 1).tolist()
        levels = list(torch.tensor_split(p, cuts))
    L = len(levels)
    if L < 1 or L > 16 or any(lv.dim() != 2 or lv.size(-1) != 4 for lv in levels):
        raise bad('levels')
    T = levels[0].size(0)
    if T == 0 or T % (1 << (L - 1)) or any(lv.size(0) != T >> l for l, lv in enumerate(levels)):
        raise bad('level lengths are not T >> l')
    use_offset = bool(levels[0][0, 0] == 0.5)
    ranges = []
    for l, lv in enumerate(levels):
        s = float(1 << l)
        x = torch.arange(lv.size(0), dtype=torch.float32) * s + (s - 0.5 if use_offset else 0.0)       # model.py:710-712, see PtGenerator
        if not (torch.equal(lv[:, 0], x) and bool((lv[:, 3] == s).all()) and bool((lv[:, 1:3] == lv[0, 1:3]).all())):
            raise bad(f'level {l}')
        ranges.append((float(lv[0, 1]), float(lv[0, 2])))
    params = _pt_gen_params(ranges, None)
    if params is None or params[2] < T:
        raise bad('regression ranges')
    return T, L, params, use_offset


def _annotate(targets, T, L, params, use_offset, center_sampling, center_sampling_radius, predicates):
    if not targets.is_cuda:
        raise RuntimeError('targets must live on the MI355X: the annotation has no CPU path')
    tg = targets.float().reshape(-1, 2).contiguous()
    n, S = tg.size(0), sum(T >> l for l in range(L))
    labels = torch.empty(n, S, dtype=torch.bool, device=tg.device)
    offsets = torch.empty(n, S, 2, dtype=torch.float32, device=tg.device)
    win = torch.empty_like(labels) if predicates else None
    rng = torch.empty_like(labels) if predicates else None
    rr, sigma, msl = params
    _lib.check(_lib.lib().dcf_annotate_points(_lib.ptr(tg), n, T, L, rr, sigma, int(use_offset), msl, int(center_sampling == 'radius'),
                                              float(center_sampling_radius), _lib.ptr(labels), _lib.ptr(offsets), _lib.ptr(win), _lib.ptr(rng),
                                              _lib.current_stream()), 'dcf_annotate_points')
    return labels, offsets, win, rng


def annotate_points_per_video(points, target, center_sampling='radius', center_sampling_radius=1.5):
    """worker_v2.py:93-133: (labels (p,), offsets (p, 2), [inside_window, inside_range]) of one target segment."""
    T, L, params, use_offset = _point_layout(points)
    labels, offsets, win, rng = _annotate(target.reshape(1, 2), T, L, params, use_offset, center_sampling, center_sampling_radius, True)
    return labels[0], offsets[0], [win[0], rng[0]]


def annotate_points(points, targets, center_sampling='radius', center_sampling_radius=1.5):
    """Trainer._annotate_points (worker_v2.py:575-637): labels (bs, p) bool and offsets (bs, p, 2) of every target, one launch."""
    T, L, params, use_offset = _point_layout(points)
    labels, offsets, _, _ = _annotate(targets, T, L, params, use_offset, center_sampling, center_sampling_radius, False)
    return labels, offsets


def _packed(parts):
    """the (B', S[, 2]) tensor whose level split `parts` is: the storage the training forward filled when the parts are its
    `split` views (modeling.py), a `cat` otherwise"""
    if torch.is_tensor(parts):
        return parts.contiguous()
    base = parts[0]._base
    if base is not None and base.is_contiguous() and base.dim() == parts[0].dim():
        off, ok = 0, True
        for p in parts:
            ok = ok and p._base is base and p.stride() == base.stride() and p.size(0) == base.size(0)
            ok = ok and p.storage_offset() == base.storage_offset() + off * base.stride(1)
            off += p.size(1)
        if ok and off == base.size(1):
            return base
    return torch.cat(tuple(parts), 1).contiguous()


def _objective_operands(outputs, targets, pack=None):
    """(l1 or None, l2, off, msk, tg, T, L) of the level tuples a forward returns, packed to (B', S[, 2])"""
    pack = pack or _packed
    if len(outputs) == 4:
        l1, l2, off = (pack(p) for p in outputs[:3])
    elif len(outputs) == 3:
        l1, (l2, off) = None, (pack(p) for p in outputs[:2])
    else:
        raise ValueError('outputs: the 4 (or, for the classes with one classification head, 3) parts the training forward returns')
    msk = _packed(outputs[-1])
    if torch.is_tensor(outputs[-1]):
        raise ValueError('outputs must be per-level tuples (the level lengths define the point layout)')
    if not (l2.is_cuda and targets.is_cuda):
        raise RuntimeError('the objective runs on the MI355X: outputs and targets must live there')
    n, S = l2.shape
    sizes = [p.size(1) for p in outputs[-1]]
    T, L = sizes[0], len(sizes)
    if sizes != [T >> l for l in range(L)] or T % (1 << (L - 1)):
        raise ValueError(f'level lengths {sizes} are not a pyramid T >> l')
    tg = targets.detach().float().reshape(-1, 2).contiguous()
    assert tg.size(0) == n and off.shape == (n, S, 2) and msk.shape == (n, S) and msk.dtype == torch.bool
    assert l2.dtype == torch.float32 and off.dtype == torch.float32 and (l1 is None or (l1.dtype == torch.float32 and l1.shape == l2.shape))
    return l1, l2, off, msk, tg, T, L


def _objective_packed(l1, l2, off, msk, tg, T, L, pt_params, use_offset, center_sampling, radius, alpha, smoothing, reg_loss, norm32, world_size,
                      loss_weight):
    n = l2.size(0)
    rows = torch.empty(n, 4, dtype=torch.float32, device=l2.device)
    out4 = torch.empty(4, dtype=torch.float32, device=l2.device) if norm32 is not None else None
    rr, sigma, msl = pt_params
    _lib.check(_lib.lib().dcf_point_objective(
        _lib.ptr(l1), _lib.ptr(l2), _lib.ptr(off), _lib.ptr(msk), _lib.ptr(tg), n, T, L, rr, sigma, int(use_offset), msl,
        int(center_sampling == 'radius'), float(radius), float(alpha), float(smoothing), int(reg_loss == 'diou'), 1e-8,
        _lib.ptr(norm32), float(world_size), float(loss_weight), _lib.ptr(rows), _lib.ptr(out4),
        _lib.current_stream()), 'dcf_point_objective')
    return rows, out4


def _objective(outputs, targets, pt_params, use_offset, center_sampling, radius, alpha, smoothing, reg_loss, norm_of, world_size, loss_weight):
    """dcf_point_objective on the level tuples a forward returns: (rows (B', 4), out4 or None when ``norm_of`` is None)"""
    l1, l2, off, msk, tg, T, L = _objective_operands(outputs, targets)
    return _objective_packed(l1, l2, off, msk, tg, T, L, pt_params, use_offset, center_sampling, radius, alpha, smoothing, reg_loss,
                             norm_of(l2.device) if norm_of is not None else None, world_size, loss_weight)


def _objective_grad_packed(l1, l2, off, msk, tg, T, L, pt_params, use_offset, center_sampling, radius, alpha, smoothing, reg_loss, norm32,
                           world_size, loss_weight, grad_total, grad_parts, out, accumulate):
    """dcf_point_objective_grad into ``out`` = (g1 or None, g2, goff), packed and contiguous"""
    g1, g2, go = out
    rr, sigma, msl = pt_params
    _lib.check(_lib.lib().dcf_point_objective_grad(
        _lib.ptr(l1), _lib.ptr(l2), _lib.ptr(off), _lib.ptr(msk), _lib.ptr(tg), l2.size(0), T, L, rr, sigma, int(use_offset), msl,
        int(center_sampling == 'radius'), float(radius), float(alpha), float(smoothing), int(reg_loss == 'diou'), 1e-8,
        _lib.ptr(norm32), float(world_size), float(loss_weight), _lib.ptr(grad_total), _lib.ptr(grad_parts), _lib.ptr(g1), _lib.ptr(g2),
        _lib.ptr(go), int(bool(accumulate)), None, None, _lib.current_stream()), 'dcf_point_objective_grad')
    return out


def _packed_for_autograd(parts):
    """_packed for parts that take part in autograd: the packed base when the parts are its views and it requires grad itself
    (the gradient then arrives at it directly), a differentiable cat otherwise"""
    x = _packed(parts)
    if not torch.is_tensor(parts) and x is parts[0]._base and not x.requires_grad and any(p.requires_grad for p in parts):
        x = torch.cat(tuple(parts), 1)
    return x


class _ObjectiveFn(torch.autograd.Function):
    """out4 = (cls, reg, total, norm) of dcf_point_objective with dcf_point_objective_grad as its backward; the upstream gradient
    of out4 is read on the device (total: element 2; cls, reg: elements 0, 1)"""

    @staticmethod
    def forward(ctx, obj, tg, msk, T, L, l2, off, l1):
        norm32 = obj._norm(l2.device)
        args = (l1.detach().contiguous() if l1 is not None else None, l2.detach().contiguous(), off.detach().contiguous(), msk, tg, T, L,
                obj.pt_params, obj.use_offset, obj.center_sampling, obj.center_sampling_radius, obj.fc_a, obj.fc_s, obj.reg_loss, norm32,
                obj.world_size, obj.loss_weight)
        rows, out4 = _objective_packed(*args)
        ctx.args = args                  # norm32 is the tensor of this step: update_norm replaces it, never writes into it
        ctx.mark_non_differentiable(rows)
        return out4, rows

    @staticmethod
    def backward(ctx, g4, _rows):
        l1, l2, off = ctx.args[:3]
        g4 = g4.float().contiguous()
        out = (torch.empty_like(l1) if l1 is not None else None, torch.empty_like(l2), torch.empty_like(off))
        _objective_grad_packed(*ctx.args, g4[2:3], g4[0:2], out, False)
        return None, None, None, None, None, out[1], out[2], out[0]


def pt_gen_params(opt, pt_gen=None):
    """((regression_range, sigma, max_seq_len), use_offset) of a PtGenerator, or of the one ``opt`` describes"""
    if pt_gen is not None:
        params = _pt_gen_params(pt_gen.regression_range, pt_gen.max_seq_len)
        if params is None:
            raise ValueError('pt_gen.regression_range is not what PtGenerator.__init__ derives')
        return params, bool(pt_gen.use_offset)
    pg = opt['pt_gen']
    return ((float(pg['regression_range']), float(pg['sigma']), int(pg.get('max_seq_len') or opt['model']['vid_net']['max_seq_len'])),
            bool(pg.get('use_offset', False)))


class PointObjective:
    """What Trainer._microbatch_forward_backward does after the model call (worker_v2.py:428-476) as one fused pass over the training forward's packed outputs: point annotation, pos = labels & masks, the focal losses of both
    heads on the valid points, the DIoU / GIoU loss on the positive points, the division by the running loss_norm, the
    world-size factor and total = cls + loss_weight * reg.  Nothing waits on the host: loss_norm lives on the device.

    ``opt.train`` supplies center_sampling, center_sampling_radius, loss_norm, loss_norm_momentum, loss_weight, reg_loss and
    ``opt.loss`` fc_a, fc_s; the point layout comes from ``pt_gen`` (a PtGenerator) or from ``opt.pt_gen`` and the video
    network's max_seq_len."""

    def __init__(self, opt, pt_gen=None, world_size=1):
        tr, ls = opt['train'], opt['loss']
        self.center_sampling = tr.get('center_sampling', 'radius')
        self.center_sampling_radius = float(tr['center_sampling_radius'])
        self.loss_norm_momentum = float(tr['loss_norm_momentum'])
        self.loss_weight = float(tr['loss_weight'])
        self.reg_loss = tr['reg_loss']
        self.fc_a, self.fc_s = float(ls['fc_a']), float(ls['fc_s'])
        self.world_size = int(world_size)
        self.pt_params, self.use_offset = pt_gen_params(opt, pt_gen)
        self._loss_norm0 = float(tr['loss_norm'])
        self._norm64 = None              # the running norm in fp64 on the device (the reference keeps a Python float)
        self._norm32 = None              # ... and the fp32 copy the kernel reads
        self.per_row = None

    def _norm(self, device):
        if self._norm64 is None or self._norm64.device != device:
            if self._norm64 is None:
                self._norm64 = torch.full((1,), self._loss_norm0, dtype=torch.float64, device=device)
            else:
                self._norm64 = self._norm64.to(device)
            self._norm32 = self._norm64.to(torch.float32)
        return self._norm32

    @property
    def loss_norm(self):
        """the running normaliser (a host read: for logging and checkpoints, not for the step)"""
        return self._loss_norm0 if self._norm64 is None else float(self._norm64)

    @loss_norm.setter
    def loss_norm(self, v):
        self._loss_norm0, self._norm64, self._norm32 = float(v), None, None

    def update_norm(self, norm_sum):
        """worker_v2.py:381-382: loss_norm = m * loss_norm + (1 - m) * max(sum of the ranks' norms, 1).  ``norm_sum``: the
        (all-gathered and summed) norm of the step, a device tensor (no host wait) or a number."""
        m = self.loss_norm_momentum
        if torch.is_tensor(norm_sum) and norm_sum.is_cuda:
            self._norm(norm_sum.device)
            self._norm64 = m * self._norm64 + (1. - m) * norm_sum.to(torch.float64).reshape(1).clamp(min=1)
            self._norm32 = self._norm64.to(torch.float32)
        else:
            self.loss_norm = m * self.loss_norm + (1. - m) * max(float(norm_sum), 1)
        return self

    def __call__(self, outputs, targets):
        parts = [p for o in outputs[:-1] for p in ((o,) if torch.is_tensor(o) else o)]
        if torch.is_grad_enabled() and any(p.requires_grad for p in parts):
            l1, l2, off, msk, tg, T, L = _objective_operands(outputs, targets, _packed_for_autograd)
            out4, rows = _ObjectiveFn.apply(self, tg, msk, T, L, l2, off, l1)
        else:
            rows, out4 = _objective(outputs, targets, self.pt_params, self.use_offset, self.center_sampling, self.center_sampling_radius, self.fc_a,
                                    self.fc_s, self.reg_loss, self._norm, self.world_size, self.loss_weight)
        self.per_row = rows
        return {'cls': out4[0], 'reg': out4[1], 'total': out4[2], 'norm': out4[3].detach().to(torch.int64)}

    def grad(self, outputs, targets, grad_total=None, out=None, accumulate=False):
        """d total / d (fpn_logits1, fpn_logits2, fpn_offsets) (two for the single-head classes) times ``grad_total`` (a number
        or a one-element device tensor; None = 1), each split into level views like the forward's outputs: what
        ``self(outputs, targets)['total'].backward()`` leaves in the leaves, without autograd, for a hand-written backward of the
        heads.  ``out``: what an earlier call returned (or the packed buffers), to write into; ``accumulate`` adds to it instead
        (micro-batches, worker_v2.py:366-376).  No host wait."""
        with torch.no_grad():
            l1, l2, off, msk, tg, T, L = _objective_operands(outputs, targets)
        sizes = [T >> l for l in range(L)]
        if out is None:
            if accumulate:
                raise ValueError('accumulate=True needs the buffers to add into (out=)')
            out = [torch.empty_like(x) for x in ((l1, l2, off) if l1 is not None else (l2, off))]
        else:
            want = [x.shape for x in ((l1, l2, off) if l1 is not None else (l2, off))]
            packed = [o if torch.is_tensor(o) else _packed(o) for o in out]
            if any(not torch.is_tensor(o) and q.data_ptr() != o[0].data_ptr() for o, q in zip(out, packed)):
                raise ValueError('out: level tuples must be the split views of one packed buffer (as grad returns them)')
            out = packed
            if [o.shape for o in out] != want or any(o.dtype != torch.float32 or not o.is_contiguous() or o.device != l2.device for o in out):
                raise ValueError(f'out: {len(want)} packed fp32 buffers of shapes {[tuple(w) for w in want]} on {l2.device}, or their level views')
        if grad_total is not None:
            if torch.is_tensor(grad_total):
                grad_total = grad_total.detach().to(device=l2.device, dtype=torch.float32).reshape(1)
            else:
                grad_total = torch.full((1,), float(grad_total), dtype=torch.float32, device=l2.device)
        bufs = ([None] if l1 is None else []) + list(out)
        _objective_grad_packed(l1, l2, off, msk, tg, T, L, self.pt_params, self.use_offset, self.center_sampling, self.center_sampling_radius,
                               self.fc_a, self.fc_s, self.reg_loss, self._norm(l2.device), self.world_size, self.loss_weight, grad_total, None,
                               bufs, accumulate)
        return tuple(o.split(sizes, 1) for o in out)
