"""The gradient of the point losses and of the Trainer's objective written out in closed form, in fp64 torch (no autograd): what
csrc/loss_elem.h (focal_grad_elem, iou_grad_elem) and the gradient side of csrc/objective.hip are checked against, next to the
reference's own autograd results in tests/golden/objective_grad.npz.  Convention at the non-smooth points: eager PyTorch
autograd -- min / max hand each argument half the gradient at a tie, clamp(min=eps) passes it where x >= eps."""
import numpy as np
import torch

F64 = torch.float64


# ------------------------------------------------------------------------------------------------------------------ focal loss
def focal_value(x, t, alpha=-1.0, gamma=2.0, smoothing=True, dt=F64):
    """``dt=torch.float32``: the same expression under fp32 autograd, the yardstick's own rounding error where the fixture holds none"""
    x, t = x.to(dt), t.to(dt)
    pos = (t >= 0.5).to(dt)
    s = t if smoothing else pos
    p = torch.sigmoid(x)
    ce = (1 - t) * x + torch.nn.functional.softplus(-x)
    loss = ce * (1 - (p * s + (1 - p) * (1 - s))) ** gamma
    if alpha >= 0:
        loss = (alpha * pos + (1 - alpha) * (1 - pos)) * loss
    return loss


def focal_grad(x, t, alpha=-1.0, gamma=2.0, smoothing=True):
    """d focal_value / d x, elementwise"""
    x, t = x.to(F64), t.to(F64)
    pos = (t >= 0.5).to(F64)
    s = t if smoothing else pos
    p, q = torch.sigmoid(x), torch.sigmoid(-x)                       # q = 1 - p without cancellation
    m = p * (1 - s) + q * s                                          # 1 - p_t
    ce = (1 - t) * x + torch.nn.functional.softplus(-x)
    g = (p - t) * m ** gamma - ce * gamma * m ** (gamma - 1) * (p * q * (2 * s - 1))
    if alpha >= 0:
        g = (alpha * pos + (1 - alpha) * (1 - pos)) * g
    return g


# ------------------------------------------------------------------------------------------------------------------- IoU losses
def iou_value(pred, gt, kind, eps=1e-8, dt=F64):
    """kind 'giou' (which is the IoU here) or 'diou'; pred, gt (..., 2)"""
    pred, gt = pred.to(dt), gt.to(dt)
    lp, rp, lg, rg = pred[..., 0], pred[..., 1], gt[..., 0], gt[..., 1]
    inter = torch.minimum(lp, lg) + torch.minimum(rp, rg)
    union = (lp + rp) + (lg + rg) - inter
    loss = 1 - inter / union.clamp(min=eps)
    if kind == 'diou':
        hull = torch.maximum(lp, lg) + torch.maximum(rp, rg)
        loss = loss + (0.5 * (rp - lp - rg + lg) / hull.clamp(min=eps)) ** 2
    return loss


def _half_at_tie(a, b):
    """d min(a, b) / d a"""
    return (a < b).to(F64) + 0.5 * (a == b).to(F64)


def iou_grad(pred, gt, kind, eps=1e-8):
    """d iou_value / d pred, (..., 2)"""
    pred, gt = pred.to(F64), gt.to(F64)
    lp, rp, lg, rg = pred[..., 0], pred[..., 1], gt[..., 0], gt[..., 1]
    inter = torch.minimum(lp, lg) + torch.minimum(rp, rg)
    union = (lp + rp) + (lg + rg) - inter
    uc = union.clamp(min=eps)
    u_open = (union >= eps).to(F64)
    out = []
    for side, (a, b) in enumerate(((lp, lg), (rp, rg))):
        d_inter = _half_at_tie(a, b)
        d_union = (1 - d_inter) * u_open
        g = -(d_inter / uc - inter / uc ** 2 * d_union)
        if kind == 'diou':
            hull = torch.maximum(lp, lg) + torch.maximum(rp, rg)
            hc = hull.clamp(min=eps)
            rho = 0.5 * (rp - lp - rg + lg)
            d_rho = -0.5 if side == 0 else 0.5
            d_hull = (1 - d_inter) * (hull >= eps).to(F64)           # d max(a, b) / d a = 1 - d min(a, b) / d a
            g = g + 2 * (rho / hc) * (d_rho / hc - rho / hc ** 2 * d_hull)
        out.append(g)
    return torch.stack(out, -1)


def non_smooth(pred, gt, eps=1e-8):
    """elements where the gradient depends on the sub-gradient convention: a tie, or union / hull under eps"""
    pred, gt = pred.to(F64), gt.to(F64)
    lp, rp, lg, rg = pred[..., 0], pred[..., 1], gt[..., 0], gt[..., 1]
    union = (lp + rp) + (lg + rg) - (torch.minimum(lp, lg) + torch.minimum(rp, rg))
    hull = torch.maximum(lp, lg) + torch.maximum(rp, rg)
    return (lp == lg) | (rp == rg) | (union < eps) | (hull < eps)


# -------------------------------------------------------------------------------------------------------------- the point rule
def annotate(T, L, max_seq_len, regression_range, sigma, targets, mode, radius, use_offset=False):
    """labels (n, S) bool and ground-truth offsets (n, S, 2) fp32 of PtGenerator's points, in numpy fp32 so that the comparisons
    fall as the reference's do (worker_v2.py:93-133, model.py:686-723)"""
    f = np.float32
    ranges, cur = [(0, regression_range)], regression_range
    for l in range(1, L):
        lo, hi = cur * sigma, cur * 2
        if l == L - 1:
            hi = max(hi, max_seq_len + 1)
        ranges.append((lo, hi))
        cur = hi
    labels, offsets = [], []
    for t0, t1 in np.asarray(targets, dtype=np.float32):
        lab, off = [], []
        for l in range(L):
            s = f(2 ** l)
            x = np.arange(T >> l, dtype=np.float32) * s + (s - f(0.5) if use_offset else f(0))
            a, b = x - t0, t1 - x
            if mode == 'radius':
                c, r = f(0.5) * (t0 + t1), s * f(radius)
                win = (x - np.maximum(c - r, t0) > 0) & (np.minimum(c + r, t1) - x > 0)
            else:
                win = (a > 0) & (b > 0)
            d = np.maximum(a, b)
            lab.append(win & (d >= f(ranges[l][0])) & (d < f(ranges[l][1])))
            off.append(np.stack([a / s, b / s], -1))
        labels.append(np.concatenate(lab)), offsets.append(np.concatenate(off))
    return torch.from_numpy(np.stack(labels)), torch.from_numpy(np.stack(offsets))


# --------------------------------------------------------------------------------------------------------------- the objective
def objective_value(l1, l2, off, msk, labels, gt, reg_loss, loss_norm, world_size, loss_weight, alpha=0.5, smoothing=0.2, dt=F64):
    """total of worker_v2.py:441-465 in fp64 (or ``dt``); l1 None: one classification head"""
    t = labels.to(dt) * (1.0 - smoothing) + smoothing / 2
    pos = labels & msk
    heads = [l2] if l1 is None else [l1, l2]
    cls = sum((focal_value(x, t, alpha, 2.0, True, dt) * msk).sum() / loss_norm * world_size for x in heads) / len(heads)
    reg = (iou_value(off, gt, reg_loss, dt=dt) * pos).sum() / loss_norm * world_size
    return cls + loss_weight * reg


def objective_grad(l1, l2, off, msk, labels, gt, reg_loss, loss_norm, world_size, loss_weight, alpha=0.5, smoothing=0.2, grad_total=1.0):
    """d total / d (l1, l2, off) in fp64 (g1 None with l1): focal' * world_size / loss_norm / n_heads on masks, loss_weight * iou' *
    world_size / loss_norm on labels & masks, exactly 0 elsewhere"""
    t = labels.to(F64) * (1.0 - smoothing) + smoothing / 2
    pos = (labels & msk)
    n_heads = 1 if l1 is None else 2
    k = float(world_size) / float(loss_norm) * float(grad_total)
    zero = torch.zeros((), dtype=F64)
    g = [None if x is None else torch.where(msk, focal_grad(x, t, alpha, 2.0, True) * (k / n_heads), zero) for x in (l1, l2)]
    go = torch.where(pos[..., None], iou_grad(off, gt, reg_loss) * (k * float(loss_weight)), zero)
    return g[0], g[1], go


def autograd_objective_grad(l1, l2, off, msk, labels, gt, reg_loss, loss_norm, world_size, loss_weight, alpha=0.5, smoothing=0.2, dt=F64):
    """the same gradient from autograd through objective_value in ``dt`` (on the CPU)"""
    leaves = [None if x is None else x.detach().to(dt).clone().requires_grad_(True) for x in (l1, l2, off)]
    objective_value(*leaves, msk, labels, gt.to(dt), reg_loss, loss_norm, world_size, loss_weight, alpha, smoothing, dt).backward()
    return tuple(None if x is None else x.grad for x in leaves)
