"""Generate tests/golden/objective_grad.npz: `total.backward()` of the Trainer's objective and the gradients of the point losses
from the reference's own functions (calc_focal_loss, calc_iou_loss, annotate_points_per_video of libs/worker_v2.py; the scripted
sigmoid_focal_loss, ctr_giou_loss, ctr_diou_loss of libs/modeling/loss.py), combined as make_golden_objective.py::trainer combines
them, next to the gradient of the same expression in fp64 (autograd through tests/objective_grad_ref.py's values).

Run where the reference is importable (not on the GPU machine):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_objective_grad.py

Cases: tests/objective_cases.py (the batches a, b, z, both modes, GRID, the single-head `late` case, bench scale) and
tests/objective_grad_cases.py (the loss-function grid, the non-smooth pairs).  The scripted functions are called several times
per case: two warm-up calls, then four that must give the same gradient, which is the one recorded.  Elements at a tie or with
union / hull under eps are left out of the comparison with the scripted reference (its gradient is not a stable function there); the generator asserts that they are at
most 1 % of the positive points of each case and prints the counts.  The constructed non-smooth pairs get their expected values
from the reference's functions with scripting disabled (PYTORCH_JIT=0, in a child process).

Bench scale is stored sparsely: the gradient at every labelled point and its neighbours and at a fixed stride through the rest,
plus per row and level the fp64 sum and sum of absolute values.  The logits' gradient does not depend on loss_weight, so it is
stored once per (loss_norm, world_size) after asserting that the reference agrees bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402
import objective_cases as C  # noqa: E402
import objective_grad_cases as G  # noqa: E402
import objective_grad_ref as R  # noqa: E402

REPEATS = 4
WARMUP = 2
BENCH_STRIDE = 61


def ties_child():
    """PYTORCH_JIT=0: the reference's loss functions as plain Python, eager autograd"""
    assert os.environ.get('PYTORCH_JIT') == '0'
    MG.install_stubs()
    from libs.modeling.loss import ctr_diou_loss, ctr_giou_loss
    out = {}
    for kind, fn in (('giou', ctr_giou_loss), ('diou', ctr_diou_loss)):
        rows = []
        for p, g in zip(G.TIE_PRED, G.TIE_GT):                     # one pair per call: no element sees another's history
            pred = torch.tensor([p], requires_grad=True)
            fn(pred, torch.tensor([g]), reduction='sum').backward()
            rows.append(pred.grad[0].tolist())
        out[kind] = rows
    print('TIES ' + json.dumps(out))


def repeated(run):
    """run() -> tuple of gradients.  The first call of a scripted function on a new kind of input runs its profiling pass, whose
    gradient can differ from all later calls in the last bit even at smooth points (measured: 1.5e-8 on values of 0.3); it is
    reported and not recorded.  Recorded is the gradient of the calls after the warm-up, REPEATS of them, all equal."""
    warm = [run() for _ in range(WARMUP)]
    first = run()
    for _ in range(REPEATS - 1):
        again = run()
        assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(first, again)), 'the scripted gradient changed between calls'
    drift = max(float((a - b).abs().max()) for w in warm for a, b in zip(w, first) if a is not None and a.numel())
    if drift > 0:
        print(f'    warm-up calls differ from the recorded gradient by up to {drift:.3e}')
    return first


def main():
    MG.install_stubs()
    from libs.modeling.loss import ctr_diou_loss, ctr_giou_loss, sigmoid_focal_loss
    from libs.modeling.model import PtGenerator
    from libs.worker_v2 import annotate_points_per_video, calc_focal_loss, calc_iou_loss

    def annotate(points, targets, mode):
        ls, os_ = [], []
        for t in targets:
            l, o, _ = annotate_points_per_video(points, t, center_sampling=mode, center_sampling_radius=C.RADIUS)
            ls.append(l), os_.append(o)
        return torch.stack(ls), torch.stack(os_)

    def trainer_total(l1, l2, off, msk, labels, gt_off, reg_loss, loss_norm, ws, lw):
        """make_golden_objective.py::trainer, the total only"""
        pos = torch.logical_and(labels, msk)
        cls2 = calc_focal_loss(logits=l2[msk], labels=labels[msk], alpha=C.FC_A, smoothing=C.FC_S) / loss_norm * ws
        if l1 is not None:
            cls1 = calc_focal_loss(logits=l1[msk], labels=labels[msk], alpha=C.FC_A, smoothing=C.FC_S) / loss_norm * ws
            cls = (cls1 + cls2) / 2
        else:
            cls = cls2
        reg = calc_iou_loss(pred_offsets=off[pos], gt_offsets=gt_off[pos], reg_loss=reg_loss) / loss_norm * ws
        return cls + lw * reg

    def ref32(l1, l2, off, msk, labels, gt_off, reg_loss, ln, ws, lw):
        def run():
            leaves = [None if x is None else x.clone().requires_grad_(True) for x in (l1, l2, off)]
            trainer_total(*leaves, msk, labels, gt_off, reg_loss, ln, ws, lw).backward()
            return tuple(None if x is None else x.grad for x in leaves)
        return repeated(run)

    def ref64(l1, l2, off, msk, labels, gt_off, reg_loss, ln, ws, lw):
        leaves = [None if x is None else x.double().requires_grad_(True) for x in (l1, l2, off)]
        R.objective_value(*leaves, msk, labels, gt_off.double(), reg_loss, ln, ws, lw, C.FC_A, C.FC_S).backward()
        return tuple(None if x is None else x.grad for x in leaves)

    def excluded(off, gt_off, pos, name, allow_empty=False):
        """the non-smooth positive points of a case; the condition of the fixture"""
        ns = R.non_smooth(off, gt_off) & pos
        n_pos, n_ex = int(pos.sum()), int(ns.sum())
        print(f'{name}: {n_pos} positive points, {n_ex} excluded')
        assert n_ex <= 0.01 * n_pos and (n_pos - n_ex >= 1 or allow_empty), name
        return ns

    out = {}
    # ------------------------------------------------------------------ small
    g = np.load(os.path.join(HERE, 'train.npz'))
    L = C.SMALL['L']
    cat = lambda n, z=g, p='': torch.cat([torch.from_numpy(z[f'{p}{n}/l{l}']) for l in range(L)], 1)      # noqa: E731
    l1, l2, off, msk = cat('logits1'), cat('logits2'), cat('offsets'), cat('masks')
    sec = np.load(os.path.join(HERE, 'train_secondary.npz'))
    sl, so, sm = cat('logits', sec, 'late/'), cat('offsets', sec, 'late/'), cat('masks', sec, 'late/')
    pg = PtGenerator(C.SMALL['max_seq_len'], L, C.SMALL['regression_range'], C.SMALL['sigma'], use_offset=False)
    points = torch.cat(pg(C.level_sizes(C.SMALL['T'], L)))
    for bn, (tg, rows) in C.SMALL_BATCHES.items():
        tg = torch.tensor(tg, dtype=torch.float32)
        a1, a2, ao, am = l1[rows], l2[rows], off[rows], msk[rows]
        for mode, (cs, reg_loss) in C.MODES.items():
            labels, gt_off = annotate(points, tg, cs)
            k = f'small/{bn}/{mode}'
            out[f'{k}/excluded'] = excluded(ao, gt_off, labels & am, k, allow_empty=bn == 'z')
            seen = {}
            for i, (ln, ws, lw) in enumerate(C.GRID):
                g1, g2, go = ref32(a1, a2, ao, am, labels, gt_off, reg_loss, ln, ws, lw)
                if (ln, ws) in seen:                                   # the logits' gradient does not see loss_weight
                    assert torch.equal(g1, seen[(ln, ws)][0]) and torch.equal(g2, seen[(ln, ws)][1])
                else:
                    seen[(ln, ws)] = (g1, g2)
                    out[f'{k}/ln{ln}_ws{ws}/g1_32'], out[f'{k}/ln{ln}_ws{ws}/g2_32'] = g1, g2
                out[f'{k}/{i}/go_32'] = go
                if i == 0:                                             # fp64: GRID[0]; the rest is this times a ratio of the grid's numbers
                    out[f'{k}/g1_64'], out[f'{k}/g2_64'], out[f'{k}/go_64'] = ref64(a1, a2, ao, am, labels, gt_off, reg_loss, ln, ws, lw)
            if bn == 'a' and mode == 'radius':                         # single-head form
                out['small/late/excluded'] = excluded(so, gt_off, labels & sm, 'small/late')
                _, out['small/late/g2_32'], out['small/late/go_32'] = ref32(None, sl, so, sm, labels, gt_off, reg_loss, 160.0, 1, 1.0)
                _, out['small/late/g2_64'], out['small/late/go_64'] = ref64(None, sl, so, sm, labels, gt_off, reg_loss, 160.0, 1, 1.0)

    # ------------------------------------------------------------------ bench scale
    T, L = C.BENCH['T'], C.BENCH['L']
    b1, b2, bo, bm, tg = C.bench_inputs()
    pg = PtGenerator(C.BENCH['max_seq_len'], L, C.BENCH['regression_range'], C.BENCH['sigma'], use_offset=False)
    points = torch.cat(pg(C.level_sizes(T, L)))
    S = points.size(0)
    lv = np.cumsum([0] + C.level_sizes(T, L))
    for mode, (cs, reg_loss) in C.MODES.items():
        labels, gt_off = annotate(points, tg, cs)
        k = f'bench/{mode}'
        out[f'{k}/excluded_idx'] = torch.nonzero(excluded(bo, gt_off, labels & bm, k))
        keep = torch.zeros(len(tg), S, dtype=torch.bool)
        keep[:, ::BENCH_STRIDE] = True
        for d in (-1, 0, 1):
            r, c = torch.nonzero(labels, as_tuple=True)
            keep[r, (c + d).clamp(0, S - 1)] = True
        idx = torch.nonzero(keep)
        out[f'{k}/idx'] = idx.to(torch.int32)
        g32 = ref32(b1, b2, bo, bm, labels, gt_off, reg_loss, 160.0, 1, 1.0)
        g64 = ref64(b1, b2, bo, bm, labels, gt_off, reg_loss, 160.0, 1, 1.0)
        for name, a, b in zip(('g1', 'g2', 'go'), g32, g64):
            out[f'{k}/{name}_32'], out[f'{k}/{name}_64'] = a[idx[:, 0], idx[:, 1]], b[idx[:, 0], idx[:, 1]]
            b = b.reshape(len(tg), S, -1)
            out[f'{k}/{name}_sum64'] = torch.stack([torch.stack([b[r, lv[l]:lv[l + 1]].sum() for l in range(L)]) for r in range(len(tg))])
            out[f'{k}/{name}_abs64'] = torch.stack([torch.stack([b[r, lv[l]:lv[l + 1]].abs().sum() for l in range(L)]) for r in range(len(tg))])
            full = (a.double() - b.reshape(a.shape)).abs().max()
            print(f'{k} {name}: max |g64| {float(b.abs().max()):.3e}, reference max |g32 - g64| {float(full):.3e} over all points, '
                  f'{float((out[f"{k}/{name}_32"].double() - out[f"{k}/{name}_64"]).abs().max()):.3e} over the {idx.size(0)} stored')
            out[f'{k}/{name}_eref_all'] = full
        out[f'{k}/valid_per_level'] = torch.stack([torch.stack([bm[r, lv[l]:lv[l + 1]].sum() for l in range(L)]) for r in range(len(tg))])

    # ------------------------------------------------------------------ the loss functions on their own
    x, t, pred, gt, sel, up = G.loss_inputs()
    assert not bool(R.non_smooth(pred, gt).any())

    def one(fn64, fn32, a, b, reduction, select, width):
        """gradient w.r.t. `a` of the reduced loss: the reference on the selected elements (fp32), the restated values (fp64)"""
        res = []
        for fn, dt in ((fn32, torch.float32), (fn64, torch.float64)):
            def run():
                leaf = a.to(dt).clone().requires_grad_(True)
                aa, bb, uu = (leaf[sel], b.to(dt)[sel], up.to(dt)[sel]) if select else (leaf, b.to(dt), up.to(dt))
                if fn is fn64:
                    loss = fn(aa, bb)
                    loss = loss if reduction == 'none' else (loss.sum() if reduction == 'sum' else loss.mean())
                else:
                    loss = fn(aa, bb, reduction)
                ((loss * uu).sum() if reduction == 'none' else loss * G.UP_SCALAR).backward()
                return (leaf.grad,)
            res.append(repeated(run)[0] if fn is fn32 else run()[0])
        return res

    for alpha, gamma, sm_ in G.FOCAL_GRID:
        for red in G.REDUCTIONS:
            for s in G.SELECTS:
                k = G.key('focal', alpha, gamma, sm_, red, s)
                out[f'{k}/g32'], out[f'{k}/g64'] = one(lambda a, b: R.focal_value(a, b, alpha, gamma, sm_),
                                                       lambda a, b, r: sigmoid_focal_loss(a, b, alpha, gamma, sm_, r), x, t, red, s, 1)
    for kind, fn in (('giou', ctr_giou_loss), ('diou', ctr_diou_loss)):
        for red in G.REDUCTIONS:
            for s in G.SELECTS:
                k = G.key('iou', kind, red, s)
                out[f'{k}/g32'], out[f'{k}/g64'] = one(lambda a, b: R.iou_value(a, b, kind), lambda a, b, r: fn(a, b, r), pred, gt, red, s, 2)
        leaf = pred.clone().requires_grad_(True)                       # 'mean' over an empty selection: 0.0 * loss.sum()
        fn(leaf[:0], gt[:0], 'mean').backward()
        assert bool((leaf.grad == 0).all())

    # ------------------------------------------------------------------ the non-smooth pairs, eager
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--ties-child'], env=dict(os.environ, PYTORCH_JIT='0'), capture_output=True,
                       text=True, check=True)
    ties = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('TIES ')][0][5:])
    for kind in G.IOU_KINDS:
        out[f'ties/{kind}'] = torch.tensor(ties[kind], dtype=torch.float64)
        restated = R.iou_grad(torch.tensor(G.TIE_PRED), torch.tensor(G.TIE_GT), kind)
        print(f'ties {kind}: eager reference {ties[kind]}')
        assert torch.allclose(out[f'ties/{kind}'], restated, rtol=1e-6, atol=0), (kind, restated)
    for i, want in G.TIE_DIOU_EAGER.items():
        assert np.allclose(ties['diou'][i], want, rtol=1e-6), (i, ties['diou'][i])
    MG.save('objective_grad.npz', out)


if __name__ == '__main__':
    if '--ties-child' in sys.argv:
        ties_child()
    else:
        main()
