"""CPU checks around the gradient of the point objective (csrc/objective.hip, csrc/loss.hip, loss.PointObjective.grad): the ABI
table, the restated formulas of tests/objective_grad_ref.py (finite differences, autograd, the convention table) and the
self-consistency of tests/golden/objective_grad.npz.  No GPU, no compute calls."""
import os
import re

import pytest
import torch

from conftest import Golden, ROOT, load_pkg
import objective_cases as C
import objective_grad_cases as G
import objective_grad_ref as R


def test_gradient_exports_are_in_header_and_ctypes_table_with_equal_arity():
    pkg = load_pkg()
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'decafnet_hip.h')).read(), flags=re.S)
    for name, arity in (('dcf_sigmoid_focal_loss_grad', 12), ('dcf_ctr_iou_loss_grad', 11), ('dcf_point_objective_grad', 30)):
        assert name in pkg._lib.SIGNATURES, name
        m = re.search(name + r'\s*\((.*?)\)\s*;', src, flags=re.S)
        assert m, name
        assert len(m.group(1).split(',')) == len(pkg._lib.SIGNATURES[name][1]) == arity
    # additions only: the version and the existing argument lists stay
    eng = open(os.path.join(ROOT, 'cvpr2025-decafnet_amd', 'csrc', 'engine.hip')).read()
    assert re.search(r'dcf_abi_version\(void\)\s*\{\s*return 12;', eng)
    assert len(pkg._lib.SIGNATURES['dcf_point_objective'][1]) == 24 and len(pkg._lib.SIGNATURES['dcf_annotate_points'][1]) == 15
    assert len(pkg._lib.SIGNATURES['dcf_sigmoid_focal_loss'][1]) == 11 and len(pkg._lib.SIGNATURES['dcf_ctr_iou_loss'][1]) == 10
    assert callable(pkg.loss.PointObjective.grad)


def test_the_elementwise_gradients_live_in_the_shared_header():
    """focal_grad_elem / iou_grad_elem are defined once, beside the values, and used by both kernel files"""
    csrc = os.path.join(ROOT, 'cvpr2025-decafnet_amd', 'csrc')
    elem = open(os.path.join(csrc, 'loss_elem.h')).read()
    for fn in ('focal_grad_elem', 'iou_grad_elem'):
        assert len(re.findall(r'__device__[^;{]*\b' + fn + r'\s*\(', elem)) == 1
        for f in ('loss.hip', 'objective.hip'):
            src = open(os.path.join(csrc, f)).read()
            assert fn + '(' in src and not re.search(r'__device__[^;{]*\b' + fn + r'\s*\(', src), (fn, f)


def test_restated_gradients_agree_with_central_differences():
    """fp64 spot check: (f(x + h) - f(x - h)) / 2h at tie-free points"""
    x, t, pred, gt, _, _ = G.loss_inputs()
    h = 1e-6
    for alpha, gamma, sm in G.FOCAL_GRID:
        xd = x.double()
        fd = (R.focal_value(xd + h, t, alpha, gamma, sm) - R.focal_value(xd - h, t, alpha, gamma, sm)) / (2 * h)
        torch.testing.assert_close(R.focal_grad(x, t, alpha, gamma, sm), fd, rtol=1e-6, atol=1e-9)
    for kind in G.IOU_KINDS:
        g = R.iou_grad(pred, gt, kind)
        for side in (0, 1):
            e = torch.zeros(2, dtype=torch.float64)
            e[side] = h
            fd = (R.iou_value(pred.double() + e, gt, kind) - R.iou_value(pred.double() - e, gt, kind)) / (2 * h)
            torch.testing.assert_close(g[:, side], fd, rtol=1e-6, atol=1e-9)


def test_restated_gradients_follow_eager_autograd_at_the_non_smooth_points():
    """the convention table of include/decafnet_hip.h: the closed form, eager autograd through the restated values, and the
    reference's functions run without scripting (stored in the fixture) agree"""
    g = Golden('objective_grad.npz')
    pred, gt = torch.tensor(G.TIE_PRED), torch.tensor(G.TIE_GT)
    assert bool(R.non_smooth(pred, gt)[[0, 1, 2, 4, 5]].all()) and not bool(R.non_smooth(pred, gt)[[3, 6]].any())
    for kind in G.IOU_KINDS:
        closed = R.iou_grad(pred, gt, kind)
        leaf = pred.double().requires_grad_(True)
        R.iou_value(leaf, gt, kind).sum().backward()
        torch.testing.assert_close(closed, leaf.grad, rtol=1e-12, atol=0)
        torch.testing.assert_close(closed, g.t(f'ties/{kind}'), rtol=1e-6, atol=0)          # the reference computed in fp32
    for i, want in G.TIE_DIOU_EAGER.items():
        torch.testing.assert_close(R.iou_grad(pred[i], gt[i], 'diou'), torch.tensor(want, dtype=torch.float64), rtol=1e-12, atol=0)
    # mirror images: swapping left and right swaps the gradient
    for a, b in ((0, 4), (1, 5), (3, 6)):
        for kind in G.IOU_KINDS:
            assert torch.equal(R.iou_grad(pred[a], gt[a], kind), R.iou_grad(pred[b], gt[b], kind).flip(-1))


def small_case(bn, mode):
    tr = Golden('train.npz')
    targets, rows = C.SMALL_BATCHES[bn]
    cat = lambda n: torch.cat([tr.t(f'{n}/l{l}') for l in range(C.SMALL['L'])], 1)[rows]          # noqa: E731
    labels, gt = R.annotate(C.SMALL['T'], C.SMALL['L'], C.SMALL['max_seq_len'], C.SMALL['regression_range'], C.SMALL['sigma'], targets,
                            C.MODES[mode][0], C.RADIUS)
    return cat('logits1'), cat('logits2'), cat('offsets'), cat('masks'), labels, gt


@pytest.mark.parametrize('mode', ['radius', 'none'])
def test_fixture_is_self_consistent(mode):
    """guards the fixture, not the kernel: the closed form reproduces the stored fp64 autograd gradient, the reference's fp32
    gradient lies within fp32 rounding of it, zeros are where they belong, and the condition on excluded elements holds"""
    g = Golden('objective_grad.npz')
    reg_loss = C.MODES[mode][1]
    want_pos = {'a': (5, 6), 'b': (6, 51), 'z': (0, 0)}
    for bn in C.SMALL_BATCHES:
        l1, l2, off, msk, labels, gt = small_case(bn, mode)
        pos = labels & msk
        k = f'small/{bn}/{mode}'
        assert int(pos.sum()) == want_pos[bn][mode == 'none']
        ex = g.t(f'{k}/excluded')
        assert torch.equal(ex, R.non_smooth(off, gt) & pos) and int(ex.sum()) <= 0.01 * int(pos.sum())
        ln, ws, lw = C.GRID[0]
        closed = R.objective_grad(l1, l2, off, msk, labels, gt, reg_loss, ln, ws, lw, C.FC_A, C.FC_S)
        for name, c in zip(('g1', 'g2', 'go'), closed):
            g64 = g.t(f'{k}/{name}_64')
            torch.testing.assert_close(c, g64, rtol=1e-9, atol=1e-15)
            zero = ~msk if name != 'go' else ~pos
            assert bool((g64[zero] == 0).all())
        for i, (ln, ws, lw) in enumerate(C.GRID):
            for name in ('g1', 'g2', 'go'):
                g32 = g.t(f'{k}/ln{ln}_ws{ws}/{name}_32') if name != 'go' else g.t(f'{k}/{i}/go_32')
                scale = (ws / ln) / (C.GRID[0][1] / C.GRID[0][0]) * (lw if name == 'go' else 1.0)
                g64 = g.t(f'{k}/{name}_64') * scale
                assert float((g32.double() - g64).abs().max()) <= 2e-6 * max(float(g64.abs().max()), 1e-30) or bn == 'z' and name == 'go'
                zero = ~msk if name != 'go' else ~pos
                assert bool((g32[zero] == 0).all())
    for m in C.MODES:
        assert g.t(f'bench/{m}/excluded_idx').numel() == 0
    x, t, pred, gt, sel, up = G.loss_inputs()
    for alpha, gamma, sm in G.FOCAL_GRID:                                                     # the loss functions: 'none', no selection
        torch.testing.assert_close(g.t(G.key('focal', alpha, gamma, sm, 'none', False) + '/g64'), R.focal_grad(x, t, alpha, gamma, sm) * up.double(),
                                   rtol=1e-9, atol=1e-15)
        want = torch.where(sel, R.focal_grad(x, t, alpha, gamma, sm) * G.UP_SCALAR / int(sel.sum()), torch.zeros((), dtype=torch.float64))
        torch.testing.assert_close(g.t(G.key('focal', alpha, gamma, sm, 'mean', True) + '/g64'), want, rtol=1e-9, atol=1e-15)
    for kind in G.IOU_KINDS:
        torch.testing.assert_close(g.t(G.key('iou', kind, 'sum', False) + '/g64'), R.iou_grad(pred, gt, kind) * G.UP_SCALAR, rtol=1e-9, atol=1e-15)


def test_gradient_path_has_no_cpu_fallback():
    Ls = load_pkg().loss
    x = torch.zeros(4, requires_grad=True)
    with pytest.raises(RuntimeError, match='MI355X'):
        Ls.sigmoid_focal_loss(x, torch.zeros(4), reduction='sum')
    with pytest.raises(RuntimeError, match='MI355X'):
        Ls.ctr_diou_loss(torch.ones(4, 2, requires_grad=True), torch.ones(4, 2), reduction='sum')
