"""GPU checks of the gradient of the point objective (k_objective's gradient instantiation, csrc/objective.hip;
k_loss_grad, csrc/loss.hip; loss.PointObjective.grad and the autograd path of loss.py) against the reference's own
`total.backward()` (tests/golden/objective_grad.npz, tests/golden/make_golden_objective_grad.py).

The yardstick is the reference, not the code under test.  Per case and gradient tensor, over the compared elements,
e_ref = max |g_ref32 - g_64| and e_gpu = max |g_gpu - g_64|, and the requirement is

    e_gpu <= max(4 * e_ref, 2^-21 * max |g_64|)

(a factor 4 because the closed-form derivative and autograd's chain of about ten fp32 operations round at different places; a
floor of four fp32 ulps of the largest element because e_ref over a dozen positive points can be small by luck).  Elements at a tie
or with union / hull under eps are left out of the comparison with the scripted reference (none in the reference-generated
cases) and covered by the constructed pairs of tests/objective_grad_cases.py.  Where the fixture holds no reference gradient
(inputs made up in the test), g_ref32 is the same expression under fp32 autograd on the CPU.

Measured on an MI355X (every case: profiles/objective_grad.md): the largest e_gpu / bound of the file is 0.45 (small/b/none grid 4,
g2: e_gpu 6.9e-9, e_ref 3.9e-9 on gradients of at most 2.0e-2); bench scale e_gpu 4.8e-10 / 2.3e-10 (logits / offsets) against
e_ref 3.1e-10 / 8.6e-11 and a bound of 1.2e-9 / 8.5e-10.
"""
import numpy as np
import pytest
import torch

from conftest import Golden, load_pkg
import objective_cases as C
import objective_grad_cases as G
import objective_grad_ref as R

pytestmark = pytest.mark.gpu
FLOOR = 2.0 ** -21


def check(tag, got, g64, g32, keep=None):
    """the accuracy requirement of this file; ``keep``: the compared elements (None = all)"""
    got, g64, g32 = got.detach().cpu().double(), g64.double(), g32.double()
    if keep is not None:
        keep = keep.expand_as(g64) if keep.dim() == g64.dim() else keep[..., None].expand_as(g64)
        got, g64, g32 = got[keep], g64[keep], g32[keep]
    if g64.numel() == 0:
        return
    assert bool(torch.isfinite(got).all()), tag
    e_ref, e_gpu, top = float((g32 - g64).abs().max()), float((got - g64).abs().max()), float(g64.abs().max())
    bound = max(4 * e_ref, FLOOR * top)
    print(f'GRADERR {tag}: max|g64| {top:.3e} e_ref {e_ref:.3e} e_gpu {e_gpu:.3e} bound {bound:.3e}')
    assert e_gpu <= bound, (tag, e_gpu, bound)


def opt_for(pkg, case, mode=None, loss_norm=160.0, loss_weight=1.0):
    opt = pkg.config.make_opt(n_levels=case['L'], max_seq_len=case['max_seq_len'])
    if mode is not None:
        opt.train['center_sampling'], opt.train['reg_loss'] = C.MODES[mode]
    opt.train['loss_norm'], opt.train['loss_weight'] = loss_norm, loss_weight
    return opt


def small_packed(rows, names=('logits1', 'logits2', 'offsets', 'masks'), fixture='train.npz', prefix=''):
    g = Golden(fixture)
    return [torch.cat([g.t(f'{prefix}{n}/l{l}') for l in range(C.SMALL['L'])], 1)[rows].contiguous() for n in names]


def levels(x, case):
    return x.split(C.level_sizes(case['T'], case['L']), 1)


def ref_annotation(case, targets, mode):
    return R.annotate(case['T'], case['L'], case['max_seq_len'], case['regression_range'], case['sigma'], targets, C.MODES[mode][0], C.RADIUS)


def cat(parts):
    return torch.cat(tuple(parts), 1)


@pytest.mark.parametrize('mode', ['radius', 'none'])
def test_gradient_matches_total_backward_of_the_reference_small(mode):
    """batches a, b, z (no positive point at all) over the grid of (loss_norm, world_size, loss_weight); zeros are exact"""
    pkg = load_pkg()
    g = Golden('objective_grad.npz')
    for bn, (targets, rows) in C.SMALL_BATCHES.items():
        l1, l2, off, msk = small_packed(rows)
        labels, _ = ref_annotation(C.SMALL, targets, mode)
        pos = labels & msk
        outs = tuple(levels(x.cuda(), C.SMALL) for x in (l1, l2, off, msk))
        tg = torch.tensor(targets).cuda()
        k = f'small/{bn}/{mode}'
        keep = ~g.t(f'{k}/excluded')
        for i, (ln, ws, lw) in enumerate(C.GRID):
            obj = pkg.loss.PointObjective(opt_for(pkg, C.SMALL, mode, ln, lw), world_size=ws)
            got = obj.grad(outs, tg)
            assert len(got) == 3 and [p.shape for p in got[2]] == [p.shape for p in outs[2]]
            scale = (ws / ln) / (C.GRID[0][1] / C.GRID[0][0])
            for name, gp in zip(('g1', 'g2', 'go'), got):
                gp = cat(gp).cpu()
                g32 = g.t(f'{k}/ln{ln}_ws{ws}/{name}_32') if name != 'go' else g.t(f'{k}/{i}/go_32')
                g64 = g.t(f'{k}/{name}_64') * (scale * (lw if name == 'go' else 1.0))
                check(f'{k} grid{i} {name}', gp, g64, g32, keep if name == 'go' else None)
                assert bool((gp[~msk if name != 'go' else ~pos] == 0).all()), (k, i, name)           # exactly 0, not small
            if bn == 'z':
                assert bool((cat(got[2]) == 0).all())


def test_gradient_of_the_single_head_form():
    pkg = load_pkg()
    g = Golden('objective_grad.npz')
    sl, so, sm = small_packed([0, 1, 2], ('logits', 'offsets', 'masks'), 'train_secondary.npz', 'late/')
    targets = C.SMALL_BATCHES['a'][0]
    outs = tuple(levels(x.cuda(), C.SMALL) for x in (sl, so, sm))
    obj = pkg.loss.PointObjective(opt_for(pkg, C.SMALL, 'radius'))
    got = obj.grad(outs, torch.tensor(targets).cuda())
    assert len(got) == 2
    keep = ~g.t('small/late/excluded')
    check('small/late g2', cat(got[0]), g.t('small/late/g2_64'), g.t('small/late/g2_32'))
    check('small/late go', cat(got[1]), g.t('small/late/go_64'), g.t('small/late/go_32'), keep)
    assert bool((cat(got[0]).cpu()[~sm] == 0).all())


@pytest.mark.parametrize('mode', ['radius', 'none'])
def test_gradient_at_bench_scale(mode):
    """the stored points (every labelled point, its neighbours, a fixed stride through the rest), the per-row-and-level sums, and
    exact zeros outside masks / labels & masks.  The sums follow from the elementwise requirement by the triangle inequality:
    |sum_gpu - sum_64| <= n_valid * bound."""
    pkg = load_pkg()
    g = Golden('objective_grad.npz')
    l1, l2, off, msk, tg = C.bench_inputs()
    labels, _ = ref_annotation(C.BENCH, C.BENCH_TARGETS, mode)
    pos = labels & msk
    assert int(pos.sum()) == {'radius': 12, 'none': 79}[mode]
    outs = tuple(levels(x.cuda(), C.BENCH) for x in (l1, l2, off, msk))
    obj = pkg.loss.PointObjective(opt_for(pkg, C.BENCH, mode))
    got = obj.grad(outs, tg.cuda())
    idx = g.t(f'bench/{mode}/idx').long()
    assert g.t(f'bench/{mode}/excluded_idx').numel() == 0
    lv = np.cumsum([0] + C.level_sizes(C.BENCH['T'], C.BENCH['L']))
    nvalid = g.t(f'bench/{mode}/valid_per_level').double()
    for name, gp in zip(('g1', 'g2', 'go'), got):
        gp = cat(gp).cpu()
        g64, g32 = g.t(f'bench/{mode}/{name}_64'), g.t(f'bench/{mode}/{name}_32')
        check(f'bench/{mode} {name}', gp[idx[:, 0], idx[:, 1]], g64, g32)
        assert bool((gp[~msk if name != 'go' else ~pos] == 0).all())
        bound = max(4 * float((g32.double() - g64).abs().max()), FLOOR * float(g64.abs().max()))
        d = gp.double().reshape(gp.size(0), gp.size(1), -1)
        sums = torch.stack([torch.stack([d[r, lv[l]:lv[l + 1]].sum() for l in range(C.BENCH['L'])]) for r in range(d.size(0))])
        sabs = torch.stack([torch.stack([d[r, lv[l]:lv[l + 1]].abs().sum() for l in range(C.BENCH['L'])]) for r in range(d.size(0))])
        width = d.size(-1)
        for what, a, b in (('sum', sums, g.t(f'bench/{mode}/{name}_sum64')), ('abs', sabs, g.t(f'bench/{mode}/{name}_abs64'))):
            err = (a - b).abs()
            print(f'GRADSUM bench/{mode} {name} {what}: max |gpu - fp64| {float(err.max()):.3e}, allowed {float((nvalid * width * bound).max()):.3e}')
            assert bool((err <= nvalid * width * bound).all()), (name, what)


def _loss_backward(fn, a, b, reduction, select, sel, up):
    leaf = a.cuda().requires_grad_(True)
    loss = fn(leaf, b.cuda(), reduction=reduction, select=sel.cuda() if select else None)
    assert loss.grad_fn is not None
    ((loss * up.cuda()).sum() if reduction == 'none' else loss * G.UP_SCALAR).backward()
    return leaf.grad


def test_loss_function_gradients():
    """sigmoid_focal_loss (alpha, gamma incl. the powf branch, smoothing) and ctr_giou_loss / ctr_diou_loss: every reduction, with
    and without a selection, through the autograd path of loss.py"""
    Ls = load_pkg().loss
    g = Golden('objective_grad.npz')
    x, t, pred, gt, sel, up = G.loss_inputs()
    for alpha, gamma, sm in G.FOCAL_GRID:
        for red in G.REDUCTIONS:
            for s in G.SELECTS:
                k = G.key('focal', alpha, gamma, sm, red, s)
                fn = lambda a, b, reduction, select: Ls.sigmoid_focal_loss(a, b, alpha, gamma, sm, reduction, select)       # noqa: E731
                got = _loss_backward(fn, x, t, red, s, sel, up)
                check(k, got, g.t(f'{k}/g64'), g.t(f'{k}/g32'))
                if s:
                    assert bool((got.cpu()[~sel] == 0).all())
    for kind, fn in (('giou', Ls.ctr_giou_loss), ('diou', Ls.ctr_diou_loss)):
        for red in G.REDUCTIONS:
            for s in G.SELECTS:
                k = G.key('iou', kind, red, s)
                got = _loss_backward(fn, pred, gt, red, s, sel, up)
                check(k, got, g.t(f'{k}/g64'), g.t(f'{k}/g32'))
                if s:
                    assert bool((got.cpu()[~sel] == 0).all())
        leaf = pred.cuda().requires_grad_(True)                          # 'mean' over an empty selection: zeros, as 0.0 * loss.sum()
        fn(leaf, gt.cuda(), reduction='mean', select=torch.zeros(G.LOSS_N, dtype=torch.bool, device='cuda')).backward()
        assert bool((leaf.grad == 0).all())
    # the helpers the Trainer wraps them in
    lab = (t >= 0.5)
    leaf = x.cuda().requires_grad_(True)
    Ls.calc_focal_loss(leaf, lab.cuda(), C.FC_S, C.FC_A).backward()
    t32 = lab.float() * (1.0 - C.FC_S) + C.FC_S / 2
    want = R.focal_grad(x, t32, C.FC_A, 2.0, True)
    tl = x.clone().requires_grad_(True)
    R.focal_value(tl, t32, C.FC_A, 2.0, True, torch.float32).sum().backward()
    check('calc_focal_loss', leaf.grad, want, tl.grad)
    leaf = pred.cuda().requires_grad_(True)
    Ls.calc_iou_loss(leaf, gt.cuda(), 'diou').backward()
    check('calc_iou_loss', leaf.grad, g.t(G.key('iou', 'diou', 'sum', False) + '/g64') / G.UP_SCALAR, g.t(G.key('iou', 'diou', 'sum', False) + '/g32') / G.UP_SCALAR)


def test_non_smooth_points_follow_eager_autograd():
    """the constructed pairs (the convention table and its mirror images): expected values from the reference's functions run
    without scripting; each pair is a case of its own, so a zero gradient must be exactly zero.  Then the fused kernel with the
    predictions set equal to the ground truth at every positive point (both ties at once: the IoU gradient vanishes)."""
    pkg = load_pkg()
    Ls = pkg.loss
    g = Golden('objective_grad.npz')
    pred, gt = torch.tensor(G.TIE_PRED), torch.tensor(G.TIE_GT)
    for kind, fn in (('giou', Ls.ctr_giou_loss), ('diou', Ls.ctr_diou_loss)):
        want = g.t(f'ties/{kind}')
        for red in ('sum', 'none'):
            leaf = pred.cuda().requires_grad_(True)
            fn(leaf, gt.cuda(), reduction=red).sum().backward()
            for i in range(len(G.TIE_PRED)):
                check(f'ties/{kind}/{red}/{i}', leaf.grad[i], R.iou_grad(pred[i], gt[i], kind), want[i])
    for i, w in G.TIE_DIOU_EAGER.items():
        torch.testing.assert_close(leaf.grad[i].cpu().double(), torch.tensor(w, dtype=torch.float64), rtol=1e-6, atol=0)
    for mode in C.MODES:
        targets, rows = C.SMALL_BATCHES['b']
        l1, l2, off, msk = small_packed(rows)
        labels, gt_off = ref_annotation(C.SMALL, targets, mode)
        pos = labels & msk
        off = torch.where(pos[..., None], gt_off, off)
        outs = tuple(levels(x.cuda(), C.SMALL) for x in (l1, l2, off, msk))
        got = pkg.loss.PointObjective(opt_for(pkg, C.SMALL, mode)).grad(outs, torch.tensor(targets).cuda())
        want = R.objective_grad(l1, l2, off, msk, labels, gt_off, C.MODES[mode][1], 160.0, 1, 1.0, C.FC_A, C.FC_S)
        assert bool((want[2] == 0).all()) and bool((cat(got[2]) == 0).all()) and int(pos.sum()) > 0


def test_extreme_logits_give_finite_gradients():
    """|x| = 20 and 100 against both smoothed labels: the loss function on its own, and inside the fused kernel"""
    pkg = load_pkg()
    Ls = pkg.loss
    x = torch.tensor(G.EXTREME_X)
    lab = torch.tensor(G.EXTREME_POS)
    for alpha, gamma, sm in G.FOCAL_GRID:
        t = (lab.float() * (1.0 - C.FC_S) + C.FC_S / 2) if sm else lab.float()
        leaf = x.cuda().requires_grad_(True)
        Ls.sigmoid_focal_loss(leaf, t.cuda(), alpha, gamma, sm, 'sum').backward()
        tl = x.clone().requires_grad_(True)
        R.focal_value(tl, t, alpha, gamma, sm, torch.float32).sum().backward()
        assert bool(torch.isfinite(tl.grad).all())
        check(G.key('extreme', alpha, gamma, sm), leaf.grad, R.focal_grad(x, t, alpha, gamma, sm), tl.grad)
    targets, rows = C.SMALL_BATCHES['b']
    l1, l2, off, msk = small_packed(rows)
    labels, gt_off = ref_annotation(C.SMALL, targets, 'none')
    where = torch.nonzero(labels & msk)[:8]
    more = torch.nonzero(~labels & msk)[:8]
    for j, v in enumerate(G.EXTREME_X):
        l1[where[j, 0], where[j, 1]] = v
        l2[more[j, 0], more[j, 1]] = v
    outs = tuple(levels(x.cuda(), C.SMALL) for x in (l1, l2, off, msk))
    got = pkg.loss.PointObjective(opt_for(pkg, C.SMALL, 'none')).grad(outs, torch.tensor(targets).cuda())
    args = (l1, l2, off, msk, labels, gt_off, 'giou', 160.0, 1, 1.0, C.FC_A, C.FC_S)
    want, ref = R.objective_grad(*args), R.autograd_objective_grad(*args, dt=torch.float32)
    for name, a, b, c in zip(('g1', 'g2', 'go'), got, want, ref):
        check(f'extreme fused {name}', cat(a), b, c)


def test_scalar_path_odd_row_length_and_unaligned_operands():
    """S % 4 != 0 (T = 250, two levels) takes the point-by-point path; so do operands that are not 16-byte aligned (the same
    (T = 256, L = 4) inputs one float into a larger buffer), which must give the bits of the aligned call"""
    pkg = load_pkg()
    case = dict(T=250, L=2, max_seq_len=256, regression_range=4, sigma=0.5)
    S = sum(C.level_sizes(case['T'], case['L']))
    gen = torch.Generator().manual_seed(5)
    l1, l2 = torch.randn(3, S, generator=gen) * 2 - 1, torch.randn(3, S, generator=gen) * 2 - 1
    off = torch.rand(3, S, 2, generator=gen) * 5
    msk = torch.rand(3, S, generator=gen) < 0.8
    targets = [[30.2, 41.7], [100.0, 180.5], [3.3, 5.1]]
    for mode in C.MODES:
        labels, gt_off = ref_annotation(case, targets, mode)
        assert int((labels & msk).sum()) > 0
        outs = tuple(levels(x.cuda(), case) for x in (l1, l2, off, msk))
        got = pkg.loss.PointObjective(opt_for(pkg, case, mode)).grad(outs, torch.tensor(targets).cuda())
        args = (l1, l2, off, msk, labels, gt_off, C.MODES[mode][1], 160.0, 1, 1.0, C.FC_A, C.FC_S)
        want, ref = R.objective_grad(*args), R.autograd_objective_grad(*args, dt=torch.float32)
        keep = ~(R.non_smooth(off, gt_off) & labels & msk)
        for name, a, b, c in zip(('g1', 'g2', 'go'), got, want, ref):
            check(f'odd/{mode} {name}', cat(a), b, c, keep if name == 'go' else None)
            assert bool((cat(a).cpu()[~msk if name != 'go' else ~(labels & msk)] == 0).all())
    # unaligned: through the C ABI
    lib, _l = pkg._lib.lib(), pkg._lib
    targets, rows = C.SMALL_BATCHES['b']
    packed = [x.cuda() for x in small_packed(rows)]
    n, S = packed[1].shape
    tg, ln = torch.tensor(targets).cuda(), torch.full((1,), 160.0, device='cuda')

    def call(shift):
        def place(x):
            buf = torch.zeros(x.numel() + 8, device='cuda', dtype=x.dtype)
            v = buf[shift:shift + x.numel()].view(x.shape)
            v.copy_(x)
            return v
        a1, a2, ao = (place(x) for x in packed[:3])
        g1, g2, go = (place(torch.full_like(x, float('nan'))) for x in packed[:3])
        _l.check(lib.dcf_point_objective_grad(_l.ptr(a1), _l.ptr(a2), _l.ptr(ao), _l.ptr(packed[3]), _l.ptr(tg), n, C.SMALL['T'], C.SMALL['L'], 4.0, 0.5,
                                              0, C.SMALL['max_seq_len'], 1, C.RADIUS, C.FC_A, C.FC_S, 1, 1e-8, _l.ptr(ln), 1.0, 1.0, None, None,
                                              _l.ptr(g1), _l.ptr(g2), _l.ptr(go), 0, None, None, _l.current_stream()), 'dcf_point_objective_grad')
        return g1.clone(), g2.clone(), go.clone()
    for a, b in zip(call(0), call(1)):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)


@pytest.mark.parametrize('scale', ['small', 'bench'])
def test_fused_gradient_equals_composed_loss_function_gradients(scale):
    """dcf_point_objective_grad against dcf_annotate_points followed by the loss functions' own gradients with select= and the
    Trainer's scalars applied in torch: both within the requirement of the fixture's case, and of each other"""
    pkg = load_pkg()
    Ls = pkg.loss
    g = Golden('objective_grad.npz')
    mode = 'radius'
    cs, reg_loss = C.MODES[mode]
    if scale == 'small':
        case, k = C.SMALL, 'small/b/radius'
        targets, rows = C.SMALL_BATCHES['b']
        l1, l2, off, msk = (x.cuda() for x in small_packed(rows))
        tg = torch.tensor(targets).cuda()
    else:
        case, k = C.BENCH, 'bench/radius'
        l1, l2, off, msk, tg = (x.cuda() for x in C.bench_inputs())
    pts = pkg.modeling.PtGenerator(case['max_seq_len'], case['L'], case['regression_range'], case['sigma'])(C.level_sizes(case['T'], case['L']))
    fused = pkg.loss.PointObjective(opt_for(pkg, case, mode)).grad(tuple(levels(x, case) for x in (l1, l2, off, msk)), tg)
    labels, gt_off = Ls.annotate_points(pts, tg, center_sampling=cs, center_sampling_radius=C.RADIUS)
    pos = labels & msk
    leaves = [x.clone().requires_grad_(True) for x in (l1, l2, off)]
    c1 = Ls.calc_focal_loss(leaves[0], labels, C.FC_S, C.FC_A, select=msk) / 160.0 * 1
    c2 = Ls.calc_focal_loss(leaves[1], labels, C.FC_S, C.FC_A, select=msk) / 160.0 * 1
    reg = Ls.calc_iou_loss(leaves[2], gt_off, reg_loss, select=pos) / 160.0 * 1
    ((c1 + c2) / 2 + 1.0 * reg).backward()
    for name, f, leaf in zip(('g1', 'g2', 'go'), fused, leaves):
        f, c = cat(f).cpu(), leaf.grad.cpu()
        if scale == 'small':
            g64, g32 = g.t(f'{k}/{name}_64'), g.t(f'{k}/ln160.0_ws1/{name}_32') if name != 'go' else g.t(f'{k}/0/go_32')
        else:
            idx = g.t(f'{k}/idx').long()
            f, c = f[idx[:, 0], idx[:, 1]], c[idx[:, 0], idx[:, 1]]
            g64, g32 = g.t(f'{k}/{name}_64'), g.t(f'{k}/{name}_32')
        check(f'composed/{scale} {name}', c, g64, g32)
        bound = max(4 * float((g32.double() - g64).abs().max()), FLOOR * float(g64.abs().max()))
        d = float((f.double() - c.double()).abs().max())
        print(f'GRADERR fused-vs-composed/{scale} {name}: {d:.3e} bound {bound:.3e}')
        assert d <= bound


def test_autograd_path_equals_the_direct_form():
    """total.backward() on leaf outputs, on level views of one packed leaf and on results of torch ops leaves the bits of
    PointObjective.grad; a non-unit upstream gradient scales it; cls / reg on their own; accumulate; values unchanged"""
    pkg = load_pkg()
    targets, rows = C.SMALL_BATCHES['b']
    l1, l2, off, msk = (x.cuda() for x in small_packed(rows))
    tg = torch.tensor(targets).cuda()
    obj = pkg.loss.PointObjective(opt_for(pkg, C.SMALL, 'none', 7.5, 0.25), world_size=4)
    mk = levels(msk, C.SMALL)
    plain = obj((levels(l1, C.SMALL), levels(l2, C.SMALL), levels(off, C.SMALL), mk), tg)
    assert all(plain[k].grad_fn is None and not plain[k].requires_grad for k in ('cls', 'reg', 'total'))
    direct = [cat(p) for p in obj.grad((levels(l1, C.SMALL), levels(l2, C.SMALL), levels(off, C.SMALL), mk), tg)]
    assert all(float(d.abs().max()) > 0 for d in direct)

    # (1) every level a leaf of its own
    leaves = [[p.clone().requires_grad_(True) for p in levels(x, C.SMALL)] for x in (l1, l2, off)]
    d = obj((*leaves, mk), tg)
    assert d['total'].grad_fn is not None and d['norm'].dtype == torch.int64 and not d['norm'].requires_grad
    for k in ('cls', 'reg', 'total'):
        assert torch.equal(d[k].detach(), plain[k])                       # values bit-equal with and without requires_grad
    assert int(d['norm']) == int(plain['norm'])
    d['total'].backward()
    for parts, want in zip(leaves, direct):
        assert torch.equal(cat([p.grad for p in parts]), want)

    # (2) level views of one packed leaf per tensor, a non-unit upstream gradient
    packed = [x.clone().requires_grad_(True) for x in (l1, l2, off)]
    d = obj((*[levels(x, C.SMALL) for x in packed], mk), tg)
    (d['total'] * 3.0).backward()
    scaled = [cat(p) for p in obj.grad((levels(l1, C.SMALL), levels(l2, C.SMALL), levels(off, C.SMALL), mk), tg, grad_total=3.0)]
    for x, want, one in zip(packed, scaled, direct):
        assert torch.equal(x.grad, want)
        torch.testing.assert_close(x.grad, 3.0 * one, rtol=2e-7, atol=0)
    by_tensor = [cat(p) for p in obj.grad((levels(l1, C.SMALL), levels(l2, C.SMALL), levels(off, C.SMALL), mk), tg,
                                          grad_total=torch.tensor([3.0], device='cuda'))]
    assert all(torch.equal(a, b) for a, b in zip(by_tensor, scaled))

    # (3) results of torch ops: the gradient arrives at the leaves through ordinary autograd
    packed = [x.clone().requires_grad_(True) for x in (l1, l2, off)]
    d = obj((levels(packed[0] * 1.0, C.SMALL), levels(packed[1] + 0.0, C.SMALL), levels(packed[2] * 2.0, C.SMALL), mk), tg)
    d['total'].backward()
    obj2 = [cat(p) for p in obj.grad((levels(l1, C.SMALL), levels(l2, C.SMALL), levels(off * 2.0, C.SMALL), mk), tg)]
    assert torch.equal(packed[0].grad, obj2[0]) and torch.equal(packed[1].grad, obj2[1]) and torch.equal(packed[2].grad, obj2[2] * 2.0)

    # (4) cls and reg on their own: cls sees the logits only, reg the offsets only (total = cls + loss_weight * reg)
    packed = [x.clone().requires_grad_(True) for x in (l1, l2, off)]
    d = obj((*[levels(x, C.SMALL) for x in packed], mk), tg)
    d['cls'].backward(retain_graph=True)
    assert torch.equal(packed[0].grad, direct[0]) and torch.equal(packed[1].grad, direct[1]) and bool((packed[2].grad == 0).all())
    for x in packed:
        x.grad = None
    d['reg'].backward()
    assert bool((packed[0].grad == 0).all()) and bool((packed[1].grad == 0).all())
    torch.testing.assert_close(packed[2].grad * 0.25, direct[2], rtol=2e-7, atol=0)

    # (5) only one tensor requires grad; no_grad returns plain values
    lone = off.clone().requires_grad_(True)
    d = obj((levels(l1, C.SMALL), levels(l2, C.SMALL), levels(lone, C.SMALL), mk), tg)
    d['total'].backward()
    assert torch.equal(lone.grad, direct[2])
    with torch.no_grad():
        assert obj((levels(l1, C.SMALL), levels(l2, C.SMALL), levels(lone, C.SMALL), mk), tg)['total'].grad_fn is None

    # (6) accumulate: twice the gradient (x + x is exact), into the buffers an earlier call returned
    outs = (levels(l1, C.SMALL), levels(l2, C.SMALL), levels(off, C.SMALL), mk)
    first = obj.grad(outs, tg)
    again = obj.grad(outs, tg, out=first, accumulate=True)
    for a, f, one in zip(again, first, direct):
        assert cat(a).data_ptr() != 0 and a[0].data_ptr() == f[0].data_ptr() and torch.equal(cat(a), 2.0 * one)
    over = obj.grad(outs, tg, out=first)                                  # accumulate=False overwrites
    assert all(torch.equal(cat(a), one) for a, one in zip(over, direct))
    with pytest.raises(ValueError):
        obj.grad(outs, tg, accumulate=True)


def test_bench_scale_gradient_is_deterministic_and_the_combined_form_returns_the_values():
    """20 repeats bit-identical through the C ABI; with rows_out / out4 the same pass returns dcf_point_objective's values, bit-equal"""
    pkg = load_pkg()
    lib, _l = pkg._lib.lib(), pkg._lib
    l1, l2, off, msk, tg = (x.cuda() for x in C.bench_inputs())
    ln = torch.full((1,), 160.0, device='cuda')
    head = (_l.ptr(l1), _l.ptr(l2), _l.ptr(off), _l.ptr(msk), _l.ptr(tg), 4, C.BENCH['T'], C.BENCH['L'], 4.0, 0.5, 0, C.BENCH['max_seq_len'], 1,
            C.RADIUS, C.FC_A, C.FC_S, 1, 1e-8, _l.ptr(ln), 1.0, 1.0)
    rows0, out0 = torch.zeros(4, 4, device='cuda'), torch.zeros(4, device='cuda')
    _l.check(lib.dcf_point_objective(*head, _l.ptr(rows0), _l.ptr(out0), _l.current_stream()), 'dcf_point_objective')
    first = None
    for it in range(20):
        g1, g2, go = torch.full_like(l1, float('nan')), torch.full_like(l2, float('nan')), torch.full_like(off, float('nan'))
        rows, out4 = torch.zeros(4, 4, device='cuda'), torch.zeros(4, device='cuda')
        both = it % 2 == 1
        _l.check(lib.dcf_point_objective_grad(*head, None, None, _l.ptr(g1), _l.ptr(g2), _l.ptr(go), 0, _l.ptr(rows) if both else None,
                                              _l.ptr(out4) if both else None, _l.current_stream()), 'dcf_point_objective_grad')
        if both:
            assert torch.equal(rows, rows0) and torch.equal(out4, out0)
        if first is None:
            first = (g1, g2, go)
        assert all(torch.equal(a, b) for a, b in zip((g1, g2, go), first))
    assert all(bool(torch.isfinite(a).all()) for a in first) and float(out0[3]) == 12


def test_forward_objective_gradient_without_a_host_wait():
    """model(..., eval=False) on the train.npz inputs -> PointObjective on the packed storage -> the gradient, directly and through
    backward(), under torch's sync debug mode set to 'error' (as tests/test_gpu_objective.py checks its forward -> loss dict)"""
    pkg = load_pkg()
    g = Golden('train.npz')
    meta, kw = g.js('meta'), g.js('opt_kwargs')
    opt = pkg.config.make_opt(**kw)
    model = pkg.modeling.create_model(opt)
    model.load_state_dict(pkg.synth.make_state_dict(g.js('shapes'), meta['wseed']))
    model = model.cuda().eval().requires_grad_(False)
    args = (g.t('vid').cuda(), g.t('shallow').cuda(), g.t('vid_masks').cuda(), g.t('tokens').cuda(), g.t('text_cls').cuda(), g.t('token_masks').cuda())
    tg = torch.tensor(C.SMALL_BATCHES['a'][0]).cuda()
    obj = pkg.loss.PointObjective(opt)
    out = model(*args, text_size=torch.tensor(meta['sizes']), eval=False)
    assert pkg.loss._packed(out[0]) is out[0][0]._base                   # the split views resolve to the packed buffer: no cat
    sizes = [p.size(1) for p in out[-1]]
    leaves = [pkg.loss._packed(p).clone().requires_grad_(True) for p in out[:3]]
    as_leaves = (*[x.split(sizes, 1) for x in leaves], out[-1])
    warm = obj.grad(out, tg)                                             # first calls: create the device-resident loss_norm, load kernels
    obj(as_leaves, tg)['total'].backward()
    for x in leaves:
        x.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        d = obj(out, tg)
        got = obj.grad(out, tg, out=warm)
        obj.grad(out, tg, grad_total=0.5, out=got, accumulate=True)
        obj(as_leaves, tg)['total'].backward()
        obj.update_norm(d['norm'])
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert int(d['norm']) == 5
    obj.loss_norm = float(opt.train['loss_norm'])                        # back to the norm the calls above divided by
    ref = obj.grad(out, tg)
    for a, r, x in zip(got, ref, leaves):
        assert bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0
        assert torch.equal(x.grad, cat(r))                               # backward() on clones of the outputs: the bits of the direct form
        torch.testing.assert_close(cat(a), 1.5 * cat(r), rtol=1e-6, atol=0)
