"""GPU checks of the point annotation and the Trainer's fused objective (csrc/objective.hip, loss.PointObjective,
evaluator.calc_loss) against the reference's own values (tests/golden/objective.npz, tests/golden/make_golden_objective.py).

Summation deviations at bench scale (T = 16384, L = 8, 4 rows; measured on an MI355X, see profiles/objective.md):
the reference's own |fp32 - fp64| is recorded in the fixture (cls 1.9e-6 / 2.8e-6, reg 2.4e-9 / 1.2e-8, total 2.5e-7 / 4.5e-6 for
radius+DIoU / none+GIoU); the bound is max(2e-5 relative, 4 x that) against the fp64 value.  The GPU's |value - fp64|, measured:
cls 1.9e-6 / 1.0e-6, reg 2.4e-9 / 1.2e-8, total 2.5e-7 / 6.8e-7; norm exact (12 / 79).
"""
import hashlib

import numpy as np
import pytest
import torch

from conftest import Golden, load_pkg
import objective_cases as C

pytestmark = pytest.mark.gpu
TOL_SUM = dict(rtol=2e-5, atol=1e-6)          # loss sums against the reference (tests/test_gpu_e2e.py, the loss block)
TOL_E2E = dict(rtol=2e-4, atol=2e-4)          # the former TOL of tests/test_gpu_e2e.py: the forward's own error enters


def digest(t):
    return hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()


def small_outputs(g, rows, device='cuda'):
    """level tuples of the reference's training-forward outputs stored in train.npz, rows selected"""
    L = C.SMALL['L']
    return tuple(tuple(g.t(f'{n}/l{l}')[rows].to(device) for l in range(L)) for n in ('logits1', 'logits2', 'offsets', 'masks'))


def opt_for(pkg, case, mode=None, loss_norm=160.0, loss_weight=1.0):
    opt = pkg.config.make_opt(n_levels=case['L'], max_seq_len=case['max_seq_len'])
    if mode is not None:
        opt.train['center_sampling'], opt.train['reg_loss'] = C.MODES[mode]
    opt.train['loss_norm'], opt.train['loss_weight'] = loss_norm, loss_weight
    return opt


def abi_annotate(pkg, case, targets, mode, uo):
    lib, _l = pkg._lib.lib(), pkg._lib
    tg = torch.tensor(targets, dtype=torch.float32).cuda()
    n, S = tg.size(0), sum(C.level_sizes(case['T'], case['L']))
    lab, win, rng = (torch.full((n, S), 7, dtype=torch.uint8, device='cuda') for _ in range(3))
    off = torch.full((n, S, 2), float('nan'), device='cuda')
    _l.check(lib.dcf_annotate_points(_l.ptr(tg), n, case['T'], case['L'], float(case['regression_range']), case['sigma'], int(uo),
                                     case['max_seq_len'], int(mode == 'radius'), C.RADIUS, _l.ptr(lab), _l.ptr(off), _l.ptr(win), _l.ptr(rng),
                                     _l.current_stream()), 'dcf_annotate_points')
    return lab.bool().cpu(), off.cpu(), win.bool().cpu(), rng.bool().cpu()


@pytest.mark.parametrize('uo', [False, True])
@pytest.mark.parametrize('mode', ['radius', 'none'])
def test_annotation_is_bit_equal_to_the_reference(mode, uo):
    """labels, offsets and both predicates, small and bench scale, through the C ABI and through loss.annotate_points*"""
    pkg = load_pkg()
    g = Golden('objective.npz')
    cs = C.MODES[mode][0]
    for bn, (targets, _) in C.SMALL_BATCHES.items():
        k = f'small/{bn}/{mode}/uo{int(uo)}'
        want = g.t(f'{k}/labels'), g.t(f'small/{bn}/uo{int(uo)}/offsets'), g.t(f'{k}/in_window'), g.t(f'{k}/in_range')
        got = abi_annotate(pkg, C.SMALL, targets, mode, uo)
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and torch.equal(a, b), k
        pts = pkg.modeling.PtGenerator(C.SMALL['max_seq_len'], C.SMALL['L'], C.SMALL['regression_range'], C.SMALL['sigma'], use_offset=uo)(
            C.level_sizes(C.SMALL['T'], C.SMALL['L']))
        tg = torch.tensor(targets).cuda()
        lab, off = pkg.loss.annotate_points(torch.cat(pts).cuda(), tg, center_sampling=cs, center_sampling_radius=C.RADIUS)
        assert lab.dtype == torch.bool and torch.equal(lab.cpu(), want[0]) and torch.equal(off.cpu(), want[1])
        l0, o0, (w0, r0) = pkg.loss.annotate_points_per_video(pts, tg[0], center_sampling=cs, center_sampling_radius=C.RADIUS)
        assert torch.equal(l0.cpu(), want[0][0]) and torch.equal(o0.cpu(), want[1][0])
        assert torch.equal(w0.cpu(), want[2][0]) and torch.equal(r0.cpu(), want[3][0])
    k = f'bench/{mode}/uo{int(uo)}'
    lab, off, win, rng = abi_annotate(pkg, C.BENCH, C.BENCH_TARGETS, mode, uo)
    assert torch.equal(torch.nonzero(lab), g.t(f'{k}/label_idx'))
    sha = g.js(f'{k}/sha')
    assert digest(off) == sha['offsets'] and digest(win) == sha['in_window'] and digest(rng) == sha['in_range']


@pytest.mark.parametrize('mode', ['radius', 'none'])
def test_objective_matches_the_trainer_on_the_reference_outputs(mode):
    """the Trainer's four outputs over the option grid, including the batch without any positive point"""
    pkg = load_pkg()
    g, tr = Golden('objective.npz'), Golden('train.npz')
    for bn, (targets, rows) in C.SMALL_BATCHES.items():
        outs = small_outputs(tr, rows)
        tg = torch.tensor(targets).cuda()
        want = g.t(f'small/{bn}/{mode}/trainer')
        for i, (ln, ws, lw) in enumerate(C.GRID):
            obj = pkg.loss.PointObjective(opt_for(pkg, C.SMALL, mode, ln, lw), world_size=ws)
            d = obj(outs, tg)
            assert d['norm'].dtype == torch.int64 and int(d['norm']) == int(want[i, 3]), (bn, i)
            for q, name in enumerate(('cls', 'reg', 'total')):
                assert d[name].dim() == 0 and d[name].is_cuda
                print(f'{bn}/{mode} grid {i} {name}: got {float(d[name]):.9g} want {float(want[i, q]):.9g}')
                torch.testing.assert_close(d[name].cpu(), want[i, q], **TOL_SUM)
            if bn == 'z':
                assert float(d['reg']) == 0.0 and int(d['norm']) == 0
            r64 = g.t(f'small/{bn}/{mode}/rows64')
            assert torch.equal(obj.per_row[:, 3].cpu().double(), r64[:, 3])
            torch.testing.assert_close(obj.per_row.cpu().double(), r64, **TOL_SUM)


@pytest.mark.parametrize('mode', ['radius', 'none'])
def test_objective_at_bench_scale_against_fp64(mode):
    pkg = load_pkg()
    g = Golden('objective.npz')
    l1, l2, off, msk, tg = (x.cuda() for x in C.bench_inputs())
    sizes = C.level_sizes(C.BENCH['T'], C.BENCH['L'])
    obj = pkg.loss.PointObjective(opt_for(pkg, C.BENCH, mode))
    d = obj((l1.split(sizes, 1), l2.split(sizes, 1), off.split(sizes, 1), msk.split(sizes, 1)), tg)
    want64, dev = g.t(f'bench/{mode}/trainer64'), g.t(f'bench/{mode}/dev')
    assert int(d['norm']) == int(want64[3]) == {'radius': 12, 'none': 79}[mode]
    for q, name in enumerate(('cls', 'reg', 'total')):
        err, bound = abs(float(d[name]) - float(want64[q])), max(2e-5 * abs(float(want64[q])), 4 * float(dev[q]))
        print(f'bench {mode} {name}: |gpu - fp64| = {err:.3e}, reference |fp32 - fp64| = {float(dev[q]):.3e}, bound {bound:.3e}')
        assert err <= bound, (name, err, bound)
    r64 = g.t(f'bench/{mode}/rows64')
    assert torch.equal(obj.per_row[:, 3].cpu().double(), r64[:, 3])
    torch.testing.assert_close(obj.per_row.cpu().double(), r64, rtol=2e-5, atol=1e-6)


@pytest.mark.parametrize('scale', ['small', 'bench'])
def test_fused_equals_composed(scale):
    """k_objective against dcf_annotate_points followed by the existing loss exports with select=: n_pos equal, sums to summation order"""
    pkg = load_pkg()
    Ls = pkg.loss
    if scale == 'small':
        case, tr = C.SMALL, Golden('train.npz')
        outs = small_outputs(tr, [0, 1, 2])
        tg = torch.tensor(C.SMALL_BATCHES['a'][0]).cuda()
    else:
        case = C.BENCH
        l1, l2, off, msk, tg = (x.cuda() for x in C.bench_inputs())
        sizes = C.level_sizes(case['T'], case['L'])
        outs = (l1.split(sizes, 1), l2.split(sizes, 1), off.split(sizes, 1), msk.split(sizes, 1))
    pts = pkg.modeling.PtGenerator(case['max_seq_len'], case['L'], case['regression_range'], case['sigma'])(C.level_sizes(case['T'], case['L']))
    for mode, (cs, reg_loss) in C.MODES.items():
        obj = Ls.PointObjective(opt_for(pkg, case, mode, 7.5, 0.25), world_size=4)
        d = obj(outs, tg)
        l1, l2, off, msk = (torch.cat(p, 1) for p in outs)
        labels, gt_off = Ls.annotate_points(pts, tg, center_sampling=cs, center_sampling_radius=C.RADIUS)
        pos = labels & msk
        assert int(d['norm']) == int(pos.sum())
        assert torch.equal(obj.per_row[:, 3].long(), pos.sum(1))
        rows = torch.stack([torch.stack([Ls.calc_focal_loss(l1[b], labels[b], C.FC_S, C.FC_A, select=msk[b]),
                                         Ls.calc_focal_loss(l2[b], labels[b], C.FC_S, C.FC_A, select=msk[b]),
                                         Ls.calc_iou_loss(off[b], gt_off[b], reg_loss, select=pos[b])]) for b in range(tg.size(0))])
        torch.testing.assert_close(obj.per_row[:, :3], rows, **TOL_SUM)
        c1 = Ls.calc_focal_loss(l1, labels, C.FC_S, C.FC_A, select=msk) / 7.5 * 4
        c2 = Ls.calc_focal_loss(l2, labels, C.FC_S, C.FC_A, select=msk) / 7.5 * 4
        reg = Ls.calc_iou_loss(off, gt_off, reg_loss, select=pos) / 7.5 * 4
        torch.testing.assert_close(d['cls'], (c1 + c2) / 2, **TOL_SUM)
        torch.testing.assert_close(d['reg'], reg, **TOL_SUM)
        torch.testing.assert_close(d['total'], (c1 + c2) / 2 + 0.25 * reg, **TOL_SUM)


def test_bench_scale_call_is_deterministic():
    """20 repeats bit-identical (out4 and rows_out), through the C ABI"""
    pkg = load_pkg()
    lib, _l = pkg._lib.lib(), pkg._lib
    l1, l2, off, msk, tg = (x.cuda() for x in C.bench_inputs())
    ln = torch.full((1,), 160.0, device='cuda')
    first = None
    for _ in range(20):
        rows, out4 = torch.zeros(4, 4, device='cuda'), torch.zeros(4, device='cuda')
        _l.check(lib.dcf_point_objective(_l.ptr(l1), _l.ptr(l2), _l.ptr(off), _l.ptr(msk), _l.ptr(tg), 4, C.BENCH['T'], C.BENCH['L'], 4.0, 0.5, 0,
                                         C.BENCH['max_seq_len'], 1, C.RADIUS, C.FC_A, C.FC_S, 1, 1e-8, _l.ptr(ln), 1.0, 1.0, _l.ptr(rows),
                                         _l.ptr(out4), _l.current_stream()), 'dcf_point_objective')
        if first is None:
            first = (rows.clone(), out4.clone())
        assert torch.equal(rows, first[0]) and torch.equal(out4, first[1])
    assert float(first[1][3]) == 12


def _train_model(pkg, name):
    if name == 'iter':
        g = Golden('train.npz')
        meta, kw = g.js('meta'), g.js('opt_kwargs')
        opt = pkg.config.make_opt(**kw)
        model = pkg.modeling.create_model(opt)
        model.load_state_dict(pkg.synth.make_state_dict(g.js('shapes'), meta['wseed']))
        model, pre = model.cuda().eval().requires_grad_(False), ''
    else:
        g = Golden('train_secondary.npz')
        case, meta = g.js('cases')[name], g.js('meta')
        opt = pkg.config.make_opt(**case['opt_kwargs'])
        model = pkg.modeling.PtTransformer(opt)
        model.load_state_dict(pkg.synth.make_state_dict(g.js(f'{name}/shapes'), case['wseed']))
        model, pre = model.cuda().train(), f'{name}/'
    args = (g.t(f'{pre}vid').cuda(), g.t(f'{pre}shallow').cuda(), g.t(f'{pre}vid_masks').cuda(), g.t(f'{pre}tokens').cuda(),
            g.t(f'{pre}text_cls').cuda(), g.t(f'{pre}token_masks').cuda())
    return opt, model, args, torch.tensor(meta['sizes'])


@pytest.mark.parametrize('name', ['iter', 'late'])
def test_forward_to_loss_dict_end_to_end_without_a_host_wait(name):
    """model(..., eval=False) on the train.npz / train_secondary.npz inputs -> PointObjective on the packed storage -> the Trainer's
    dict; the objective call runs under torch's sync debug mode set to 'error'"""
    pkg = load_pkg()
    fx = Golden('objective.npz')
    opt, model, args, sizes = _train_model(pkg, name)
    out = model(*args, text_size=sizes, eval=False)
    assert len(out) == (4 if name == 'iter' else 3)
    assert pkg.loss._packed(out[-1]) is out[-1][0]._base                 # the split views resolve to the packed buffer: no cat
    tg = torch.tensor(C.SMALL_BATCHES['a'][0]).cuda()
    obj = pkg.loss.PointObjective(opt)
    obj(out, tg)                                                         # first call: creates the device-resident loss_norm
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        d = obj(out, tg)
        obj.update_norm(d['norm'])
    finally:
        torch.cuda.set_sync_debug_mode('default')
    want = fx.t('small/a/radius/trainer')[0] if name == 'iter' else fx.t('small/late/trainer')      # GRID[0] = (160, 1, 1.0)
    assert int(d['norm']) == int(want[3]) == 5
    for q, k in enumerate(('cls', 'reg', 'total')):
        print(f'{name} {k}: got {float(d[k]):.9g} want {float(want[q]):.9g}')
        torch.testing.assert_close(d[k].cpu(), want[q], **TOL_E2E)
    # the validation-time loss on the same forward (the classification head the evaluator scores with)
    stats, per_row = pkg.evaluator.calc_loss(out[-3:], tg, opt)
    rows, mean = (fx.t('small/a/eval_rows'), fx.t('small/a/eval_mean')) if name == 'iter' else (fx.t('small/late/eval_rows'), fx.t('small/late/eval_mean'))
    np.testing.assert_allclose(per_row, rows.numpy(), rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose([stats['cls_loss'], stats['reg_loss']], mean.numpy(), rtol=2e-4, atol=2e-4)


def test_update_norm_follows_the_trainer_over_three_steps():
    """worker_v2.py:381-382 with the device-resident norm: three steps, one of them without a positive point (max(.., 1))"""
    pkg = load_pkg()
    tr = Golden('train.npz')
    obj = pkg.loss.PointObjective(opt_for(pkg, C.SMALL, 'none', 7.5))
    ref, m = 7.5, 0.9
    for bn in ('b', 'z', 'a'):
        targets, rows = C.SMALL_BATCHES[bn]
        d = obj(small_outputs(tr, rows), torch.tensor(targets).cuda())
        world = [d['norm'], d['norm']]                                   # two ranks' norms, all-gathered
        obj.update_norm(sum(world))
        ref = m * ref + (1. - m) * max(sum(int(n) for n in world), 1)
        assert obj.loss_norm == ref
    # ... and the next step divides by it
    d = obj(small_outputs(tr, [0, 1]), torch.tensor(C.SMALL_BATCHES['b'][0]).cuda())
    want = Golden('objective.npz').t('small/b/none/trainer')[4]           # GRID[4] = (7.5, 1, 1.0)
    torch.testing.assert_close(d['reg'].cpu() * np.float32(ref), want[1] * np.float32(7.5), **TOL_SUM)
    obj.update_norm(3)                                                   # a host number works as well
    assert obj.loss_norm == m * ref + (1. - m) * 3


def test_evaluator_calc_loss_matches_the_reference():
    """Evaluator._calc_loss on the reference's outputs: per row and the mean, including the rows whose n_pos is 0 (norm -> 1),
    in both accepted forms of `outputs`"""
    pkg = load_pkg()
    g, tr = Golden('objective.npz'), Golden('train.npz')
    opt = opt_for(pkg, C.SMALL)
    for bn in ('a', 'b', 'z'):
        targets, rows = C.SMALL_BATCHES[bn]
        outs = small_outputs(tr, rows)[1:]
        tg = torch.tensor(targets).cuda()
        stats, per_row = pkg.evaluator.calc_loss(outs, tg, opt)
        np.testing.assert_allclose(per_row, g.t(f'small/{bn}/eval_rows').numpy(), rtol=2e-5, atol=1e-6)
        np.testing.assert_allclose([stats['cls_loss'], stats['reg_loss']], g.t(f'small/{bn}/eval_mean').numpy(), rtol=2e-5, atol=1e-6)
        if bn != 'b':
            assert per_row[1, 1] == 0.0                                  # [100.25, 100.75]: no positive point, reg 0 / max(0, 1)
        ref_form = tuple([tuple(p[l][i:i + 1] for l in range(C.SMALL['L'])) for i in range(len(rows))] for p in outs)
        stats2, per_row2 = pkg.evaluator.calc_loss((ref_form[0], ref_form[1], None, ref_form[2]), tg, opt)
        assert stats2 == stats and np.array_equal(per_row2, per_row)
