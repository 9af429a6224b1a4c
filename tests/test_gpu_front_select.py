"""GPU checks of selected-clip training (include/decafnet_hip_front_select.h, ``autograd.selected_vid_map``,
``train.training_forward(expert='selected')``, ``train.TrainStep(expert='selected')``) against the reference
(tests/golden/front_grad_<case>.npz; tests/golden/step_grad_<case>*.npz for the whole step).  The project's rule on every compared
tensor, forward values included:

    e_gpu <= max(4 * e_ref, 2^-21 * max |x_64|),   e = max |x - x_64|

x_64 the reference's fp64 yardstick, e_ref the error of its fp32 run; where a test makes its own operands, x_64 is the fp64 restatement
(tests/front_select_ref.py) and e_ref the error of the reference's dense formula evaluated by torch in fp32.  Every check prints an
`FSERR` line; the figures are in profiles/front_select.md."""
import pytest
import torch

from conftest import load_pkg
import front_grad_ref as R
import front_select_ref as FS
import step_grad_ref as S

pytestmark = pytest.mark.gpu
FLOOR = 2.0 ** -21


def check(tag, got, x64, x32=None, e_ref=None, top=None):
    got, x64 = got.detach().cpu().double(), x64.detach().double()
    assert got.shape == x64.shape, (tag, got.shape, x64.shape)
    assert bool(torch.isfinite(got).all()), tag
    top = float(x64.abs().max()) if top is None else top
    e_ref = float((x32.detach().double() - x64).abs().max()) if e_ref is None else e_ref
    e_gpu = float((got - x64).abs().max())
    bound = max(4 * e_ref, FLOOR * top)
    ok = e_gpu <= bound
    print(f'FSERR {tag}: max|x64| {top:.3e} e_ref {e_ref:.3e} e_gpu {e_gpu:.3e} bound {bound:.3e} ratio {e_gpu / bound if bound else 0.0:.3f}'
          f'{"" if ok else "  MISSED"}')
    return None if ok else (tag, e_gpu, bound)


@pytest.fixture(scope='module')
def pkg():
    return load_pkg()


_fixtures = {}


def fixture(name):
    if name not in _fixtures:
        _fixtures[name] = R.Fixture(name)
    return _fixtures[name]


def place(rows, half=False, offset=0, capacity=0, fill=0.0):
    """the packed rows on the GPU: fp32 or float16, `capacity` extra rows of `fill` behind them, the first element `offset` ELEMENTS
    past a 256-byte aligned allocation"""
    n, D = rows.shape
    dt = torch.float16 if half else torch.float32
    buf = torch.full((offset + (n + capacity) * D + 8,), fill, dtype=dt, device='cuda')
    view = buf[offset:offset + (n + capacity) * D].view(n + capacity, D)
    view[:n] = rows.to(dt).cuda()
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + offset * buf.element_size()
    return view


def run(pkg, ops, dY, rows=None, weight_grad=True, half=False):
    """one forward and backward of selected_vid_map; ops = (rows, row_first, pos, shallow, gate, mask, correl, sizes, W, bias) on the host,
    `rows` a placed GPU tensor in place of ops[0] -> (Y, dW (E, Cin) or None, db) on the GPU"""
    c = lambda z: None if z is None else z.cuda()
    r, first, pos, sh, gate, mask, correl, sizes, W, bias = ops
    w = torch.nn.Parameter(W[:, :, None].clone().float().cuda(), requires_grad=weight_grad)
    b = torch.nn.Parameter(bias.clone().float().cuda())
    feat = (lambda z: None if z is None else z.half().cuda()) if half else (lambda z: None if z is None else z.float().cuda())
    y = pkg.autograd.selected_vid_map(feat(r) if rows is None else rows, first, c(pos), feat(sh), c(gate.float()), c(mask), c(correl), sizes, w, b)
    y.backward(c(dY))
    return y.detach(), None if w.grad is None else w.grad[:, :, 0], b.grad


def fixture_ops(f):
    _, sh, gate, mask, correl, sizes, W, bias = f.operands(torch.float32)
    rows, first, pos, counts = FS.fixture_pack(f, torch.float32)
    assert counts == [96, 31]
    return (rows, first, pos, sh, gate, mask, correl, sizes, W, bias)


_base = {}


def base(pkg, name):
    if name not in _base:
        f = fixture(name)
        _base[name] = run(pkg, fixture_ops(f), f.dY)
    return _base[name]


def column_groups(D, msf, scat, cin):
    g = [('dW1', slice(0, D))]
    if msf:
        g.append(('dW2', slice(D, 2 * D)))
    if scat:
        g.append(('dw3', slice(cin - 1, cin)))
    return g


def integer_case():
    """the integer operands of the shared path's orientation test (nvid = 2, D = 64, T = 70, E = 96, sizes [2, 1], a padded tail) with
    the rows gathered by list -> (ops, dY, dense vid)"""
    nvid, D, T, E, sizes = 2, 64, 70, 96, [2, 1]
    t, d, e = torch.arange(T), torch.arange(D), torch.arange(E)
    vid = ((3 * d[None, :, None] + 5 * t[None, None, :] + 7 * torch.arange(nvid)[:, None, None]) % 11 - 4).float()
    shallow = ((2 * d[None, :, None] + 3 * t[None, None, :] + torch.arange(nvid)[:, None, None]) % 7 - 2).float()
    dY = ((5 * e[None, None, :] + 2 * t[None, :, None] + 3 * torch.arange(3)[:, None, None]) % 9 - 3).float()
    gate = ((t[None, :] // 8 + torch.arange(3)[:, None]) % 3 == 0).float()
    mask = torch.ones(3, T, dtype=torch.bool)
    mask[2, 50:] = False
    vid_masks = torch.stack([mask[0], mask[2]])
    correl = ((t[None, :] + 2 * torch.arange(3)[:, None]) % 5 - 2).float()
    W = ((e[:, None] + 2 * torch.arange(2 * D + 1)[None, :]) % 5 - 2).float()
    bias = (e % 3 - 1).float()
    rows, first, pos, _, counts = FS.pack(vid, gate, vid_masks, sizes)
    assert first[-1] % 8 != 0 and T % 64 != 0 and E % 64 != 0, first
    return (rows, first, pos, shallow, gate, mask, correl, sizes, W, bias), dY, vid


def grid_case():
    """E = 128, D = 64, T = 136, operands on the 2^-10 grid (the features within what binary16 holds exactly: |x| < 2), three videos of
    [2, 1, 1] queries: 29 rows (a boundary inside the first 32-row chunk of the packed rows), 24 rows, and ONE selected clip"""
    gen = torch.Generator().manual_seed(29)
    nvid, D, T, E, sizes = 3, 64, 136, 128, [2, 1, 1]
    grid = lambda *s, scale=1.0: torch.round(torch.randn(*s, generator=gen) * scale * 1024) / 1024
    vid, shallow = grid(nvid, D, T, scale=0.4).clamp(-1.9, 1.9), grid(nvid, D, T, scale=0.4).clamp(-1.9, 1.9)
    correl, W, bias = grid(4, T), grid(E, 2 * D + 1, scale=0.1), grid(E, scale=0.1)
    dY = torch.randn(4, T, E, generator=gen) * 1e-3
    gate = torch.zeros(4, T)
    gate[0, 8:21], gate[1, 16:37], gate[2, 70:94], gate[3, 5] = 1.0, 1.0, 1.0, 1.0
    mask = torch.ones(4, T, dtype=torch.bool)
    mask[2, 120:] = False
    vid_masks = torch.stack([mask[0], mask[2], mask[3]])
    rows, first, pos, _, counts = FS.pack(vid, gate, vid_masks, sizes)
    assert counts == [29, 24, 1] and first == [0, 29, 53, 54]
    assert torch.equal(vid.half().float(), vid) and torch.equal(shallow.half().float(), shallow)
    return (rows, first, pos, shallow, gate, mask, correl, sizes, W, bias), dY, vid


def yardsticks(ops, dY, vid):
    """(y64, dw64, db64) by the fp64 restatement on the packed rows, (y32, dw32, db32) by the reference's dense formula in fp32"""
    rows, first, pos, sh, gate, mask, correl, sizes, W, bias = ops
    d = lambda z: None if z is None else z.double()
    y64 = FS.selected_forward(d(rows), first, pos, d(sh), d(gate), mask, d(correl), sizes, d(W), d(bias))
    dw64, db64 = FS.selected_grads(d(rows), first, pos, d(sh), d(gate), mask, d(correl), sizes, d(dY))
    x32 = R.dense_input(vid, sh, gate, correl, sizes)
    return (y64, dw64, db64), (R.dense_forward(x32, mask, W, bias),) + tuple(R.dense_grads(x32, mask, dY))


# ---------------------------------------------------------------------------------------------- 1: orientation, exactly
def test_operand_orientation_on_exact_integer_data(pkg):
    """small integers with an asymmetric pattern: every product and every sum is exact in the fp16 planes and in fp32, so the result
    equals the integer answer of the DENSE formula bit for bit; a transposed or mirrored operand, or a row of another clip, cannot"""
    ops, dY, vid = integer_case()
    _, first, pos, sh, gate, mask, correl, sizes, W, bias = ops
    y, dw, db = run(pkg, ops, dY)
    d = lambda z: z.double()
    y64 = R.shared_forward(d(vid), d(sh), d(gate), mask, d(correl), sizes, d(W), d(bias))
    dw64, db64 = R.shared_grads(d(vid), d(sh), d(gate), mask, d(correl), sizes, d(dY))
    assert float(dw64.abs().max()) < 2 ** 24 and float(y64.abs().max()) < 2 ** 24
    assert torch.equal(y.cpu().double(), y64)
    assert torch.equal(dw.cpu().double(), dw64)
    assert torch.equal(db.cpu().double(), db64)


# ---------------------------------------------------------------------------------------------- 2: the fixture cases
@pytest.mark.parametrize('name', R.CASES)
def test_forward_and_gradients_meet_the_rule(pkg, name):
    f = fixture(name)
    y, dw, db = base(pkg, name)
    missed = [check(f'{name} Y', y, f.y64, f.y32), check(f'{name} db', db, f.db64, f.db32)]
    for tag, cols in column_groups(f.D, f.msf, f.scat, f.W.size(1)):
        missed.append(check(f'{name} {tag}', dw[:, cols], f.dw64[:, cols], f.dw32[:, cols]))
    missed = [m for m in missed if m is not None]
    assert not missed, missed


# ---------------------------------------------------------------------------------------------- 3: the split row-GEMM path
def test_the_split_row_gemm_path_and_a_video_of_one_clip(pkg):
    ops, dY, vid = grid_case()
    y, dw, db = run(pkg, ops, dY)
    (y64, dw64, db64), (y32, dw32, db32) = yardsticks(ops, dY, vid)
    missed = [check('split Y', y, y64, y32), check('split db', db, db64, db32)]
    for tag, cols in column_groups(64, True, True, 129):
        missed.append(check(f'split {tag}', dw[:, cols], dw64[:, cols], dw32[:, cols]))
    missed = [m for m in missed if m is not None]
    assert not missed, missed


# ---------------------------------------------------------------------------------------------- 4: bits
@pytest.mark.parametrize('name', R.CASES)
def test_fresh_runs_scaling_accumulation_and_the_capacity_rows(pkg, name):
    f = fixture(name)
    ops = fixture_ops(f)
    y0, dw0, db0 = base(pkg, name)
    y1, dw1, db1 = run(pkg, ops, f.dY)
    assert torch.equal(y0, y1) and torch.equal(dw0, dw1) and torch.equal(db0, db1)
    _, dw32, db32 = run(pkg, ops, f.dY * 32.0)
    assert torch.equal(dw32, dw0 * 32.0) and torch.equal(db32, db0 * 32.0)
    # NaN in the capacity rows beyond row_first[nvid] changes no bit
    y2, dw2, db2 = run(pkg, ops, f.dY, rows=place(ops[0], capacity=40, fill=float('nan')))
    assert torch.equal(y0, y2) and torch.equal(dw0, dw2) and torch.equal(db0, db2)
    # accumulate = 1 onto the first result gives exactly twice it
    lb = pkg._lib
    c = lambda z: None if z is None else z.cuda().contiguous()
    rows, first, pos, sh, gate, mask, correl, sizes, W, bias = ops
    dev = [c(rows), c(pos), c(sh), c(gate.float()), c(mask), c(correl), c(f.dY)]
    host_first, nq = torch.tensor(first, dtype=torch.int32), torch.tensor(sizes, dtype=torch.int32)
    dw, db = dw0.clone().contiguous(), db0.clone()
    lb.check(lb.lib().dcf_op_vidmap_selected_bwd(lb.ptr(dev[0]), lb.ptr(host_first), lb.ptr(dev[1]), lb.ptr(dev[2]), lb.ptr(dev[3]), lb.ptr(dev[4]),
                                                 lb.ptr(dev[5]), lb.ptr(nq), lb.ptr(dev[6]), lb.ptr(dw), lb.ptr(db), 2, f.D, f.T, f.E, 1,
                                                 lb.current_stream()), 'dcf_op_vidmap_selected_bwd')
    assert torch.equal(dw, dw0 * 2.0) and torch.equal(db, db0 * 2.0)


# ---------------------------------------------------------------------------------------------- 5: float16
@pytest.mark.parametrize('shape,offset', [('integer', 0), ('grid', 0), ('grid', 1)])
def test_a_float16_pair_gives_the_bits_of_the_fp32_operators(pkg, shape, offset):
    """rows / shallow as binary16 values (both cases hold only values binary16 has) against the same values as fp32: forward, dW and db
    bit for bit.  offset 1: the rows start 2 bytes past 16-byte alignment, so the weight gradient takes its 2-byte loads"""
    ops, dY, _ = integer_case() if shape == 'integer' else grid_case()
    assert torch.equal(ops[0].half().float(), ops[0]) and torch.equal(ops[3].half().float(), ops[3])
    want = run(pkg, ops, dY)
    rows = place(ops[0], half=True, offset=offset)
    assert rows.data_ptr() % 16 == 2 * offset
    got = run(pkg, ops, dY, rows=rows, half=True)
    assert all(torch.equal(a, b) for a, b in zip(got, want))


# ---------------------------------------------------------------------------------------------- 6: needs_input_grad, refusals
def test_a_frozen_weight_leaves_the_bias_its_bits_and_features_take_no_gradient(pkg):
    f = fixture('msf+scat')
    ops = fixture_ops(f)
    _, _, db0 = base(pkg, 'msf+scat')
    _, dw, db = run(pkg, ops, f.dY, weight_grad=False)
    assert dw is None and torch.equal(db, db0)
    rows, first, pos, sh, gate, mask, correl, sizes, W, bias = ops
    w, b = torch.nn.Parameter(W[:, :, None].cuda()), torch.nn.Parameter(bias.cuda())
    for bad in ('rows', 'shallow'):
        x = {'rows': rows.cuda(), 'shallow': sh.cuda()}
        x[bad] = x[bad].requires_grad_(True)
        with pytest.raises(ValueError, match='requires a gradient'):
            pkg.autograd.selected_vid_map(x['rows'], first, pos.cuda(), x['shallow'], gate.float().cuda(), mask.cuda(), correl.cuda(), sizes, w, b)


def test_shapes_outside_the_contract_fail_with_a_message(pkg):
    lb = pkg._lib
    z = torch.zeros(8192, device='cuda')
    pos = torch.zeros(64, dtype=torch.int32, device='cuda')
    m = torch.ones(4096, dtype=torch.bool, device='cuda')
    bad = [(1, 48, 64, 1, [1], [0, 1]), (1, 32, 48, 1, [1], [0, 1]), (1, 32, 1056, 1, [1], [0, 1]), (1, 32, 64, 1, [0], [0, 1]),
           (1, 32, 64, 0, [1], [0, 1]), (17, 32, 64, 1, [1] * 17, list(range(18))), (0, 32, 64, 1, [1], [0, 1]),
           (2, 32, 64, 2, [1, 1], [0, 1, 1]), (2, 32, 64, 2, [1, 1], [1, 2, 3]), (1, 32, 64, 2, [1], [0, 3])]
    for nvid, D, E, T, nq, first in bad:
        host_nq, host_first = torch.tensor(nq, dtype=torch.int32), torch.tensor(first, dtype=torch.int32)     # host arrays, held in names
        L = lb.lib()
        rcs = {'dcf_op_vidmap_selected': L.dcf_op_vidmap_selected(lb.ptr(z), lb.ptr(host_first), lb.ptr(pos), None, lb.ptr(z), lb.ptr(z), lb.ptr(z),
                                                                   lb.ptr(m), None, lb.ptr(host_nq), lb.ptr(z), nvid, D, T, E, lb.current_stream())}
        with pytest.raises(RuntimeError, match=r'dcf_op_vidmap_selected:'):
            lb.check(rcs['dcf_op_vidmap_selected'], 'fwd')
        for name in ('dcf_op_vidmap_selected_bwd', 'dcf_op_vidmap_selected_bwd_h'):
            rcs[name] = getattr(L, name)(lb.ptr(z), lb.ptr(host_first), lb.ptr(pos), None, lb.ptr(z), lb.ptr(m), None, lb.ptr(host_nq),
                                         lb.ptr(z), lb.ptr(z), None, nvid, D, T, E, 0, lb.current_stream())
            with pytest.raises(RuntimeError, match=name + ':'):
                lb.check(rcs[name], 'bwd')
        assert set(rcs.values()) == {-1}, (nvid, D, E, T, nq, first, rcs)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 7: the whole step
def _tapped(pkg, keep):
    """autograd.selected_vid_map wrapped: its output keeps its gradient, and the call's operands land in `keep`"""
    inner = pkg.autograd.selected_vid_map

    def tap(rows, row_first, pos, shallow, gate, mask, correl, *rest, **kw):
        y = inner(rows, row_first, pos, shallow, gate, mask, correl, *rest, **kw)
        y.retain_grad()
        keep.append(dict(y=y, mask=mask, correl=correl, rows=rows, row_first=list(row_first)))
        return y
    return inner, tap


@pytest.mark.parametrize('how', ['gather', 'expert_fn'])
@pytest.mark.parametrize('name', S.CASES)
def test_the_whole_step_on_selected_rows_matches_the_reference(pkg, name, how):
    import test_gpu_train_step as TS
    f = TS.fixture(name)
    model = f.model(pkg).cuda()
    batch, targets = TS.batch_of(f)
    calls, extra = [], {}
    if how == 'expert_fn':
        host = f.vid.clone()                                        # the "encoder": indexes a host copy, clip-major rows to the GPU

        def expert_fn(b, clips):
            assert clips.device.type == 'cpu' and clips.dtype == torch.int64 and bool((clips[1:] > clips[:-1]).all())
            calls.append(b)
            return host[b][:, clips].t().contiguous().cuda()
        batch = dict(batch, vid=None)
        extra = {'expert_fn': expert_fn}
    keep = []
    inner, tap = _tapped(pkg, keep)
    pkg.autograd.selected_vid_map = tap
    try:
        out = pkg.train.training_forward(model, **batch, expert='selected', **extra)
    finally:
        pkg.autograd.selected_vid_map = inner
    assert len(keep) == 1 and (how == 'gather' or calls == list(range(len(f.text_size))))
    # what the op was handed: the rows of the union of the fixture's gates AND the video mask, nothing dense
    _, first, _, _, counts = FS.pack(None, f.gate.float(), f.vid_masks, f.text_size)
    assert keep[0]['row_first'] == first and keep[0]['rows'].shape == (first[-1], f.vid.size(1)) and first[-1] < f.vid.size(0) * f.vid.size(2)
    total = pkg.loss.PointObjective(f.opt(pkg))(out, targets)['total']
    total.backward()
    missed = [check(f'{name} {how} total', total, f.total['64'], f.total['32']),
              check(f'{name} {how} tap/vid_map', keep[0]['y'], f.taps['64']['vid_map'], f.taps['32']['vid_map'])]
    seen = 0
    for k, p in model.named_parameters():
        assert p.grad is not None, k
        missed.append(check(f'{name} {how} {k}', p.grad, f.gp['64'][k], f.gp['32'][k], top=f.top(k)))
        seen += 1
    assert seen == f.meta['n_params'] == 252
    missed = [m for m in missed if m is not None]
    assert not missed, missed


# ---------------------------------------------------------------------------------------------- 8: the public step
def _scat_step(pkg, **kw):
    import test_gpu_train_step as TS
    f = TS.fixture('s2')
    opt = pkg.config.make_opt(**dict(f.opt_kwargs, scat=True))
    opt.train.center_sampling, opt.train.reg_loss = f.meta['center_sampling'], f.meta['reg_loss']
    opt.train.warmup_epochs = 0
    torch.manual_seed(20260)
    model = pkg.modeling.PtTransformerEarlyFusionIterative(opt, second_fusion=f.second_fusion).cuda()
    return f, model, pkg.train.TrainStep(model, opt, itrs_per_epoch=1, **kw)


def test_a_scat_model_trains_through_the_public_step_on_selected_rows(pkg):
    import test_gpu_train_step as TS
    f, model, ts = _scat_step(pkg, expert='selected')
    assert model.vid_map.conv.weight.shape[1] == 2 * f.vid.size(1) + 1 and ts.expert == 'selected'
    batch, targets = TS.batch_of(f)
    keep = []
    inner, tap = _tapped(pkg, keep)
    pkg.autograd.selected_vid_map = tap
    try:
        outs = [ts.step(batch, targets) for _ in range(2)]
    finally:
        pkg.autograd.selected_vid_map = inner
    assert len(keep) == 2 and all(bool(torch.isfinite(o['total'])) for o in outs)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    last = keep[-1]
    dY, m, c = last['y'].grad.cpu(), last['mask'].cpu(), last['correl'].cpu()
    assert float(dY.abs().max()) > 0 and float(c.abs().max()) > 0
    ref = {dt: (m.to(dt)[..., None] * c.to(dt)[..., None] * dY.to(dt)).sum((0, 1)) for dt in (torch.float64, torch.float32)}
    miss = check('s2+scat dw3 after two selected steps', model.vid_map.conv.weight.grad[:, -1, 0], ref[torch.float64], ref[torch.float32])
    assert miss is None, miss


def test_state_round_trip_on_selected_rows(pkg):
    import test_gpu_train_step as TS
    f = TS.fixture('s1')
    ts = pkg.train.TrainStep(f.model(pkg).cuda(), TS.opt_of(pkg, f), itrs_per_epoch=1, expert='selected')
    batch, targets = TS.batch_of(f)
    for _ in range(2):
        ts.step(batch, targets)
    fresh = pkg.train.TrainStep(f.model(pkg).cuda(), TS.opt_of(pkg, f), itrs_per_epoch=1, expert='selected')
    fresh.load_state(*ts.state())
    assert fresh.itr == 2 and fresh.expert == 'selected' and not TS.bits_differ(TS.state_of(fresh), TS.state_of(ts))
    a, b = ts.step(batch, targets), fresh.step(batch, targets)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not TS.bits_differ(TS.state_of(fresh), TS.state_of(ts))


def test_expert_dense_gives_the_bits_of_a_step_built_without_the_keyword(pkg):
    import test_gpu_train_step as TS
    f = TS.fixture('s1')
    batch, targets = TS.batch_of(f)
    steps = [pkg.train.TrainStep(f.model(pkg).cuda(), TS.opt_of(pkg, f), itrs_per_epoch=1, **kw) for kw in ({}, {'expert': 'dense'})]
    for _ in range(2):
        a, b = (ts.step(batch, targets) for ts in steps)
        assert all(torch.equal(a[k], b[k]) for k in a)
    assert not TS.bits_differ(TS.state_of(steps[0]), TS.state_of(steps[1]))
