"""GPU checks of vid_map on shared products (include/decafnet_hip_front.h, ``autograd.gated_vid_map``,
``train.training_forward(front_end='shared')``) against the reference (tests/golden/front_grad_<case>.npz, make_golden_front_grad.py;
tests/golden/step_grad_<case>*.npz for the whole step).  The project's rule, unchanged, on every compared tensor, forward values
included:

    e_gpu <= max(4 * e_ref, 2^-21 * max |x_64|),   e = max |x - x_64|

x_64 the reference's fp64 yardstick, e_ref the error of its fp32 run.  Every check prints an `FGERR` line; the figures are in
profiles/front_grad.md."""
import pytest
import torch

from conftest import load_pkg
import front_grad_ref as R
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
    print(f'FGERR {tag}: max|x64| {top:.3e} e_ref {e_ref:.3e} e_gpu {e_gpu:.3e} bound {bound:.3e} ratio {e_gpu / bound if bound else 0.0:.3f}'
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


def run(pkg, f, skip=True, vid=None, dY=None, weight_grad=True):
    """one forward and backward of gated_vid_map on the fixture's operands -> (Y, dW (E, Cin) or None, db), on the GPU"""
    c = lambda z: None if z is None else z.cuda()
    v, sh, gate, mask, correl, sizes, W, bias = f.operands(torch.float32)
    w = torch.nn.Parameter(W[:, :, None].clone().cuda(), requires_grad=weight_grad)
    b = torch.nn.Parameter(bias.clone().cuda())
    y = pkg.autograd.gated_vid_map(c(v if vid is None else vid), c(sh), c(gate), c(mask), c(correl), sizes, w, b, skip=skip)
    y.backward(c(f.dY if dY is None else dY))
    return y.detach(), None if w.grad is None else w.grad[:, :, 0], b.grad


_base = {}


def base(pkg, name):
    if name not in _base:
        _base[name] = run(pkg, fixture(name))
    return _base[name]


def column_groups(f):
    g = [('dW1', slice(0, f.D))]
    if f.msf:
        g.append(('dW2', slice(f.D, 2 * f.D)))
    if f.scat:
        g.append(('dw3', slice(f.W.size(1) - 1, f.W.size(1))))
    return g


# ---------------------------------------------------------------------------------------------- 0: orientation, exactly
def test_operand_orientation_on_exact_integer_data(pkg):
    """small integers with an asymmetric pattern: every product and every sum is exact in the fp16 planes and in fp32, so the
    result equals the integer answer bit for bit; a transposed or mirrored operand of the weight-gradient kernel cannot"""
    nvid, D, T, E, sizes = 2, 64, 70, 96, [2, 1]
    t, d, e = torch.arange(T), torch.arange(D), torch.arange(E)
    vid = ((3 * d[None, :, None] + 5 * t[None, None, :] + 7 * torch.arange(nvid)[:, None, None]) % 11 - 4).float()
    shallow = ((2 * d[None, :, None] + 3 * t[None, None, :] + torch.arange(nvid)[:, None, None]) % 7 - 2).float()
    dY = ((5 * e[None, None, :] + 2 * t[None, :, None] + 3 * torch.arange(3)[:, None, None]) % 9 - 3).float()
    gate = ((t[None, :] // 8 + torch.arange(3)[:, None]) % 3 == 0).float()
    mask = torch.ones(3, T, dtype=torch.bool)
    mask[2, 50:] = False
    correl = ((t[None, :] + 2 * torch.arange(3)[:, None]) % 5 - 2).float()
    W = ((e[:, None] + 2 * torch.arange(2 * D + 1)[None, :]) % 5 - 2).float()
    bias = (e % 3 - 1).float()
    w, b = torch.nn.Parameter(W[:, :, None].cuda()), torch.nn.Parameter(bias.cuda())
    y = pkg.autograd.gated_vid_map(vid.cuda(), shallow.cuda(), gate.cuda(), mask.cuda(), correl.cuda(), sizes, w, b)
    y.backward(dY.cuda())
    y64 = R.shared_forward(vid.double(), shallow.double(), gate.double(), mask, correl.double(), sizes, W.double(), bias.double())
    dw64, db64 = R.shared_grads(vid.double(), shallow.double(), gate.double(), mask, correl.double(), sizes, dY.double())
    assert float(dw64.abs().max()) < 2 ** 24 and float(y64.abs().max()) < 2 ** 24
    assert torch.equal(y.detach().cpu().double(), y64)
    assert torch.equal(w.grad[:, :, 0].cpu().double(), dw64)
    assert torch.equal(b.grad.cpu().double(), db64)


def test_the_split_tile_path_of_the_forward_products(pkg):
    """E = 128, T % 4 == 0: the products run on the split tile kernel with the closed row tiles skipped (the fixtures' E = 64 takes the
    generic path).  Operands on the 2^-10 grid; the yardstick is the fp64 restatement, e_ref the error of the dense formula evaluated
    by torch in fp32 on the CPU; skip on / off and garbage in the closed tiles give equal bits."""
    gen = torch.Generator().manual_seed(23)
    nvid, D, T, E, sizes = 2, 64, 136, 128, [2, 1]
    grid = lambda *s, scale=1.0: torch.round(torch.randn(*s, generator=gen) * scale * 1024) / 1024
    vid, shallow, correl, W, bias = grid(nvid, D, T), grid(nvid, D, T), grid(3, T), grid(E, 2 * D + 1, scale=0.1), grid(E, scale=0.1)
    dY = torch.randn(3, T, E, generator=gen) * 1e-3
    gate = torch.zeros(3, T)
    gate[0, 8:24], gate[1, 16:40], gate[2, 70:94] = 1.0, 1.0, 1.0          # video 0: tiles 1 and 2 closed; video 1: tiles 0 and 2
    mask = torch.ones(3, T, dtype=torch.bool)
    mask[2, 120:] = False
    c = lambda z: z.cuda()

    def once(v, skip):
        w, b = torch.nn.Parameter(c(W[:, :, None].clone())), torch.nn.Parameter(c(bias.clone()))
        y = pkg.autograd.gated_vid_map(c(v), c(shallow), c(gate), c(mask), c(correl), sizes, w, b, skip=skip)
        y.backward(c(dY))
        return y.detach(), w.grad[:, :, 0], b.grad

    y, dw, db = once(vid, True)
    d = lambda z: z.double()
    y64 = R.shared_forward(d(vid), d(shallow), d(gate), mask, d(correl), sizes, d(W), d(bias))
    dw64, db64 = R.shared_grads(d(vid), d(shallow), d(gate), mask, d(correl), sizes, d(dY))
    x32 = R.dense_input(vid, shallow, gate, correl, sizes)
    y32, (dw32, db32) = R.dense_forward(x32, mask, W, bias), R.dense_grads(x32, mask, dY)
    missed = [check('split Y', y, y64, y32), check('split dW', dw, dw64, dw32), check('split db', db, db64, db32)]
    assert not [m for m in missed if m is not None], missed
    other = vid.clone()
    other[0, :, 64:], other[1, :, :64], other[1, :, 128:] = 777.0, -555.0, 3.0
    for got in (once(vid, False), once(other, True)):
        assert all(torch.equal(a, b) for a, b in zip(got, (y, dw, db)))


# ---------------------------------------------------------------------------------------------- 1: the fixture cases
@pytest.mark.parametrize('name', R.CASES)
def test_forward_and_gradients_meet_the_rule(pkg, name):
    f = fixture(name)
    y, dw, db = base(pkg, name)
    missed = [check(f'{name} Y', y, f.y64, f.y32), check(f'{name} db', db, f.db64, f.db32)]
    for tag, cols in column_groups(f):
        missed.append(check(f'{name} {tag}', dw[:, cols], f.dw64[:, cols], f.dw32[:, cols]))
    missed = [m for m in missed if m is not None]
    assert not missed, missed


# ---------------------------------------------------------------------------------------------- 2: the dense path, same yardstick
@pytest.mark.parametrize('name', ['msf', 'nomsf'])
def test_masked_conv1d_on_the_materialised_input_meets_the_same_rule(pkg, name):
    f = fixture(name)
    v, sh, gate, mask, correl, sizes, W, bias = f.operands(torch.float32)
    x = R.dense_input(v, sh, gate, correl, sizes).cuda()
    w, b = torch.nn.Parameter(W[:, :, None].clone().cuda()), torch.nn.Parameter(bias.clone().cuda())
    y = pkg.autograd.masked_conv1d(x, mask.cuda(), w, b)
    y.backward(f.dY.cuda())
    missed = [check(f'{name} dense Y', y, f.y64, f.y32), check(f'{name} dense db', b.grad, f.db64, f.db32)]
    for tag, cols in column_groups(f):
        missed.append(check(f'{name} dense {tag}', w.grad[:, cols, 0], f.dw64[:, cols], f.dw32[:, cols]))
    missed = [m for m in missed if m is not None]
    assert not missed, missed


# ---------------------------------------------------------------------------------------------- 3: skipping changes no bit
@pytest.mark.parametrize('name', R.CASES)
def test_skipping_and_the_content_of_closed_tiles_change_no_bit(pkg, name):
    f = fixture(name)
    y0, dw0, db0 = base(pkg, name)
    y1, dw1, db1 = run(pkg, f, skip=False)
    assert torch.equal(y0, y1) and torch.equal(dw0, dw1) and torch.equal(db0, db1)
    closed = f.closed_tiles()
    assert closed
    vid = f.vid.clone()
    for b, t0, t1 in closed:
        vid[b, :, t0:t1] = 1000.0 - 3.0 * vid[b, :, t0:t1]
    assert not torch.equal(vid, f.vid)
    y2, dw2, db2 = run(pkg, f, vid=vid)
    assert torch.equal(y0, y2) and torch.equal(dw0, dw2) and torch.equal(db0, db2)


# ---------------------------------------------------------------------------------------------- 4: bits
@pytest.mark.parametrize('name', R.CASES)
def test_fresh_runs_scaling_and_accumulation(pkg, name):
    f = fixture(name)
    y0, dw0, db0 = base(pkg, name)
    y1, dw1, db1 = run(pkg, f)
    assert torch.equal(y0, y1) and torch.equal(dw0, dw1) and torch.equal(db0, db1)
    _, dw32, db32 = run(pkg, f, dY=f.dY * 32.0)
    assert torch.equal(dw32, dw0 * 32.0) and torch.equal(db32, db0 * 32.0)
    # accumulate = 1 onto the first result gives exactly twice it
    lb = pkg._lib
    c = lambda z: None if z is None else z.cuda().contiguous()
    v, sh, gate, mask, correl, sizes, W, bias = f.operands(torch.float32)
    ops = [c(v), c(sh), c(gate), c(mask), c(correl), c(f.dY)]
    nq = torch.tensor(sizes, dtype=torch.int32)
    dw, db = dw0.clone().contiguous(), db0.clone()
    lb.check(lb.lib().dcf_op_vidmap_shared_bwd(lb.ptr(ops[0]), lb.ptr(ops[1]), lb.ptr(ops[2]), lb.ptr(ops[3]), lb.ptr(ops[4]), lb.ptr(nq),
                                               lb.ptr(ops[5]), lb.ptr(dw), lb.ptr(db), 2, f.D, f.T, f.E, 0, 1, lb.current_stream()),
             'dcf_op_vidmap_shared_bwd')
    assert torch.equal(dw, dw0 * 2.0) and torch.equal(db, db0 * 2.0)


# ---------------------------------------------------------------------------------------------- 5: needs_input_grad
def test_a_frozen_weight_leaves_the_bias_its_bits_and_features_take_no_gradient(pkg):
    f = fixture('msf+scat')
    _, _, db0 = base(pkg, 'msf+scat')
    _, dw, db = run(pkg, f, weight_grad=False)
    assert dw is None and torch.equal(db, db0)
    v, sh, gate, mask, correl, sizes, W, bias = f.operands(torch.float32)
    w, b = torch.nn.Parameter(W[:, :, None].cuda()), torch.nn.Parameter(bias.cuda())
    for bad in ('vid', 'shallow'):
        ops = {'vid': v.cuda(), 'shallow': sh.cuda()}
        ops[bad] = ops[bad].requires_grad_(True)
        with pytest.raises(ValueError, match='requires a gradient'):
            pkg.autograd.gated_vid_map(ops['vid'], ops['shallow'], gate.cuda(), mask.cuda(), correl.cuda(), sizes, w, b)


def test_shapes_outside_the_contract_fail_with_a_message(pkg):
    lb = pkg._lib
    z = torch.zeros(4096, device='cuda')
    m = torch.ones(4096, dtype=torch.bool, device='cuda')
    for D, E, nq in ((48, 64, [1]), (32, 48, [1]), (32, 64, [0])):
        host_nq = torch.tensor(nq, dtype=torch.int32)          # held in a name: the library reads this host array during the call
        rc = lb.lib().dcf_op_vidmap_shared(lb.ptr(z), None, lb.ptr(z), lb.ptr(z), lb.ptr(z), lb.ptr(m), None, lb.ptr(host_nq),
                                           lb.ptr(z), 1, D, 1, E, 0, lb.current_stream())
        assert rc == -1
        with pytest.raises(RuntimeError, match='dcf_op_vidmap_shared'):
            lb.check(rc, 'dcf_op_vidmap_shared')


# ---------------------------------------------------------------------------------------------- 6: the whole step
def _tapped(pkg, keep):
    """autograd.gated_vid_map wrapped: its output keeps its gradient, and the call's output / mask / correl land in `keep`"""
    inner = pkg.autograd.gated_vid_map

    def tap(vid, shallow, gate, mask, correl, *rest, **kw):
        y = inner(vid, shallow, gate, mask, correl, *rest, **kw)
        y.retain_grad()
        keep.append(dict(y=y, mask=mask, correl=correl))
        return y
    return inner, tap


@pytest.mark.parametrize('name', S.CASES)
def test_the_whole_step_on_the_shared_front_end_matches_the_reference(pkg, name):
    import test_gpu_train_step as TS
    f = TS.fixture(name)
    model = f.model(pkg).cuda()
    batch, targets = TS.batch_of(f)
    keep = []
    inner, tap = _tapped(pkg, keep)
    pkg.autograd.gated_vid_map = tap
    try:
        out = pkg.train.training_forward(model, **batch, front_end='shared')
    finally:
        pkg.autograd.gated_vid_map = inner
    assert len(keep) == 1
    total = pkg.loss.PointObjective(f.opt(pkg))(out, targets)['total']
    total.backward()
    missed = [check(f'{name} total', total, f.total['64'], f.total['32']),
              check(f'{name} tap/vid_map', keep[0]['y'], f.taps['64']['vid_map'], f.taps['32']['vid_map'])]
    seen = 0
    for k, p in model.named_parameters():
        assert p.grad is not None, k
        missed.append(check(f'{name} {k}', p.grad, f.gp['64'][k], f.gp['32'][k], top=f.top(k)))
        seen += 1
    assert seen == f.meta['n_params'] == 252
    missed = [m for m in missed if m is not None]
    assert not missed, missed


# ---------------------------------------------------------------------------------------------- 7: scat through the public step
def test_a_scat_model_trains_through_the_public_step(pkg):
    import test_gpu_train_step as TS
    f = TS.fixture('s2')
    opt = pkg.config.make_opt(**dict(f.opt_kwargs, scat=True))
    opt.train.center_sampling, opt.train.reg_loss = f.meta['center_sampling'], f.meta['reg_loss']
    opt.train.warmup_epochs = 0
    torch.manual_seed(20260)
    model = pkg.modeling.PtTransformerEarlyFusionIterative(opt, second_fusion=f.second_fusion).cuda()
    assert model.vid_map.conv.weight.shape[1] == 2 * f.vid.size(1) + 1
    ts = pkg.train.TrainStep(model, opt, itrs_per_epoch=1)                 # 'dense' asked for: a scat model takes the shared path anyway
    batch, targets = TS.batch_of(f)
    keep = []
    inner, tap = _tapped(pkg, keep)
    pkg.autograd.gated_vid_map = tap
    try:
        outs = [ts.step(batch, targets) for _ in range(2)]
    finally:
        pkg.autograd.gated_vid_map = inner
    assert len(keep) == 2 and all(bool(torch.isfinite(o['total'])) for o in outs)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    last = keep[-1]
    dY, m, c = last['y'].grad.cpu(), last['mask'].cpu(), last['correl'].cpu()
    assert float(dY.abs().max()) > 0 and float(c.abs().max()) > 0
    ref = {dt: (m.to(dt)[..., None] * c.to(dt)[..., None] * dY.to(dt)).sum((0, 1)) for dt in (torch.float64, torch.float32)}
    miss = check('s2+scat dw3 after two steps', model.vid_map.conv.weight.grad[:, -1, 0], ref[torch.float64], ref[torch.float32])
    assert miss is None, miss


# ---------------------------------------------------------------------------------------------- 8: state round trip
def test_state_round_trip_on_the_shared_front_end(pkg):
    import test_gpu_train_step as TS
    f = TS.fixture('s1')
    ts = pkg.train.TrainStep(f.model(pkg).cuda(), TS.opt_of(pkg, f), itrs_per_epoch=1, front_end='shared')
    batch, targets = TS.batch_of(f)
    for _ in range(2):
        ts.step(batch, targets)
    fresh = pkg.train.TrainStep(f.model(pkg).cuda(), TS.opt_of(pkg, f), itrs_per_epoch=1, front_end='shared')
    fresh.load_state(*ts.state())
    assert fresh.itr == 2 and fresh.front_end == 'shared' and not TS.bits_differ(TS.state_of(fresh), TS.state_of(ts))
    a, b = ts.step(batch, targets), fresh.step(batch, targets)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not TS.bits_differ(TS.state_of(fresh), TS.state_of(ts))
