"""GPU checks of the batch-assembly operator (dcf_op_assemble_rows, include/decafnet_hip_batch.h) and of the training data path on it.

1. The operator through the C ABI against torch slicing on the CPU, as integers (a copy has no tolerance), on ``out`` and ``mask``
   pre-filled with 0xFF bytes so that an unwritten byte shows: the cases of tests/batch_abi_cases.py.
2. The same cases between poisoned borders through tests/borders.run_case / arena.run_three_ways, with both fills: the bank, ``desc``,
   ``out`` and ``mask`` untouched outside, the clamped descriptors (n > T_out, n < 0) among them.
3. The refusals: non-zero, a message, nothing launched.
4. ``TrainLoader`` with a ``FeatureBank`` and with ``bank=None`` on the tree of tests/golden/train_data.npz: bit-identical batches and
   targets, in fp32 and with ``feature_dtype='stored'`` on float16 copies of the files.
5. ``TrainStep.step`` on the tiny model of tests/golden/step_grad_s2 (the ``config.make_opt`` sizes of tests/test_gpu_train_step.py)
   with ``front_end='shared'``, fed from the banked loader and from the host route: losses, grad_norm and every parameter bit for
   bit after each of two steps, the losses finite; then ``train.run_epoch`` against the same loop written out."""
import ctypes

import numpy as np
import pytest
import torch

import batch_abi_cases as C
import borders
import step_grad_ref as R
import train_data_tree as TT
from borders import ctx  # noqa: F401  (the module-scoped fixture)
from conftest import GOLDEN, load_pkg

pytestmark = pytest.mark.gpu
IDS = [c.tag for c in C.CASES]


def test_case_table_covers_the_pending_record():
    table = load_pkg()._lib.PENDING[0].table
    assert {c.export for c in C.CASES} | set(C.EXCLUDED) == set(table) and len(set(IDS)) == len(IDS)


@pytest.mark.parametrize('case', C.CASES, ids=IDS)
def test_operator_equals_torch_slicing(ctx, case):
    specs, call, _, verify = case.make()
    v = {}
    for name, t, role, *_ in specs:
        v[name] = t.cuda() if role == 'in' else torch.full(t.shape, 0xFF if t.dtype == torch.uint8 else -1, dtype=t.dtype, device='cuda')
    ctx.pkg._lib.check(call(ctx, v), case.export)
    torch.cuda.synchronize()
    verify(v)
    for name, t, role, *_ in specs:
        if role == 'in':
            assert torch.equal(v[name].cpu(), t), name


def _after(case, specs, plain, verify):
    verify(plain)


@pytest.mark.parametrize('case', C.CASES, ids=IDS)
def test_poisoned_borders(ctx, case):
    borders.run_case(ctx, case, _after)


def test_refusals_launch_nothing(ctx):
    lib, st, p = ctx.lib, ctx.stream(), C.p
    bank = torch.arange(64, dtype=torch.int32, device='cuda')
    desc = torch.tensor([[0, 4]], dtype=torch.int64, device='cuda')
    out = torch.full((4, 8), -1, dtype=torch.int32, device='cuda')
    mask = torch.full((1, 8), 0xFF, dtype=torch.uint8, device='cuda')
    a = dict(bank=p(bank), eb=4, desc=p(desc), B=1, C=4, T=8, out=p(out), mask=p(mask))
    odd = ctypes.c_void_p(bank.data_ptr() + 1)
    bad = [dict(eb=1), dict(eb=8), dict(eb=0), dict(B=0), dict(C=0), dict(T=0), dict(B=-1), dict(bank=None), dict(desc=None), dict(out=None),
           dict(bank=odd), dict(eb=2, out=ctypes.c_void_p(out.data_ptr() + 1))]
    for change in bad:
        k = dict(a, **change)
        rc = lib.dcf_op_assemble_rows(k['bank'], k['eb'], k['desc'], k['B'], k['C'], k['T'], k['out'], k['mask'], st)
        assert rc != 0, change
        msg = lib.dcf_last_error().decode()
        assert 'dcf_op_assemble_rows' in msg, (change, msg)
    torch.cuda.synchronize()
    assert bool((out == -1).all()) and bool((mask == 0xFF).all())
    assert lib.dcf_op_assemble_rows(a['bank'], 4, a['desc'], 1, 4, 8, a['out'], None, st) == 0          # mask is optional
    torch.cuda.synchronize()
    assert torch.equal(out[:, :4].cpu(), torch.arange(16, dtype=torch.int32).view(4, 4).t()) and bool((out[:, 4:] == 0).all())
    assert bool((mask == 0xFF).all())


# ---------------------------------------------------------------------------------------------- the loader
Z = np.load(f'{GOLDEN}/train_data.npz')
META = TT.js(Z, 'meta')


def same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and a.device == b.device, what
    assert torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8)), what


def same_batch(x, y, what):
    (bx, tx), (by, ty) = x, y
    assert set(bx) == set(by) == {'vid', 'shallow', 'vid_masks', 'tokens', 'text_cls', 'token_masks', 'text_size'}
    for k in bx:
        same_bits(bx[k], by[k], f'{what}: {k}')
    same_bits(tx, ty, f'{what}: targets')


@pytest.mark.parametrize('half', [False, True], ids=['fp32', 'stored-f16'])
def test_banked_loader_equals_the_host_route(tmp_path, half):
    D = load_pkg().data
    TT.write_tree(str(tmp_path), Z, half=half)
    cfg = TT.cfg_of(str(tmp_path), dict(META['configs']['crop'], feature_dtype='stored' if half else np.float32))
    make = lambda mode='same': D.VideoCentricTrainData(cfg, num_epochs=META['epochs'], seed=META['seed'], shallow_window=mode)
    tb, th = make(), make()
    bank = D.FeatureBank(tb)
    want = torch.float16 if half else torch.float32
    assert bank.data['vid'].dtype == bank.data['shallow'].dtype == want and bank.data['text'].dtype == torch.float32
    assert bank.data['vid'].is_cuda and bank.nbytes == sum(t.numel() * t.element_size() for t in list(bank.data.values()) + [bank.cls])
    kw = dict(input_vid_len=META['input_vid_len'], vid_stride=META['vid_stride'])
    banked, host = D.TrainLoader(tb, bank, 3, **kw), D.TrainLoader(th, None, 3, **kw)
    assert len(banked) == len(host) == len(tb) // 3
    seen = 0
    for e in range(META['epochs']):
        for k, (x, y) in enumerate(zip(banked.epoch(e), host.epoch(e))):
            same_batch(x, y, f'epoch {e} batch {k}')
            assert x[0]['vid'].dtype == want and x[0]['vid'].shape[1:] == (10, META['input_vid_len']) and x[1].dtype == torch.float32
            assert x[0]['vid_masks'].dtype == torch.bool and x[0]['tokens'].shape[1:] == (8, tb.max_text_len)
            seen += 1
    assert seen == META['epochs'] * len(banked)
    tb, th = make(), make()                                                   # micro-batches: lists, sliced alike
    banked, host = D.TrainLoader(tb, D.FeatureBank(tb), 4, microbatch_size=2, **kw), D.TrainLoader(th, None, 4, microbatch_size=2, **kw)
    for x, y in zip(banked.epoch(0), host.epoch(0)):
        assert len(x[0]) == len(x[1]) == len(y[0]) == 2
        for i in range(2):
            same_batch((x[0][i], x[1][i]), (y[0][i], y[1][i]), f'micro-batch {i}')
    tr = make('reference')                                                    # the reference's uncropped shallow stream of a long video
    with pytest.raises(ValueError, match='do not fit'):
        list(D.TrainLoader(tr, D.FeatureBank(tr), 3, **kw).epoch(0))


# ---------------------------------------------------------------------------------------------- the step
def test_two_steps_fed_from_the_bank_equal_the_host_route(tmp_path):
    pkg = load_pkg()
    D = pkg.data
    f = R.Fixture('s2')
    kw = f.opt_kwargs
    T, L, stride = 80, 9, kw['vid_stride']                                    # the fixture's own input length and token count
    arrays, data = TT.random_tree(5, 5, kw['D'], kw['text_in'], T, L)
    TT.write_tree(str(tmp_path), arrays)
    cfg = TT.cfg_of(str(tmp_path), data)
    runs = []
    for banked in (True, False):
        td = D.VideoCentricTrainData(cfg, num_epochs=2, seed=3)
        loader = D.TrainLoader(td, D.FeatureBank(td) if banked else None, len(td) // 2, input_vid_len=T, vid_stride=stride)
        assert len(loader) == 2
        opt = f.opt(pkg)
        opt.train.warmup_epochs = 1
        model = f.model(pkg).cuda()
        ts = pkg.train.TrainStep(model, opt, itrs_per_epoch=len(loader), front_end='shared')
        steps = [ts.step(b, t) for b, t in loader.epoch(0)]
        after_two = [p.detach().clone() for p in model.parameters()]
        if banked:
            sums = pkg.train.run_epoch(ts, loader, 1)
            assert ts.epoch == 2 and sums.pop('steps') == 2
        else:
            sums = {}
            for b, t in loader.epoch(1):
                for k, v in ts.step(b, t).items():
                    sums[k] = v if k not in sums else sums[k] + v
        assert ts.itr == 4
        runs.append((steps, after_two, sums, [p.detach().clone() for p in model.parameters()]))
    (sa, pa, ea, qa), (sb, pb, eb, qb) = runs
    for i, (x, y) in enumerate(zip(sa, sb)):
        assert set(x) == set(y) == {'cls', 'reg', 'total', 'grad_norm'}
        for k in x:
            same_bits(x[k], y[k], f'step {i}: {k}')
            assert bool(torch.isfinite(x[k]).all()), (i, k)
    moved = 0
    for i, (x, y, z) in enumerate(zip(pa, pb, f.model(pkg).parameters())):
        same_bits(x, y, f'parameter {i} after the second step')
        moved += not torch.equal(x.cpu(), z)
    assert moved > len(pa) // 2                                                # the steps did train
    assert set(ea) == set(eb)
    for k in ea:
        same_bits(ea[k], eb[k], f'run_epoch: {k}')
    for i, (x, y) in enumerate(zip(qa, qb)):
        same_bits(x, y, f'parameter {i} after run_epoch')
