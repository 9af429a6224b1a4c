"""GPU checks of ``train.TrainStep(..., device_count=True)`` on the smallest model and batch of tests/test_gpu_train_step.py (fixture
s1, its builders imported) with the poisoned batch of tests/test_gpu_guard_step.py (one NaN in one clip's expert feature).

1. device_count=True on finite batches, three steps with the warm-up on (lr = 0, then the base lr): every tensor, every output and
   every ``p.grad`` has the bits of the default ``TrainStep`` -- with and without ``skip_nonfinite``, and for
   ``DataParallelTrainStep`` without a group.
2. skip_nonfinite=True, device_count=True over good, bad, good: every count read through ``state()`` is 1 after the skipped step and
   2 after the third (the default gives 2 and 3); the guard reports 2 applied, 1 skipped.  The third step equals, bit for bit in all
   tensors and outputs, the step a fresh DEFAULT ``TrainStep`` takes on the good batch after loading the ``state()`` taken after the
   skip -- a host count resumed at 1.  The default guarded run's third step does not equal them.
3. ``state()`` -> a fresh device_count=True step -> ``load_state`` -> one more step equals the uninterrupted run.

The conv-gradient word is consumed in a ``finally``, as tests/test_gpu_guard_step.py does.  Bit-exact throughout."""
import pytest
import torch

from conftest import load_pkg
from test_gpu_guard_step import batches, make_step, settle_conv_word
from test_gpu_train_step import batch_of, bits_differ, fixture, opt_of, state_of

pytestmark = pytest.mark.gpu
_default = {}


@pytest.fixture(scope='module')
def pkg():
    return load_pkg()


def warm_step(pkg, cls=None, **kw):
    """a step with the warm-up on: lr 0 at the first step, the base lr from the second on"""
    f = fixture('s1')
    return (cls or pkg.train.TrainStep)(f.model(pkg).cuda(), opt_of(pkg, f), itrs_per_epoch=1, **kw)


def counts(ts):
    return [float(s['step']) for s in ts.state()[1]['optimizer']['state'].values()]


def outputs(out):
    return {n: v.detach().cpu().clone() for n, v in out.items()}


def same_outputs(a, b):
    return sorted(a) == sorted(b) == ['cls', 'grad_norm', 'reg', 'total'] and all(torch.equal(a[n].view(torch.int32), b[n].view(torch.int32)) for n in a)


def three_steps(ts):
    batch, targets = batch_of(fixture('s1'))
    rows = []
    for _ in range(3):
        lr = ts.optimizer.param_groups[0]['lr']
        out = ts.step(batch, targets)
        rows.append((state_of(ts), outputs(out), [p.grad.detach().cpu().clone() for p in ts.model.parameters()], lr))
    return rows


def default_reference(pkg):
    """three steps of the default TrainStep, computed once and left unchanged"""
    if 'rows' not in _default:
        _default['rows'] = three_steps(warm_step(pkg))
    return _default['rows']


@pytest.mark.parametrize('kind', ['plain', 'guarded', 'data-parallel'])
def test_finite_batches_have_the_bits_of_the_default_step(pkg, kind):
    want = default_reference(pkg)
    assert [row[3] for row in want][0] == 0.0 and want[1][3] > 0.0, 'the warm-up is on: lr changes between the steps'
    if kind == 'data-parallel':
        ts = warm_step(pkg, pkg.train.DataParallelTrainStep, device_count=True)
        assert ts.world == 1
    else:
        ts = warm_step(pkg, skip_nonfinite=kind == 'guarded', device_count=True)
    assert ts.device_count is True and ts.optimizer.device_count is True
    got = three_steps(ts)
    for k, ((s, out, grads, lr), (ws, wout, wgrads, wlr)) in enumerate(zip(got, want)):
        assert lr == wlr and not bits_differ(s, ws), (k, bits_differ(s, ws)[:8])
        assert same_outputs(out, wout), k
        assert len(grads) == len(wgrads) and all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(grads, wgrads)), k
    assert counts(ts) == [3.0] * len(ts.optimizer.state) and ts.itr == 3
    if kind == 'guarded':
        rep = ts.guard.report()
        assert (rep['applied'], rep['skipped']) == (3, 0)


def test_a_skipped_step_holds_the_counts_back(pkg):
    batch, bad, targets = batches()
    try:
        ts = make_step(pkg, skip_nonfinite=True, device_count=True)
        ts.step(batch, targets)
        assert counts(ts) == [1.0] * len(ts.optimizer.state)
        s1 = state_of(ts)
        ts.step(bad, targets)
        assert not bits_differ(s1, state_of(ts)), 'a skipped step moved something'
        ckpt = ts.state()
        n = len(ckpt[1]['optimizer']['state'])
        assert n == len(list(ts.model.parameters())) and [float(s['step']) for s in ckpt[1]['optimizer']['state'].values()] == [1.0] * n
        assert ts.itr == 2 and ts.scheduler.last_epoch == 2, 'the scheduler and itr follow the attempts'
        third = outputs(ts.step(batch, targets))
        s3 = state_of(ts)
        assert counts(ts) == [2.0] * n
        rep = ts.guard.report()
        assert (rep['applied'], rep['skipped'], rep['last_skipped_attempt']) == (2, 1, 1)
        assert len({k for k, _ in bits_differ(s1, s3)}) == 4, 'the third step applied'

        resumed = make_step(pkg).load_state(*ckpt)         # a host count resumed at 1
        assert resumed.device_count is False and all(float(st['step']) == 1.0 for st in resumed.optimizer.state.values())
        out = outputs(resumed.step(batch, targets))
        assert not bits_differ(state_of(resumed), s3), bits_differ(state_of(resumed), s3)[:8]
        assert same_outputs(out, third)
        assert counts(resumed) == [2.0] * n

        default = make_step(pkg, skip_nonfinite=True)      # the count follows the attempts: 2 after the skip, 3 after the third
        default.step(batch, targets)
        default.step(bad, targets)
        assert counts(default) == [2.0] * n and not bits_differ(state_of(default), s1)
        default.step(batch, targets)
        assert counts(default) == [3.0] * n
        moved = {k for k, _ in bits_differ(state_of(default), s3)}
        assert {'p', 'ema'} <= moved, 'the default guarded run takes its third step with the corrections of count 3'
    finally:
        settle_conv_word(pkg)


def test_a_checkpoint_resumes_the_device_counts(pkg):
    batch, targets = batch_of(fixture('s1'))
    ts = warm_step(pkg, device_count=True)
    ts.step(batch, targets)
    ts.step(batch, targets)
    ckpt = ts.state()
    assert sorted(ckpt[1]) == ['epoch', 'itr', 'loss_norm', 'optimizer', 'scheduler'], 'no new key'
    want_out = outputs(ts.step(batch, targets))
    fresh = warm_step(pkg, device_count=True).load_state(*ckpt)
    assert fresh.optimizer._steps.tolist() == [2] * len(ckpt[1]['optimizer']['state'])
    out = outputs(fresh.step(batch, targets))
    assert not bits_differ(state_of(fresh), state_of(ts)) and same_outputs(out, want_out)
    assert counts(fresh) == counts(ts) == [3.0] * len(ts.optimizer.state)
