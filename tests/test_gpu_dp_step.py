"""GPU checks of the data-parallel training step (train.DataParallelTrainStep, dist.GradReducer) on fixture s1, with the helpers of
tests/test_gpu_train_step.py.

1. One process, no group: three steps (warmup_epochs = 0) give the bits of ``TrainStep`` in every parameter, both moments, the EMA
   copy, the returned losses and grad_norm, for bucket_bytes of 4 KiB (many buckets), 64 KiB and the default (one bucket); one
   micro-batch and two.  After a step every ``p.grad`` lies in the arena at its planned offset, and the optimizer's table was
   uploaded once in three steps.
2. A parameter that received no gradient is packed as zeros; a gradient that is a 4-byte aligned view is packed like any other.
3. Two REAL ranks on one card (two fresh processes of tests/dp_rank_main.py, gloo rendezvous, both on cuda:0; rank r takes video r;
   once with the default bucket size, one bucket, and once with 64 KiB, fourteen buckets reduced from inside the backward):
   (a) the ranks are bit-identical in every tensor after every step, (b) and bit-identical to a comparator built here from public
   pieces: both videos as micro-batches through training_forward + PointObjective(world_size=2) + backward(), p.grad.mul_(0.5),
   update_norm of the summed norm, grad_norm_and_coef, optimizer.step(clip_coef), the scheduler.  Why bits: halving is exact, a
   two-term sum commutes, the norm is summed in the table's order, which both sides share; the exactness premise (no non-zero
   gradient value below 2^-100) is asserted too.
4. The same over nccl (RCCL) with 64 KiB buckets, one card per rank, where there are two cards; skipped otherwise.

Every check prints a `DPSTEP` line."""
import os
import socket
import subprocess
import sys
import time

import pytest
import torch

from conftest import load_pkg
from test_gpu_optim import KINDS
from test_gpu_train_step import batch_of, bits_differ, fixture, opt_of, state_of

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
KIB = 1024
STEPS = 3
_single, _comparator = {}, {}


@pytest.fixture(scope='module')
def pkg():
    return load_pkg()


def make_step(pkg, cls, **kw):
    f = fixture('s1')
    opt = opt_of(pkg, f)
    opt.train.warmup_epochs = 0                                    # every step runs at the base lr
    return cls(f.model(pkg).cuda(), opt, itrs_per_epoch=1, **kw)


def micro_batches(micro):
    f = fixture('s1')
    if micro == 1:
        return batch_of(f)
    parts = [batch_of(f, [0]), batch_of(f, [1])]
    return [b for b, _ in parts], [t for _, t in parts]


def three_steps(ts, micro, after=None):
    batch, targets = micro_batches(micro)
    rows = []
    for k in range(STEPS):
        out = ts.step(batch, targets)
        if after is not None:
            after(k)
        rows.append((state_of(ts), {n: v.detach().cpu().clone() for n, v in out.items()}))
    return rows


def single_rank_reference(pkg, micro):
    """three steps of TrainStep, computed once per micro-batch count and left unchanged"""
    if micro not in _single:
        _single[micro] = three_steps(make_step(pkg, pkg.train.TrainStep), micro)
    return _single[micro]


@pytest.mark.parametrize('micro', [1, 2])
@pytest.mark.parametrize('bucket_bytes', [4 * KIB, 64 * KIB, None], ids=['4KiB', '64KiB', 'default'])
def test_without_a_group_it_is_the_single_rank_step(pkg, bucket_bytes, micro):
    want = single_rank_reference(pkg, micro)
    ts = make_step(pkg, pkg.train.DataParallelTrainStep, **({} if bucket_bytes is None else {'bucket_bytes': bucket_bytes}))
    assert ts.world == 1 and ts.objective.world_size == 1
    red = ts.reducer
    K = len(red.plan['buckets'])
    assert bucket_bytes is not None or (K == 1 and pkg.dist.DEFAULT_BUCKET_BYTES == 25 * KIB * KIB)
    assert bucket_bytes != 4 * KIB or K > 4
    named = [(n, p) for n, p in ts.model.named_parameters() if p.requires_grad]
    assert [p for _, p in named] == red.params

    def after(k):
        lo, hi = red.arena.data_ptr(), red.arena.data_ptr() + 4 * red.arena.numel()
        for (n, p), off in zip(named, red.offsets):
            assert p.grad is not None and p.grad.data_ptr() == lo + 4 * off and p.grad.data_ptr() + 4 * p.numel() <= hi and off % 64 == 0, n
            assert p.grad.shape == p.shape and p.grad.is_contiguous()
        assert sorted(red.launched) == list(range(K)) == red.launched, 'every bucket once, in index order'

    got = three_steps(ts, micro, after)
    assert ts.optimizer.table_uploads == 1, 'the gradients no longer move: one upload of the optimizer table in three steps'
    for k, ((s, out), (ws, wout)) in enumerate(zip(got, want)):
        bad = bits_differ(s, ws)
        assert not bad, (k, bad[:8])
        assert sorted(out) == sorted(wout) == ['cls', 'grad_norm', 'reg', 'total']
        for n in out:
            assert torch.equal(out[n].view(torch.int32), wout[n].view(torch.int32)), (k, n, out[n], wout[n])
    print(f'DPSTEP no group, bucket_bytes {bucket_bytes}, {micro} micro-batch(es): {K} buckets, {len(named)} tensors, {STEPS} steps: '
          f'p / exp_avg / exp_avg_sq / ema and cls / reg / total / grad_norm bit-identical to TrainStep; table uploads {ts.optimizer.table_uploads}')


def test_a_missing_gradient_is_packed_as_zeros_and_a_view_like_any_other(pkg):
    D = pkg.dist
    g = torch.Generator().manual_seed(3)
    ps = [torch.nn.Parameter(torch.randn(n, generator=g).cuda()) for n in (5, 4097, 70, 3)]
    frozen = torch.nn.Parameter(torch.randn(9, generator=g).cuda(), requires_grad=False)
    red = D.GradReducer(ps + [frozen], None, 4 * KIB)
    assert red.params == ps and len(red.plan['buckets']) == 3 and red.world == 1
    w = [torch.randn(p.numel(), generator=g).cuda() for p in ps]
    buf = torch.zeros(80, device='cuda')
    ps[2].grad = buf[1:71]                                         # accumulated into in place: the source is a view at 4 mod 16
    assert ps[2].grad.data_ptr() % 16 == 4
    red.arm()
    ((ps[0] * w[0]).sum() + (ps[1] * w[1]).sum() + (ps[2] * w[2]).sum()).backward()           # nothing reaches ps[3]
    red.disarm()
    assert ps[3].grad is None
    red.finalize()
    assert red.launched == [0, 1, 2]
    torch.cuda.synchronize()
    for i in (0, 1, 2):
        assert torch.equal(ps[i].grad, w[i]) and ps[i].grad.data_ptr() == red.views[i].data_ptr(), i
    assert ps[3].grad is not None and ps[3].grad.data_ptr() == red.views[3].data_ptr() and not bool(ps[3].grad.view(torch.int32).any())
    assert frozen.grad is None
    used = torch.zeros(red.arena.numel(), dtype=torch.bool)
    for p, off in zip(ps, red.offsets):
        used[off:off + p.numel()] = True
    assert not bool(red.arena.cpu()[~used].view(torch.int32).any()), 'the padding was zeroed once and stays zero'
    # the hooks are gone after disarm(): a further backward accumulates into the arena views and launches nothing
    red.launched = []
    (ps[0] * w[0]).sum().backward()
    assert red.launched == [] and torch.equal(ps[0].grad, w[0] + w[0])
    print(f'DPSTEP reducer alone: 4 tensors in {len(red.plan["buckets"])} buckets, one without a gradient -> +0, one source at 4 mod 16')


# ---------------------------------------------------------------------------------------------- two real ranks
def run_two_ranks(backend, out_dir, bucket_bytes=None, limit=240.0):
    """two fresh processes of dp_rank_main.py; the parent waits with a time limit and ends both when it runs out or when one fails.
    It does not start them again."""
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    env0 = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), WORLD_SIZE='2', PYTHONDONTWRITEBYTECODE='1')
    cmd = [sys.executable] + (['-s'] if sys.flags.no_user_site else []) + [os.path.join(HERE, 'dp_rank_main.py'), backend, str(out_dir)] + \
        ([] if bucket_bytes is None else [str(bucket_bytes)])
    logs = [open(os.path.join(out_dir, f'rank{r}.log'), 'w+') for r in range(2)]
    procs = [subprocess.Popen(cmd, env=dict(env0, RANK=str(r), LOCAL_RANK=str(r)), stdout=logs[r], stderr=subprocess.STDOUT, cwd=HERE)
             for r in range(2)]
    t0, why = time.time(), None
    try:
        while any(p.poll() is None for p in procs):
            if any(p.poll() not in (None, 0) for p in procs):
                why = 'a rank failed'
                break
            if time.time() - t0 > limit:
                why = f'no result after {limit:.0f} s'
                break
            time.sleep(0.05)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
            p.wait()
    tails = []
    for r, log in enumerate(logs):
        log.seek(0)
        tails.append(f'--- rank {r} (exit {procs[r].returncode}) ---\n' + log.read()[-3000:])
        log.close()
    assert why is None and all(p.returncode == 0 for p in procs), f'{why}\n' + '\n'.join(tails)
    return [torch.load(os.path.join(out_dir, f'rank{r}.pt')) for r in range(2)], time.time() - t0


def comparator(pkg):
    """one process doing both ranks' work, from public pieces (a TrainStep only holds the objective, the optimizer, the scheduler and
    the EMA copy; its step() is not called); computed once and left unchanged"""
    if 'steps' not in _comparator:
        _comparator['steps'] = _comparator_steps(pkg)
    return _comparator['steps']


def _comparator_steps(pkg):
    T, O = pkg.train, pkg.optim
    f = fixture('s1')
    ts = make_step(pkg, T.TrainStep, world_size=2)
    params = list(ts.model.parameters())
    parts = [batch_of(f, [0]), batch_of(f, [1])]
    steps = []
    for _ in range(STEPS):
        ts.optimizer.zero_grad(set_to_none=True)
        norm = None
        for batch, targets in parts:
            d = ts.objective(T.training_forward(ts.model, **batch), targets)
            d['total'].backward()
            norm = d['norm'] if norm is None else norm + d['norm']
        with torch.no_grad():
            for p in params:
                p.grad.mul_(0.5)
        ts.objective.update_norm(norm)
        gn, coef = O.grad_norm_and_coef(params, ts.clip_grad_norm)
        ts.optimizer.step(clip_coef=coef)
        ts.scheduler.step()
        steps.append({'state': state_of(ts), 'grads': [p.grad.detach().cpu().clone() for p in params], 'grad_norm': gn.detach().cpu().clone(),
                      'loss_norm': ts.objective.loss_norm})
    return steps


def same(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def check_two_ranks(pkg, backend, out_dir, bucket_bytes=None):
    ranks, seconds = run_two_ranks(backend, out_dir, bucket_bytes)
    r0, r1 = ranks
    assert r0['buckets'] == r1['buckets'] and r0['uploads'] == r1['uploads'] == 1
    assert r0['buckets'] == 1 if bucket_bytes is None else r0['buckets'] > 4
    n_t = len(r0['steps'][0]['grads'])
    # (a) the replicas stay bit-identical
    for k in range(STEPS):
        a, b = r0['steps'][k], r1['steps'][k]
        bad = bits_differ(a['state'], b['state']) + [('grad', i) for i, (u, v) in enumerate(zip(a['grads'], b['grads'])) if not same(u, v)]
        assert not bad, f'(a) step {k}: ranks 0 and 1 differ in {bad[:8]}'
        assert same(a['out']['grad_norm'], b['out']['grad_norm']) and a['loss_norm'] == b['loss_norm']
        assert a['launched'] == b['launched'] == list(range(r0['buckets']))
        assert not same(a['out']['total'], b['out']['total']), 'the returned losses are rank-local: two videos, two totals'
    print(f'DPSTEP {backend}, two ranks: (a) {STEPS} steps x ({len(KINDS)} x {n_t} state tensors + {n_t} gradients + grad_norm + loss_norm) '
          f'bit-identical between the ranks; {r0["buckets"]} bucket(s); {seconds:.1f} s for both processes')
    # (b) ... and they are what one process computes that does both ranks' work
    want = comparator(pkg)
    tiny = 0
    for k in range(STEPS):
        a, w = r0['steps'][k], want[k]
        for g in w['grads'] + a['grads']:
            tiny += int(((g != 0) & (g.abs() < 2.0 ** -100)).sum())
        bad = [('grad', i) for i, (u, v) in enumerate(zip(a['grads'], w['grads'])) if not same(u, v)] + bits_differ(a['state'], w['state'])
        print(f'DPSTEP {backend}, two ranks: (b) step {k}: {len(bad)} of {(len(KINDS) + 1) * n_t} tensors differ from the comparator; grad_norm '
              f'{float(a["out"]["grad_norm"])!r} against {float(w["grad_norm"])!r}; loss_norm {a["loss_norm"]!r} against {w["loss_norm"]!r}')
        assert not bad, f'(b) step {k}: rank 0 differs from the comparator in {bad[:8]}'
        assert same(a['out']['grad_norm'], w['grad_norm']) and a['loss_norm'] == w['loss_norm']
    assert tiny == 0, f'{tiny} non-zero gradient values below 2^-100: halving them is not exact'


@pytest.mark.parametrize('bucket_bytes', [None, 64 * KIB], ids=['default', '64KiB'])
def test_two_ranks_on_one_card_stay_identical_and_match_one_process(pkg, tmp_path, bucket_bytes):
    check_two_ranks(pkg, 'gloo', tmp_path, bucket_bytes)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason='RCCL needs one card per rank: fewer than two cards here')
def test_two_ranks_over_rccl(pkg, tmp_path):
    check_two_ranks(pkg, 'nccl', tmp_path, 64 * KIB)
