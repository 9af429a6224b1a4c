"""GPU checks of the guarded training step (``train.TrainStep(..., skip_nonfinite=True)``) on the smallest model and batch of
tests/test_gpu_train_step.py (fixture s1, its builders imported).  The poisoned batch has one NaN in one clip's expert feature.

1. skip_nonfinite=True, three steps, the second poisoned: after it every parameter, moment and EMA tensor has the bits it had after
   the first; ``p.grad`` holds the NaN; the third step runs without raising and leaves everything finite and moved;
   ``guard.report(names)`` says 2 applied, 1 skipped (attempt 1) and names a parameter of the model; ``state()`` carries the counters.
2. skip_nonfinite=False, the same two steps: the parameters are non-finite after the second.  This is what the option exists to
   prevent.  Which of two things the unguarded step does is a race between the host and the conv-gradient word: if the word reaches
   the host while the backward is still being enqueued, a later conv gradient of the SAME backward fails with the one-shot error
   (the run stops there, with finite parameters); otherwise the update runs and every parameter is NaN.  The test takes either; in
   the first case it repeats the step with the word held back by an armed guard that nobody hands to the update, which is the second
   case made deterministic.  The word is consumed afterwards.
3. skip_nonfinite=True without a poisoned batch: three steps have the bits of skip_nonfinite=False in every tensor and every output.
4. Two real ranks (tests/guard_rank_main.py, gloo, both on cuda:0), only rank 1's share poisoned at the second step: both ranks skip
   that step and no other, and stay bit-identical."""
import math
import os
import socket
import subprocess
import sys
import time

import pytest
import torch

from conftest import load_pkg
from test_gpu_train_step import batch_of, bits_differ, fixture, opt_of, state_of

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = ('p', 'exp_avg', 'exp_avg_sq', 'ema')


@pytest.fixture(scope='module')
def pkg():
    return load_pkg()


def make_step(pkg, **kw):
    f = fixture('s1')
    opt = opt_of(pkg, f)
    opt.train.warmup_epochs = 0                                    # every step runs at the base lr
    return pkg.train.TrainStep(f.model(pkg).cuda(), opt, itrs_per_epoch=1, **kw)


def batches():
    """-> (batch, poisoned batch, targets): the poison is one NaN in the feature of clip 5 of video 0"""
    batch, targets = batch_of(fixture('s1'))
    bad = dict(batch, vid=batch['vid'].clone())
    bad['vid'][0, 3, 5] = float('nan')
    return batch, bad, targets


def finite(state):
    return all(bool(torch.isfinite(t).all()) for k in KINDS for t in state[k])


def settle_conv_word(pkg):
    """consume a pending one-shot failure of the conv-gradient exports, so that the tests that follow in this process find none"""
    lib, L = pkg._lib.lib(), pkg._lib
    X, dY, dW = torch.zeros(64, 32, device='cuda'), torch.zeros(64, 32, device='cuda'), torch.empty(32, 1, 32, device='cuda')
    for _ in range(2):
        torch.cuda.synchronize()
        lib.dcf_op_conv_bwd_weight(L.ptr(X), None, L.ptr(dY), L.ptr(dW), None, 1, 64, 32, 32, 1, 0, L.current_stream())
    torch.cuda.synchronize()


def test_a_poisoned_step_is_skipped_and_the_next_one_applies(pkg):
    ts = make_step(pkg, skip_nonfinite=True)
    batch, bad, targets = batches()
    names = [n for n, _ in ts.model.named_parameters()]
    try:
        assert isinstance(ts.guard, pkg.optim.StepGuard) and ts.state()[1]['guard'] == {'applied': 0, 'skipped': 0}
        ts.step(batch, targets)
        s1 = state_of(ts)
        assert finite(s1)
        out = ts.step(bad, targets)
        s2 = state_of(ts)
        assert not bits_differ(s1, s2), f'a skipped step moved {bits_differ(s1, s2)[:4]}'
        assert not math.isfinite(float(out['grad_norm'])) and float(ts.last_coef) == 0.0
        assert any(not bool(torch.isfinite(p.grad).all()) for p in ts.model.parameters()), 'p.grad keeps the offending gradient'
        assert not ts.guard.armed and ts.itr == 2 and ts.scheduler.last_epoch == 2
        rep = ts.guard.report(names)
        assert (rep['applied'], rep['skipped'], rep['last_skipped_attempt'], rep['verdict']) == (1, 1, 1, 1) and rep['first_bad'] in names
        out = ts.step(batch, targets)                              # does not raise: the conv-gradient word was consumed on the device
        s3 = state_of(ts)
        assert finite(s3) and math.isfinite(float(out['grad_norm'])) and float(ts.last_coef) > 0.0
        assert len({k for k, _ in bits_differ(s2, s3)}) == len(KINDS)
        rep = ts.guard.report(names)
        print(f'GUARDSTEP report after three steps: {rep}')
        assert (rep['applied'], rep['skipped'], rep['last_skipped_attempt'], rep['verdict']) == (2, 1, 1, 0)
        assert rep['first_bad'] in names and rep['n_bad_rows'] >= 1
        assert all(float(st['step']) == 3.0 for st in ts.optimizer.state.values()), 'the count follows the attempts'
        model_ckpt, state_ckpt = ts.state()
        assert state_ckpt['guard'] == {'applied': 2, 'skipped': 1}
        fresh = make_step(pkg, skip_nonfinite=True).load_state(model_ckpt, state_ckpt)
        rep = fresh.guard.report()
        assert (rep['applied'], rep['skipped'], rep['first_bad']) == (2, 1, None)
        assert 'guard' not in make_step(pkg).load_state(model_ckpt, state_ckpt).state()[1]
    finally:
        settle_conv_word(pkg)


def test_without_the_guard_the_same_step_destroys_the_parameters(pkg):
    ts = make_step(pkg)
    batch, bad, targets = batches()
    assert ts.guard is None and 'guard' not in ts.state()[1]
    try:
        ts.step(batch, targets)
        assert finite(state_of(ts))
        try:
            ts.step(bad, targets)
            raised = False
        except RuntimeError as e:                                  # the word reached the host while the backward was still being enqueued
            assert 'earlier gradient call' in str(e) and 'non-finite' in str(e), e
            raised = True
        print(f'GUARDSTEP unguarded poisoned step: {"raised inside its backward" if raised else "ran through"}')
        if raised:                                                 # the same step with the word held back: the update itself
            assert finite(state_of(ts))
            hold = pkg.optim.StepGuard('cuda').arm()
            try:
                ts.step(bad, targets)
            finally:
                hold.disarm()
        s2 = state_of(ts)
        assert all(not bool(torch.isfinite(t).any()) for t in s2['p']), 'every parameter is NaN after one non-finite gradient'
        assert not finite(s2)
    finally:
        settle_conv_word(pkg)


def test_the_guarded_step_has_the_unguarded_bits_on_finite_batches(pkg):
    plain, guarded = make_step(pkg), make_step(pkg, skip_nonfinite=True)
    batch, _, targets = batches()
    for k in range(3):
        a, b = plain.step(batch, targets), guarded.step(batch, targets)
        assert not bits_differ(state_of(plain), state_of(guarded)), k
        assert sorted(a) == sorted(b) and all(torch.equal(a[n], b[n]) for n in a), k
        assert torch.equal(plain.last_coef, guarded.last_coef)
        assert all(torch.equal(p.grad, q.grad) for p, q in zip(plain.model.parameters(), guarded.model.parameters()))
    rep = guarded.guard.report()
    assert (rep['applied'], rep['skipped'], rep['first_bad'], rep['last_skipped_attempt']) == (3, 0, None, -1)
    assert guarded.optimizer.table_uploads == plain.optimizer.table_uploads


# ---------------------------------------------------------------------------------------------- two real ranks
def run_two_ranks(out_dir, limit=240.0):
    """two fresh processes of guard_rank_main.py (gloo, both on cuda:0); the parent waits with a time limit and ends both when it runs
    out or when one fails.  It does not start them again."""
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    env0 = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), WORLD_SIZE='2', PYTHONDONTWRITEBYTECODE='1')
    cmd = [sys.executable] + (['-s'] if sys.flags.no_user_site else []) + [os.path.join(HERE, 'guard_rank_main.py'), 'gloo', str(out_dir)]
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
    return [torch.load(os.path.join(out_dir, f'rank{r}.pt')) for r in range(2)]


def test_two_ranks_reach_the_same_verdict_when_one_share_is_poisoned(pkg, tmp_path):
    """the verdict comes from the norm of the averaged gradient, which is the same on both ranks: no further collective"""
    r0, r1 = run_two_ranks(tmp_path)
    import dp_rank_main
    assert len(r0['steps']) == len(r1['steps']) == dp_rank_main.STEPS == 3
    for k, (a, b) in enumerate(zip(r0['steps'], r1['steps'])):
        assert not bits_differ(a['state'], b['state']), f'the ranks part at step {k}'
        assert torch.equal(a['grad_norm'].view(torch.int32), b['grad_norm'].view(torch.int32))
        assert a['report'] == b['report'], (k, a['report'], b['report'])
        assert math.isfinite(float(a['grad_norm'])) == (k != 1)
    reports = [s['report'] for s in r0['steps']]
    print(f'GUARDSTEP two ranks, rank 1 poisoned at step 1: {reports}')
    assert [(r['applied'], r['skipped'], r['verdict']) for r in reports] == [(1, 0, 0), (1, 1, 1), (2, 1, 0)]
    assert reports[2]['last_skipped_attempt'] == 1 and reports[2]['first_bad'] in r0['names']
    assert not bits_differ(r0['steps'][0]['state'], r0['steps'][1]['state']), 'the skipped step moved something'
    assert bits_differ(r0['steps'][1]['state'], r0['steps'][2]['state']) and finite(r0['steps'][2]['state'])
    assert r0['conv_flag_seen'] is False and r1['conv_flag_seen'] is True      # the word is rank-local; the verdict is not
