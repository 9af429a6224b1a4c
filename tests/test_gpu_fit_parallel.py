"""GPU checks of ``train.fit_parallel``: ``Trainer.run`` on a process group, with sharded evaluation, the validation loss on the device and
skips agreed over the ranks.  The set-up is tests/fit_setup.py (model s2, generated trees, T = 80).

One rank (this process):
1. ``fit_parallel`` on a world-1 ``TrainStep`` writes the files of ``fit`` and leaves the same tensor and metric bits; with
   ``val_loss=True`` the report gains the loss line and the results the losses, and nothing else changes.

Two REAL ranks on one card -- ONE launch of two fresh processes of tests/fit_rank_main.py (gloo, both on cuda:0, a tree with two steps
per epoch per rank) serves every test below; the parent waits with a time limit, ends both when one fails and starts nothing again:
2. (a) two epochs with ``eval_run=1, val_loss=True``: parameters, EMA copy and optimizer state bit-equal over the ranks, equal result
   lists, rank 1 made no ``torch.save`` call and wrote no file, the evaluation shares disjoint, covering and equal to ``assign_units``,
   the metrics those of ``GroundingEvaluator.from_checkpoint(root, '2-4')`` on the host route, the loss row table bit-equal to the
   parent's and the losses within (N + V) * 2^-52, the report file ``report()`` plus the loss line.
3. (b) one epoch, then fresh objects with ``resume=True`` to two epochs: the tensors and results of (a).
4. (c) ``agree_skips=True``: rank 1 alone raises the conv-gradient word at step 1 (finite gradients); both ranks skip that step, stay
   bit-equal after every step, rank 0's ``conv_flag`` holds the remote bit.  With ``agree_skips=False`` the same three steps leave the
   ranks different after step 1: the hole the option closes, and the proof that this test can fail."""
import os
import signal
import socket
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import fit_setup as S
from conftest import load_pkg

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def pkg():
    return load_pkg()


# ---------------------------------------------------------------------------------------------- one rank
def test_one_rank_is_fit(pkg, tmp_path_factory):
    T = pkg.train
    f, cfg, ed, bank = S.build_world(pkg, str(tmp_path_factory.mktemp('tree')))
    roots = [str(tmp_path_factory.mktemp(n)) for n in ('fit', 'parallel', 'loss')]
    kw = dict(num_epochs=2, eval_data=bank, eval_by='epoch', eval_run=1)
    ts, loader = S.make_step(pkg, f, cfg)
    want = T.fit(ts, loader, roots[0], **kw)
    want_t = S.tensors(ts)
    ts, loader = S.make_step(pkg, f, cfg)
    got = T.fit_parallel(ts, loader, roots[1], **kw)
    assert not S.differing(S.tensors(ts), want_t)
    assert [tuple(r)[:2] for r in got] == [r[:2] for r in want] == [(1, 2), (2, 4)] and all(r.loss is None for r in got)
    assert all(np.array_equal(r.metrics, w[2]) for r, w in zip(got, want))
    listing = lambda root: sorted(os.path.relpath(os.path.join(d, n), root) for d, _, names in os.walk(root) for n in names)
    assert listing(roots[1]) == listing(roots[0]) and len(listing(roots[0])) == 6
    for name in listing(roots[0]):
        if name.endswith('.txt'):
            assert open(os.path.join(roots[1], name)).read() == open(os.path.join(roots[0], name)).read(), name
    ts, loader = S.make_step(pkg, f, cfg)
    lossy = T.fit_parallel(ts, loader, roots[2], val_loss=True, **kw)
    assert not S.differing(S.tensors(ts), want_t) and all(np.array_equal(r.metrics, w[2]) for r, w in zip(lossy, want))
    for r in lossy:
        assert set(r.loss) == {'cls_loss', 'reg_loss'} and all(isinstance(v, float) and v > 0 for v in r.loss.values())
        plain = open(os.path.join(roots[0], f'eval_{r.epoch}_{r.itr}.txt')).read()
        assert open(os.path.join(roots[2], f'eval_{r.epoch}_{r.itr}.txt')).read() == \
            plain + f"cls_loss: {r.loss['cls_loss']:.3f}; reg_loss: {r.loss['reg_loss']:.3f}; "


# ---------------------------------------------------------------------------------------------- two real ranks
def run_two_ranks(out_dir, tree, limit=420.0):
    """two fresh processes of fit_rank_main.py; the parent waits with a time limit and ends both when it runs out or when one fails.
    It does not start them again."""
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    env0 = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), WORLD_SIZE='2', PYTHONDONTWRITEBYTECODE='1')
    cmd = ['timeout', '-k', '10', str(int(limit) + 30), sys.executable] + (['-s'] if sys.flags.no_user_site else []) + \
        [os.path.join(HERE, 'fit_rank_main.py'), 'gloo', str(out_dir), str(tree)]
    logs = [open(os.path.join(out_dir, f'rank{r}.log'), 'w+') for r in range(2)]
    procs = [subprocess.Popen(cmd, env=dict(env0, RANK=str(r), LOCAL_RANK=str(r)), stdout=logs[r], stderr=subprocess.STDOUT, cwd=HERE,
                              start_new_session=True) for r in range(2)]
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
                try:
                    os.killpg(p.pid, signal.SIGKILL)                  # `timeout` and the rank under it
                except ProcessLookupError:
                    pass
            p.wait()
    tails = []
    for r, log in enumerate(logs):
        log.seek(0)
        tails.append(f'--- rank {r} (exit {procs[r].returncode}) ---\n' + log.read()[-3000:])
        log.close()
    assert why is None and all(p.returncode == 0 for p in procs), f'{why}\n' + '\n'.join(tails)
    return [torch.load(os.path.join(out_dir, f'rank{r}.pt'), weights_only=False) for r in range(2)], time.time() - t0


@pytest.fixture(scope='module')
def ranks(pkg, tmp_path_factory):
    """the ONE launch: (world of the parent, out_dir, [what rank 0 saved, what rank 1 saved])"""
    tree, out_dir = str(tmp_path_factory.mktemp('tree')), str(tmp_path_factory.mktemp('ranks'))
    world = S.build_world(pkg, tree, S.N_VIDEOS_TWO_RANKS)
    saved, seconds = run_two_ranks(out_dir, tree)
    print(f'FITPAR two ranks, three scenarios: {seconds:.1f} s for both processes')
    return world, out_dir, saved


def same_results(a, b):
    assert len(a) == len(b) > 0
    for x, y in zip(a, b):
        assert x[:2] == y[:2] and np.array_equal(x[2], y[2]) and x[3] == y[3], (x, y)


def test_two_epochs_with_sharded_evaluation_and_validation_loss(pkg, ranks):
    (f, cfg, ed, bank), out_dir, (r0, r1) = ranks
    a0, a1 = r0['a'], r1['a']
    assert a0['epoch_itr'] == a1['epoch_itr'] == (2, 4)
    assert not S.differing(a0['tensors'], a1['tensors']), 'the ranks parted'
    same_results(a0['results'], a1['results'])
    assert [r[:2] for r in a0['results']] == [(1, 2), (2, 4)]
    # rank 0 alone saves and writes
    root = os.path.join(out_dir, 'a')
    assert a1['log']['saves'] == [] and a1['log']['writes'] == []
    assert len(a0['log']['saves']) == 6 and sorted(os.path.basename(p) for p in a0['log']['writes']) == ['eval_1_2.txt', 'eval_2_4.txt']
    assert sorted(os.listdir(os.path.join(root, 'models'))) == ['1-2.pth', '2-4.pth', 'last.pth']
    # the shares
    index = list(bank.index)
    clips = [bank.rows['vid'][k][1] for k in index]
    want = [[index[i] for i in share] for share in pkg.dist.assign_units(clips, 2)]
    for e in range(2):
        s0, s1 = a0['log']['evaluated'][e], a1['log']['evaluated'][e]
        assert [s0, s1] == want and not set(s0) & set(s1) and sorted(s0 + s1) == sorted(index)
    # one model, one evaluation: the host route on rank 0's checkpoint
    opt = S.make_opt(pkg, f)
    ev = pkg.evaluator.GroundingEvaluator.from_checkpoint(opt, root, ckpt='2-4')
    host = ev.run(ed, counter=pkg.evaluator.RecallCounter(opt['eval']['ranks'], opt['eval']['iou_threshs']))
    epoch2 = a0['results'][1]
    print('FITPAR epoch 2 metrics', epoch2[2].tolist(), 'of', host.n_queries, 'losses', epoch2[3])
    assert host.n_queries == bank.meta.shape[0] and np.array_equal(epoch2[2], host.metrics())
    rows, _, stats = S.host_loss(pkg, ev, ed, opt)
    for r in (r0, r1):
        table = r['a']['log']['rows'][1]
        assert torch.equal(table.view(torch.int32), rows.view(torch.int32)), 'the reduced loss row table'
    bound = S.loss_bound(bank)
    for k in ('cls_loss', 'reg_loss'):
        err = abs(epoch2[3][k] - stats[k]) / stats[k]
        print(f'FITPAR {k}: two ranks {epoch2[3][k]!r} host {stats[k]!r} relative {err:.3g} bound {bound:.3g}')
        assert err <= bound, k
    line = f"cls_loss: {epoch2[3]['cls_loss']:.3f}; reg_loss: {epoch2[3]['reg_loss']:.3f}; "
    assert open(os.path.join(root, 'eval_2_4.txt')).read() == host.report() + line


def test_resume_continues_the_uninterrupted_run(ranks):
    _, _, (r0, r1) = ranks
    for r in (r0, r1):
        assert r['b']['epoch_itr'] == (2, 4)
        assert not S.differing(r['b']['tensors'], r0['a']['tensors']), 'resumed and uninterrupted'
        same_results(r['b']['results'], r0['a']['results'])


def test_skips_are_agreed_over_the_ranks(ranks):
    _, _, (r0, r1) = ranks
    REMOTE = r0['remote']
    agree0, agree1 = r0['c']['agree'], r1['c']['agree']
    assert len(agree0) == len(agree1) == 3
    for k, (x, y) in enumerate(zip(agree0, agree1)):
        assert not S.differing(x['tensors'], y['tensors']), f'the ranks part at step {k}'
        assert x['finite_grads'] and y['finite_grads'], 'the real gradients stay finite'
        assert (x['report']['verdict'], y['report']['verdict']) == ((1, 1) if k == 1 else (0, 0)), k
    assert [(s['report']['applied'], s['report']['skipped']) for s in agree0] == [(1, 0), (1, 1), (2, 1)]
    assert [(s['report']['applied'], s['report']['skipped']) for s in agree1] == [(1, 0), (1, 1), (2, 1)]
    assert agree0[1]['report']['conv_flag'] == REMOTE and agree1[1]['report']['conv_flag'] == 1 | REMOTE
    # Adam's host-side step counts follow attempts (train.py, "The guarded step"): they are the one-element tensors that advance
    moved = [i for i in S.differing(agree0[0]['tensors'], agree0[1]['tensors']) if agree0[0]['tensors'][i].numel() > 1]
    assert agree0[1]['report']['first_bad'] is None and not moved, 'the skipped step moved something'
    assert S.differing(agree0[1]['tensors'], agree0[2]['tensors'])
    # the hole: without the agreement rank 1 skips alone
    alone0, alone1 = r0['c']['alone'], r1['c']['alone']
    assert not S.differing(alone0[0]['tensors'], alone1[0]['tensors'])
    assert (alone0[1]['report']['verdict'], alone1[1]['report']['verdict']) == (0, 1)
    assert S.differing(alone0[1]['tensors'], alone1[1]['tensors']) and S.differing(alone0[2]['tensors'], alone1[2]['tensors'])
    assert not S.differing(alone0[0]['tensors'], agree0[0]['tensors']), 'on finite steps agree_skips changes no bit'
