"""GPU checks of the training log in the loops (``train.StepLog``, ``fit(..., log_interval=)``) and of the resumable data stream
(``fit(..., data_state=True)``), on the set-up of tests/fit_setup.py: the tiny model of tests/golden/step_grad_s2, a generated tree of
5 videos, two steps per epoch, ``front_end='shared'``.

1. A logged run against a plain run: ``fit(num_epochs=2, log_interval=2)`` writes the lines of itr 1, 2 and 4; a second run stepped by
   hand, with ``float(v)`` per step into an ``AverageMeter`` written out here and reset at the same iterations, gives the same lines
   string for string up to the last `` | ``; the time field parses and the seconds are positive; parameters, EMA copy and optimizer
   state are bit-equal to those of a ``fit`` without the log.
2. No host wait: eight ``update``s of a ``StepLog(log_interval=4)`` under ``torch.cuda.set_sync_debug_mode('error')``.
3. ``log_interval=1``: ascending lines, one ``on_line`` call per line with ``steps == 1``; ``log_interval=0``: no ``log.txt`` and the
   listing of today's ``fit``.
4. ``fit_parallel`` on a world-1 step writes the loss fields of ``fit``.
5. ``data_state=True`` on a tree with ``crop_ratio=(0.5, 1.0)``: one epoch plus a resume to two leaves the tensors of the
   uninterrupted run, and without the data state it does not."""
import os
import re
import shutil

import pytest
import torch

import fit_setup as S
import train_data_tree as TT
from conftest import load_pkg

pytestmark = pytest.mark.gpu
KEYS = ('cls', 'reg', 'total')
TIME = re.compile(r'^(\d+\.\d)([smh])$')


class AverageMeter:
    """libs/train_utils.py:34-53, written out"""

    def __init__(self):
        self.reset()

    def reset(self):
        self.val = 0
        self.sum = 0
        self.mean = 0
        self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.mean = self.sum / self.count

    def item(self):
        return self.mean


@pytest.fixture(scope='module')
def world(tmp_path_factory):
    pkg = load_pkg()
    f, cfg, _, _ = S.build_world(pkg, str(tmp_path_factory.mktemp('tree')))
    return pkg, f, cfg


def listing(root):
    return sorted(os.path.relpath(os.path.join(d, n), root) for d, _, names in os.walk(root) for n in names)


def read_lines(root):
    return open(os.path.join(root, 'log.txt')).read().splitlines()


def loss_fields(lines):
    """every line up to and including its last `` | ``"""
    assert all(' | ' in line for line in lines)
    return [line[:line.rindex(' | ') + 3] for line in lines]


@pytest.fixture(scope='module')
def logged(world, tmp_path_factory):
    """fit over two epochs with log_interval=2 -> (root, tensors, what on_line was handed)"""
    pkg, f, cfg = world
    root = str(tmp_path_factory.mktemp('logged'))
    ts, loader = S.make_step(pkg, f, cfg)
    calls = []
    assert pkg.train.fit(ts, loader, root, num_epochs=2, log_interval=2, on_line=lambda *a: calls.append(a)) == []
    assert (ts.epoch, ts.itr) == (2, 4)
    return root, S.tensors(ts), calls


@pytest.fixture(scope='module')
def plain(world, tmp_path_factory):
    """today's fit: no log argument -> (root, tensors)"""
    pkg, f, cfg = world
    root = str(tmp_path_factory.mktemp('plain'))
    ts, loader = S.make_step(pkg, f, cfg)
    pkg.train.fit(ts, loader, root, num_epochs=2)
    return root, S.tensors(ts)


def test_logged_run_against_a_plain_run(world, logged, plain):
    pkg, f, cfg = world
    root, tensors, calls = logged
    lines = read_lines(root)
    print('\n'.join(lines))
    ts, loader = S.make_step(pkg, f, cfg)                                       # the reference's way: a host read per value and step
    meters, want, num_itrs = {k: AverageMeter() for k in KEYS}, [], 2 * len(loader)
    while ts.epoch < 2:
        for batch, targets in loader.epoch(ts.epoch):
            out = ts.step(batch, targets)
            for k in KEYS:
                meters[k].update(out[k].detach().item())
            if ts.itr == 1 or ts.itr % 2 == 0:                                  # worker_v2.py:334, 705-713
                t = len(str(num_itrs))
                log_str = f'[{ts.itr:0{t}d}/{num_itrs:0{t}d}] '
                for k, v in meters.items():
                    log_str += f'{k} {v.item():.3f} | '
                    v.reset()
                want.append(log_str)
        ts.epoch += 1
    assert [w[:5] for w in want] == ['[1/4]', '[2/4]', '[4/4]']
    assert loss_fields(lines) == want, (lines, want)
    assert [c[0] for c in calls] == [1, 2, 4] and [c[2] for c in calls] == [1, 1, 2]
    for line, (itr, stats, steps, seconds) in zip(lines, calls):
        field = line[line.rindex(' | ') + 3:]
        assert TIME.match(field) and field == pkg.train.time_str(seconds), line
        assert 0.0 < seconds < 600.0, 'device seconds per step'
        assert tuple(stats) == KEYS and all(tuple(s) == pkg.train.LOG_STATS for s in stats.values())
        assert all(s['n_finite'] == steps and s['min'] <= s['finite_mean'] == s['mean'] <= s['max'] for s in stats.values())
    assert not S.differing(S.tensors(ts), plain[1]), 'stepping by hand is the plain fit'
    assert not S.differing(tensors, plain[1]), 'the log changed a parameter, an EMA tensor or an optimizer state'
    assert listing(root) == sorted(listing(plain[0]) + ['log.txt'])


def test_update_never_waits_for_the_device(world, tmp_path):
    pkg, f, cfg = world
    ts, loader = S.make_step(pkg, f, cfg)
    calls = []
    log = pkg.train.StepLog(ts, 8, str(tmp_path / 'log.txt'), log_interval=4, on_line=lambda *a: calls.append(a))
    for e in (0, 1, 0, 1):
        for batch, targets in loader.epoch(e):
            out = ts.step(batch, targets)
            torch.cuda.set_sync_debug_mode('error')                              # the step itself uploads its batch; the log must not wait
            try:
                log.update(out)
            finally:
                torch.cuda.set_sync_debug_mode('default')
    assert ts.itr == 8 and log.lines + len(log._pending) == 3
    log.drain()                                                                  # the one wait, outside the mode
    assert log.lines == 3 and not log._pending and log.drain() == 0
    lines = open(tmp_path / 'log.txt').read().splitlines()
    assert [line[:5] for line in lines] == ['[1/8]', '[4/8]', '[8/8]'] and [c[2] for c in calls] == [1, 3, 4]


def test_every_step_logged_in_order_and_the_default_writes_nothing(world, plain, tmp_path):
    pkg, f, cfg = world
    ts, loader = S.make_step(pkg, f, cfg)
    calls = []
    pkg.train.fit(ts, loader, str(tmp_path), num_epochs=2, log_interval=1, log_keys=('total', 'grad_norm'),
                  on_line=lambda *a: calls.append(a))
    lines = read_lines(str(tmp_path))
    assert [line[:5] for line in lines] == ['[1/4]', '[2/4]', '[3/4]', '[4/4]']
    assert all(re.match(r'^\[\d/4\] total \S+ \| grad_norm \S+ \| \d+\.\d[smh]$', line) for line in lines), lines
    assert [c[0] for c in calls] == [1, 2, 3, 4] and all(c[2] == 1 and tuple(c[1]) == ('total', 'grad_norm') for c in calls)
    assert all(c[1]['total']['mean'] == c[1]['total']['last'] == c[1]['total']['min'] for c in calls)
    # the default: today's files and no other
    assert 'log.txt' not in listing(plain[0])
    assert listing(plain[0]) == ['models/1-2.pth', 'models/2-4.pth', 'models/last.pth', 'states/last.pth']


def test_fit_parallel_on_one_rank_writes_the_same_loss_fields(world, logged, tmp_path):
    pkg, f, cfg = world
    ts, loader = S.make_step(pkg, f, cfg)
    assert pkg.train.fit_parallel(ts, loader, str(tmp_path), num_epochs=2, log_interval=2) == []
    assert loss_fields(read_lines(str(tmp_path))) == loss_fields(read_lines(logged[0]))
    assert listing(str(tmp_path)) == listing(logged[0])
    assert not S.differing(S.tensors(ts), logged[1])


def test_resume_with_the_data_state_continues_the_uninterrupted_run(world, tmp_path):
    pkg, f, cfg = world
    cfg = dict(cfg, crop_ratio=(0.5, 1.0))                                       # the same tree; every decision now draws a window
    fit = pkg.train.fit
    ts, loader = S.make_step(pkg, f, cfg)
    fit(ts, loader, str(tmp_path / 'whole'), num_epochs=2, data_state=True)
    whole = S.tensors(ts)
    assert listing(str(tmp_path / 'whole')) == ['models/1-2.pth', 'models/2-4.pth', 'models/last.pth', 'states/data_last.pth', 'states/last.pth']
    s = torch.load(tmp_path / 'whole' / 'states' / 'last.pth', map_location='cpu', weights_only=False)
    assert set(s) == {'optimizer', 'scheduler', 'epoch', 'itr', 'loss_norm'}, 'the data state has a file of its own'
    d = torch.load(tmp_path / 'whole' / 'states' / 'data_last.pth', map_location='cpu', weights_only=False)
    assert d['world_size'] == 1 and len(d['ranks']) == 1 and set(d['ranks'][0]) == {'rng'}

    ts, loader = S.make_step(pkg, f, cfg)
    fit(ts, loader, str(tmp_path / 'parts'), num_epochs=1, data_state=True)
    assert (ts.epoch, ts.itr) == (1, 2)
    shutil.copytree(tmp_path / 'parts', tmp_path / 'stateless')
    os.remove(tmp_path / 'stateless' / 'states' / 'data_last.pth')
    ts, loader = S.make_step(pkg, f, cfg)                                        # fresh objects: everything comes from the files
    fit(ts, loader, str(tmp_path / 'parts'), num_epochs=2, resume=True, data_state=True)
    assert (ts.epoch, ts.itr) == (2, 4)
    assert not S.differing(S.tensors(ts), whole), 'resumed with the data state and uninterrupted'

    ts, loader = S.make_step(pkg, f, cfg)                                        # without it the streams start over: other windows
    fit(ts, loader, str(tmp_path / 'stateless'), num_epochs=2, resume=True)
    assert (ts.epoch, ts.itr) == (2, 4)
    assert S.differing(S.tensors(ts), whole), 'the tree and seed of this test must make the data state matter'
    assert 'states/data_last.pth' not in listing(str(tmp_path / 'stateless'))
