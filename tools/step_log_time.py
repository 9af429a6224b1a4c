"""What the training log costs per step (profiles/step_log.md):

    python tools/step_log_time.py <repository root> [--shape small|large] [--steps 20] [--passes 9] [--warmup 2] [--variants none,steplog,item]

Three variants of ``fit``'s step loop on the set-up of tests/fit_setup.py ('small': the tiny model of tests/golden/step_grad_s2, T = 80,
two samples a step) or on a wider one ('large': D = 256, E = 128, 4 levels, T = 320, six samples a step, synthetic weights):

    none      ts.step alone, as ``fit`` runs it with ``log_interval=0``
    steplog   ts.step and ``StepLog(log_interval=10).update``: one launch a step, a flush and a 192-byte copy every tenth
    item      ts.step and ``float(v)`` on cls, reg and total after every step: the reference's meters (worker_v2.py:326-335)

Each variant owns a fresh (ts, loader) of the same initial state.  A pass is ``--steps`` steps of one variant, timed on the host clock
from the first call to the end of a final ``torch.cuda.synchronize()``: the time a loop of that length takes, the host running ahead
where the variant lets it.  The variants alternate pass by pass in one process; the first ``--warmup`` passes of each are dropped.
Printed: per variant the median, minimum and maximum of milliseconds per step, for 'steplog' the host time of an ``update`` call
(``time.perf_counter`` around it, flushes and polls included), and one JSON line.

``<repository root>`` may be a checkout of an earlier commit with its own build: where ``train.StepLog`` does not exist the 'none'
variant runs alone -- the measurement of "default arguments cost nothing" against the parent and not against this tree; compare it
with ``--variants none`` on this tree, a process that likewise holds one model."""
import argparse
import importlib
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ap = argparse.ArgumentParser()
ap.add_argument('root')
ap.add_argument('--shape', choices=('small', 'large'), default='small')
ap.add_argument('--steps', type=int, default=20)
ap.add_argument('--passes', type=int, default=9)
ap.add_argument('--warmup', type=int, default=2)
ap.add_argument('--variants', default='none,steplog,item')
args = ap.parse_args()

root = os.path.abspath(args.root)
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, 'tests'))
pkg = importlib.import_module('cvpr2025-decafnet_amd')
import fit_setup as S  # noqa: E402
import step_grad_ref as R  # noqa: E402
import train_data_tree as TT  # noqa: E402

LARGE = dict(D=256, E=128, TE=128, text_in=64, n_levels=4, win=5, n_heads=4, sn=8, sratio=0.5, norm=True, max_seq_len=256, text_layers=2,
             text_max_len=24, text_use_abs_pe=True, n_stem=1, vid_stride=2, msf=True)
LARGE_T, LARGE_VIDEOS = 320, 12


def small_world(tree):
    f, cfg, _, _ = S.build_world(pkg, tree)
    return lambda: S.make_step(pkg, f, cfg)


def large_world(tree):
    arrays, data = TT.random_tree(5, LARGE_VIDEOS, LARGE['D'], LARGE['text_in'], LARGE_T, 9)
    TT.write_tree(tree, arrays)
    cfg = TT.cfg_of(tree, dict(data, crop_ratio=None))
    f = R.Fixture('s2')                                                          # for the Trainer's settings of the case alone

    def make():
        td = pkg.data.VideoCentricTrainData(cfg, num_epochs=2, seed=3)
        loader = pkg.data.TrainLoader(td, pkg.data.FeatureBank(td), 6, input_vid_len=LARGE_T, vid_stride=LARGE['vid_stride'])
        opt = pkg.config.make_opt(**LARGE)
        opt.train.center_sampling, opt.train.reg_loss, opt.train.warmup_epochs = f.meta['center_sampling'], f.meta['reg_loss'], 1
        model = pkg.modeling.create_model(opt)
        model.load_state_dict(pkg.synth.make_state_dict({k: list(v.shape) for k, v in model.state_dict().items()}, 2025))
        return pkg.train.TrainStep(model.cuda(), opt, itrs_per_epoch=len(loader), front_end='shared'), loader
    return make


def batches(loader):
    """the batches of epochs 0, 1, 0, 1, ... without end"""
    e = 0
    while True:
        yield from loader.epoch(e % 2)
        e += 1


class Variant:
    def __init__(self, name, make, tree):
        self.name = name
        self.ts, loader = make()
        self.stream = batches(loader)
        self.log = None
        if name == 'steplog':
            self.log = pkg.train.StepLog(self.ts, 10 ** 6, os.path.join(tree, 'log.txt'), log_interval=10)
        self.ms, self.update_s, self.updates = [], 0.0, 0

    def one_pass(self, steps):
        ts, log, item = self.ts, self.log, self.name == 'item'
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            batch, targets = next(self.stream)
            out = ts.step(batch, targets)
            if log is not None:
                t1 = time.perf_counter()
                log.update(out)
                self.update_s += time.perf_counter() - t1
                self.updates += 1
            elif item:
                for k in ('cls', 'reg', 'total'):
                    float(out[k])
        torch.cuda.synchronize()
        if log is not None:
            log.drain()
        self.ms.append((time.perf_counter() - t0) * 1e3 / steps)


with tempfile.TemporaryDirectory() as tree:
    make = (small_world if args.shape == 'small' else large_world)(tree)
    names = tuple(n for n in args.variants.split(',') if n in ('none', 'steplog', 'item'))
    if not hasattr(pkg.train, 'StepLog'):
        names = ('none',)
    variants = [Variant(n, make, tree) for n in names]
    for _ in range(args.warmup + args.passes):
        for v in variants:
            v.one_pass(args.steps)
    result = {'root': os.path.basename(root) or root, 'shape': args.shape, 'steps': args.steps, 'passes': args.passes, 'warmup': args.warmup}
    for v in variants:
        kept = v.ms[args.warmup:]
        result[v.name] = {'median_ms': round(statistics.median(kept), 3), 'min_ms': round(min(kept), 3), 'max_ms': round(max(kept), 3)}
        print(f'STEPLOG {result["root"]} {args.shape} {v.name:8s} median {statistics.median(kept):8.3f} ms/step, min {min(kept):8.3f}, '
              f'max {max(kept):8.3f} ({args.passes} passes of {args.steps} steps after {args.warmup})')
    for v in variants:
        if v.log is not None:
            result['log_lines'], result['update_host_us'] = v.log.lines, round(v.update_s / v.updates * 1e6, 1)
            print(f'STEPLOG {result["root"]} {args.shape} StepLog.update: {result["update_host_us"]} us of host time per call ({v.updates} calls, '
                  f'{v.log.lines} lines)')
    print(json.dumps(result))
