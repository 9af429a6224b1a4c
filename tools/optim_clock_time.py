"""Cost of Adam's step counts on the device (csrc/optim_clock.hip) against the guarded update with the counts by value
(csrc/optim_guard.hip) on the default model's parameter tensors, seeded gradients, the EMA copy attached, in the style of
tools/grad_pack_time.py:

    device, on ONE table and the same tensors, the guard's verdict apply, tables and counts resident:
    (g) dcf_guard_adam_step    the two groups' corrections by value
    (c) dcf_clock_adam_step    the count and the corrections read per chunk, plus the launch of one thread per row
    (t) dcf_clock_adam_step with n_chunks = 0: that second launch alone (on counts of its own)
    host, what a training step calls (the gathering pass, the comparison with the table of the step before, the launch):
    (h) AdamW.step(clip_coef, guard)                       device_count=False
    (d) AdamW.step(clip_coef, guard)                       device_count=True

Each sample is a window of WINDOW consecutive calls between device events, after warm-up; the paths alternate, REPEATS samples each,
median and range printed.  For (h) and (d) the host's own time for the same window (perf_counter around the calls, which do not wait
for the device) is printed too: the step is host bound, so the two figures agree.

    python tools/optim_clock_time.py [--window 20] [--repeats 9] [--out FILE]"""
import argparse
import ctypes
import importlib
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module('cvpr2025-decafnet_amd')
O, lb = pkg.optim, pkg._lib

ap = argparse.ArgumentParser()
ap.add_argument('--window', type=int, default=20)
ap.add_argument('--repeats', type=int, default=9)
ap.add_argument('--out', default=None, help='also write the printed lines to this file')
args = ap.parse_args()
assert torch.cuda.is_available(), 'needs the GPU: there is nothing to time without it'
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


opt_tree = pkg.config.make_opt()
conf, beta, max_norm = opt_tree.optimizer, opt_tree.train.get('ema_beta', 0.999), opt_tree.optimizer.clip_grad_norm


def optimizer(device_count):
    torch.manual_seed(0)
    model = pkg.modeling.create_model(opt_tree).cuda()
    g = torch.Generator(device='cuda').manual_seed(1)
    for p in model.parameters():
        p.grad = torch.randn(p.shape, device='cuda', generator=g) * 0.01
    opt = O.make_optimizer(model, conf, device_count=device_count)
    O.ModelEma(model, beta).init_from().attach(opt)
    params, guard, table = list(model.parameters()), O.StepGuard('cuda'), O._Table()
    _, coef = O.grad_norm_and_coef(params, max_norm, _table=table, guard=guard)        # finite gradients: the verdict is apply and stays
    opt.step(clip_coef=coef, guard=guard)                                              # lays out the table, the counts, the moments
    return opt, guard, coef, params


off, guard_h, coef_h, _ = optimizer(False)
on, guard_d, coef_d, params = optimizer(True)
assert guard_d.report()['verdict'] == 0 and guard_h.report()['verdict'] == 0
n_el = sum(p.numel() for p in params)
lib, dev = lb.lib(), params[0].device

# ---- the device paths: both exports on the table, tensors, coefficient and guard of `on`
table = on._table
groups_c, bc_tables, bc_len = on._clock_args(dev)
groups_g = on._group_array({(g, 5): g for g in range(len(on.param_groups))})           # by value: the corrections of count 5 for both groups
n_groups, ema = len(on.param_groups), (1, float(beta))
state = guard_d._on(dev)


def path_g():
    lb.check(lib.dcf_guard_adam_step(*table.args(), ctypes.cast(groups_g, ctypes.c_void_p), n_groups, lb.ptr(coef_d), state, *ema,
                                     lb.current_stream()), 'dcf_guard_adam_step')


def path_c():
    lb.check(lib.dcf_clock_adam_step(*table.args(), ctypes.cast(groups_c, ctypes.c_void_p), n_groups, ctypes.cast(bc_tables, ctypes.c_void_p),
                                     ctypes.cast(bc_len, ctypes.c_void_p), lb.ptr(on._steps), lb.ptr(coef_d), state, *ema, lb.current_stream()),
             'dcf_clock_adam_step')


ticks = torch.zeros_like(on._steps)


def path_t():
    lb.check(lib.dcf_clock_adam_step(lb.ptr(table.rows), None, table.n_tensors, 0, ctypes.cast(groups_c, ctypes.c_void_p), n_groups, None, None,
                                     lb.ptr(ticks), lb.ptr(coef_d), state, *ema, lb.current_stream()), 'dcf_clock_adam_step')


def path_h():
    off.step(clip_coef=coef_h, guard=guard_h)


def path_d():
    on.step(clip_coef=coef_d, guard=guard_d)


paths = {'g': path_g, 'c': path_c, 't': path_t, 'h': path_h, 'd': path_d}
names = {'g': 'dcf_guard_adam_step, one launch', 'c': 'dcf_clock_adam_step, two launches', 't': 'dcf_clock_adam_step, no chunks', 'h': 'AdamW.step, device_count=False',
         'd': 'AdamW.step, device_count=True'}
say(f'default model: {table.n_tensors} tensors, {n_el} elements, {table.n_chunks} chunks, bias-correction tables of {list(bc_len)} entries; '
    f'window {args.window} calls, {args.repeats} samples per path, alternating')
for fn in paths.values():
    for _ in range(5):
        fn()
torch.cuda.synchronize()
times, host = {k: [] for k in paths}, {k: [] for k in paths}
for _ in range(args.repeats):
    for k, fn in paths.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        t0 = time.perf_counter()
        for _ in range(args.window):
            fn()
        t1 = time.perf_counter()
        e1.record()
        e1.synchronize()
        times[k].append(e0.elapsed_time(e1) * 1e3 / args.window)
        host[k].append((t1 - t0) * 1e6 / args.window)
med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
for k, v in times.items():
    say(f'({k}) {names[k]:36s} {med(v):9.1f} us per call between device events (min {min(v):.1f}, max {max(v):.1f}); '
        f'host {med(host[k]):8.1f} us per call (min {min(host[k]):.1f}, max {max(host[k]):.1f})')
say(f'    (c) - (g) = {med(times["c"]) - med(times["g"]):+.1f} us between device events ({100 * (med(times["c"]) / med(times["g"]) - 1):+.1f} %); '
    f'(d) - (h) = {med(host["d"]) - med(host["h"]):+.1f} us of host time ({100 * (med(host["d"]) / med(host["h"]) - 1):+.1f} %)')
b = 36.0 * n_el
say(f'    36 B per element = {b / 1e6:.0f} MB per update: (g) {b / med(times["g"]) / 1e3:.0f} GB/s, (c) {b / med(times["c"]) / 1e3:.0f} GB/s')
say(f'    counts after the run: min {int(on._steps.min())}, max {int(on._steps.max())}; guard: {guard_d.report()["applied"]} applied')

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
