"""Cost of the step guard (csrc/optim_guard.hip) against the unguarded update (csrc/optim.hip) on the default model's parameter
tensors, seeded gradients, the EMA copy attached, in the style of tools/optim_step_time.py:

    (u) optim.grad_norm_and_coef + AdamW.step(clip_coef)                       dcf_optim_grad_norm, dcf_optim_adam_step
    (g) the same with guard=StepGuard, finite gradients (verdict apply)        dcf_guard_grad_norm, dcf_guard_adam_step
    (s) the same with one NaN in one gradient (verdict skip: nothing written)

Kernels: the library profiler (device events around each launch), the three paths alternating launch by launch inside one window, so
that each sees the same machine; ROUNDS windows, the median per kernel over the windows and the range.  Steps: windows of WINDOW
consecutive steps between device events, the paths alternating, as in optim_step_time.py (host bound: it shows what the host adds).

    python tools/optim_guard_time.py [--window 20] [--rounds 7] [--out FILE]"""
import argparse
import ctypes
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module('cvpr2025-decafnet_amd')
O = pkg.optim

ap = argparse.ArgumentParser()
ap.add_argument('--window', type=int, default=20)
ap.add_argument('--rounds', type=int, default=7)
ap.add_argument('--out', default=None, help='also write the printed lines to this file')
args = ap.parse_args()
assert torch.cuda.is_available(), 'needs the GPU: there is nothing to time without it'

opt_tree = pkg.config.make_opt()
conf, beta, max_norm = opt_tree.optimizer, opt_tree.train.get('ema_beta', 0.999), opt_tree.optimizer.clip_grad_norm
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def path(guarded, poisoned):
    torch.manual_seed(0)
    model = pkg.modeling.create_model(opt_tree).cuda()
    g = torch.Generator(device='cuda').manual_seed(1)
    for p in model.parameters():
        p.grad = torch.randn(p.shape, device='cuda', generator=g) * 0.01
    params = list(model.parameters())
    if poisoned:
        params[len(params) // 2].grad.view(-1)[0] = float('nan')
    opt = O.make_optimizer(model, conf)
    O.ModelEma(model, beta).init_from().attach(opt)
    table, guard = O._Table(), O.StepGuard('cuda') if guarded else None

    def step():
        _, coef = O.grad_norm_and_coef(params, max_norm, _table=table, guard=guard)
        opt.step(clip_coef=coef, guard=guard)
    step.guard, step.n_el = guard, sum(p.numel() for p in params)
    return step


paths = {'u': path(False, False), 'g': path(True, False), 's': path(True, True)}
n_el = paths['u'].n_el
say(f'default model: {len(list(pkg.modeling.create_model(opt_tree).parameters()))} tensors, {n_el} elements; {args.rounds} windows of {args.window} '
    f'steps per path, alternating')
for fn in paths.values():
    for _ in range(5):
        fn()
torch.cuda.synchronize()
med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731

# ---- the kernels: one profiler window per (round, path); inside a round the paths alternate launch by launch
lib = pkg._lib.lib()
kernel = {}
for _ in range(args.rounds):
    got = {k: {} for k in paths}
    for k in paths:                                          # the profiler keys by kernel name: (g) and (s) share names, so one report each
        lib.dcf_profile_enable(1)
        for _ in range(args.window):
            paths[k]()
            for other in paths:                              # the other two run in between, unprofiled names do not collide with k's
                if other != k and {other, k} != {'g', 's'}:
                    paths[other]()
        torch.cuda.synchronize()
        need = lib.dcf_profile_report(None, 0)
        buf = ctypes.create_string_buffer(int(need) + 16)
        lib.dcf_profile_report(buf, len(buf))
        lib.dcf_profile_enable(0)
        rep = json.loads(buf.value.decode())
        want = ('optim_grad_norm', 'optim_adam_step') if k == 'u' else ('guard_grad_norm', 'guard_adam_step')
        for name in want:
            kernel.setdefault((k, name), []).append(1e3 * rep[name]['ms'] / rep[name]['count'])
label = {'u': 'unguarded', 'g': 'guarded, apply', 's': 'guarded, skip'}
for (k, name), v in kernel.items():
    say(f'    kernel {name:16s} ({label[k]:14s}) {med(v):8.2f} us per launch (min {min(v):.2f}, max {max(v):.2f})')
for a, b in (('optim_grad_norm', 'guard_grad_norm'), ('optim_adam_step', 'guard_adam_step')):
    u, g, s = med(kernel[('u', a)]), med(kernel[('g', b)]), med(kernel[('s', b)])
    say(f'    {b} - {a}: apply {g - u:+.2f} us ({100 * (g / u - 1):+.1f} %), skip {s - u:+.2f} us')

# ---- whole steps between device events (the host's gathering pass included)
times = {k: [] for k in paths}
for _ in range(args.rounds):
    for k, fn in paths.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.window):
            fn()
        e1.record()
        e1.synchronize()
        times[k].append(e0.elapsed_time(e1) * 1e3 / args.window)
for k, v in times.items():
    say(f'({k}) {label[k]:16s} {med(v):9.1f} us per step (min {min(v):.1f}, max {max(v):.1f})')
for k in ('g', 's'):
    rep = paths[k].guard.report()
    say(f'({k}) guard.report(): applied {rep["applied"]}, skipped {rep["skipped"]}, first_bad {rep["first_bad"]}, n_bad_rows {rep["n_bad_rows"]}')

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
