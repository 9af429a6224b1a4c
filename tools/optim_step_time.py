"""Time of the training update on the default model's 449 parameter tensors (14 512 236 elements), seeded gradients:

    (a) this package: optim.grad_norm_and_coef + optim.AdamW.step(clip_coef) with the EMA copy attached (three kernel launches)
    (b) torch as the reference runs it: nn.utils.clip_grad_norm_, torch.optim.AdamW.step() (its default implementation) and the
        Python loop `p_ema.copy_(p.lerp(p_ema, beta))` over the parameters (libs/worker_v2.py:320-325, :654-656)
    (c) the same as (b) with torch.optim.AdamW(fused=True), if this torch build takes it

Each sample is a window of WINDOW consecutive steps between device events, after warm-up; the three paths alternate, REPEATS samples
each, median and range printed.  Then the kernels of (a) alone from the library profiler (device events around each launch) with the
bytes each must move -- 36 B per element for the update with the EMA copy, 28 B without, 4 B for the norm -- as GB/s and as a share of
the measured HBM copy rate (6.29 TB/s).  `--only a|b|c` runs one path alone (for a kernel trace of its own).

    python tools/optim_step_time.py [--window 20] [--repeats 7] [--only a] [--out FILE]

The lines are printed; --out also writes them to FILE (appended with --only, so that single-path runs collect in one file)."""
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
HBM_COPY = 6.29e12                      # B/s, measured float4 copy (the HBM row of the micro-architecture notes)

ap = argparse.ArgumentParser()
ap.add_argument('--window', type=int, default=20)
ap.add_argument('--repeats', type=int, default=7)
ap.add_argument('--only', default=None, choices=['a', 'b', 'c'])
ap.add_argument('--out', default=None, help='also write the printed lines to this file')
args = ap.parse_args()
assert torch.cuda.is_available(), 'needs the GPU: there is nothing to time without it'

opt_tree = pkg.config.make_opt()
conf, beta, max_norm = opt_tree.optimizer, opt_tree.train.get('ema_beta', 0.999), opt_tree.optimizer.clip_grad_norm
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def fresh_model():
    torch.manual_seed(0)
    model = pkg.modeling.create_model(opt_tree).cuda()
    g = torch.Generator(device='cuda').manual_seed(1)
    for p in model.parameters():
        p.grad = torch.randn(p.shape, device='cuda', generator=g) * 0.01
    return model


def path_a():
    model = fresh_model()
    opt = O.make_optimizer(model, conf)
    O.ModelEma(model, beta).init_from().attach(opt)
    params = list(model.parameters())
    table = O._Table()

    def step():
        _, coef = O.grad_norm_and_coef(params, max_norm, _table=table)
        opt.step(clip_coef=coef)
    return step, opt


def path_torch(fused):
    model = fresh_model()
    decay, no_decay = O.split_decay(model)
    named = dict(model.named_parameters())
    groups = [{'params': [named[k] for k in decay], 'weight_decay': conf.weight_decay, 'lr': conf.lr},
              {'params': [named[k] for k in no_decay], 'weight_decay': 0.0, 'lr': conf.lr}]
    opt = torch.optim.AdamW(groups, lr=conf.lr, betas=(0.9, 0.999), **({'fused': True} if fused else {}))
    ema = O.ModelEma(model, beta).init_from()
    params = list(model.parameters())

    @torch.no_grad()
    def step():
        torch.nn.utils.clip_grad_norm_(params, max_norm)
        opt.step()
        for p, e in zip(params, ema.module.parameters()):
            e.copy_(p.detach().lerp(e, beta))
    return step, opt


paths = {}
if args.only in (None, 'a'):
    paths['a'] = path_a()[0]
if args.only in (None, 'b'):
    paths['b'] = path_torch(False)[0]
if args.only in (None, 'c'):
    try:
        step_c = path_torch(True)[0]
        step_c()
        torch.cuda.synchronize()
        paths['c'] = step_c
    except Exception as e:                                   # this build refuses fused=True: said, not hidden
        say(f'(c) torch.optim.AdamW(fused=True) is not available here: {type(e).__name__}: {e}')

n_el = sum(p.numel() for p in pkg.modeling.create_model(opt_tree).parameters())
say(f'default model: 449 tensors, {n_el} elements; window {args.window} steps, {args.repeats} samples per path, alternating')
for fn in paths.values():                                    # warm-up: code objects, the allocator, torch's foreach grouping
    for _ in range(5):
        fn()
torch.cuda.synchronize()
times = {k: [] for k in paths}
for _ in range(args.repeats):
    for k, fn in paths.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.window):
            fn()
        e1.record()
        e1.synchronize()
        times[k].append(e0.elapsed_time(e1) * 1e3 / args.window)
med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
names = {'a': 'this package: norm + coefficient, fused update + EMA', 'b': 'torch: clip_grad_norm_, AdamW.step(), EMA loop',
         'c': 'torch with AdamW(fused=True)'}
for k, v in times.items():
    say(f'({k}) {names[k]:55s} {med(v):9.1f} us per step (min {min(v):.1f}, max {max(v):.1f})')
for k in ('b', 'c'):
    if k in times and 'a' in times:
        say(f'    ({k}) / (a) = {med(times[k]) / med(times["a"]):.2f}')

if 'a' in paths:
    lib = pkg._lib.lib()
    bytes_per = {'optim_adam_step': 36.0, 'optim_grad_norm': 4.0}

    def kernel_times(fn, n=20):
        lib.dcf_profile_enable(1)
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        need = lib.dcf_profile_report(None, 0)
        buf = ctypes.create_string_buffer(int(need) + 16)
        lib.dcf_profile_report(buf, len(buf))
        lib.dcf_profile_enable(0)
        return {k: 1e3 * v['ms'] / v['count'] for k, v in json.loads(buf.value.decode()).items()}

    for k, us in kernel_times(paths['a']).items():
        b = bytes_per.get(k, 0.0) * n_el
        say(f'    kernel {k}: {us:8.1f} us per launch, {b / 1e6:.1f} MB -> {b / us / 1e3:.0f} GB/s = {100 * b / (us * 1e-6) / HBM_COPY:.0f} % of the HBM copy rate')
    step_noema, opt_noema = path_a()
    opt_noema.attach_ema(None, None)
    for _ in range(3):
        step_noema()
    us = kernel_times(step_noema)['optim_adam_step']
    b = 28.0 * n_el
    say(f'    kernel optim_adam_step without the EMA copy: {us:8.1f} us per launch, {b / 1e6:.1f} MB -> {b / us / 1e3:.0f} GB/s = '
        f'{100 * b / (us * 1e-6) / HBM_COPY:.0f} % of the HBM copy rate')

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a' if args.only else 'w') as f:
        f.write('\n'.join(lines) + '\n')
