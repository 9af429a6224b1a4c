"""Time of the sliding-window attention core with dropout on its map (include/decafnet_hip_attn_drop.h) against the released
dropout-free exports, forward and backward:

    (i)  per core call, three paths that take turns: the new export at p = 0.1, the new export at p = 0 (which runs the dropout-free
         kernels after its own checks) and the released export (dcf_op_local_attn / dcf_op_local_attn_bwd).  E = 256 on 4 heads,
         window 9 and 19, at level 0 (T = 2304) and at the smallest pyramid level (T = 36) of a training batch of 4 videos x 2
         queries of the default model.  q, k, v ~ N(0, 1), dO ~ 1e-3 N(0, 1), prefix masks.
    (i') the same for cross attention (Lk = 24, T = 2304 and 36) and global self attention (T = 288 and 36), p = 0.1 against p = 0,
         which is the released export behind this export's checks.
    (iii) ``TrainStep.step`` of the synthetic default model (config.make_opt(text_in=320), synth weights; 2 videos x 2 queries at T = 2304) with
         attn_pdrop = 0.1 on vid_net, fusion and text_net against 0, the TCN at 0.5 in both.
    (ii) ``TrainStep.step`` on the `s1` fixture of tests/golden with vid_net.attn_pdrop = 0.1 (``enable_dropout(sites='all')``)
         against the same step with attn_pdrop = 0, the other rates (proj 0.2, path 0.3, TCN 0.5) alike.

The paths alternate in one process, device events around each sample, warm-up, REPEATS samples each; median and range printed.

    python tools/attn_drop_time.py [--repeats 7] [--window 20] [--out FILE]"""
import argparse
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
pkg = importlib.import_module('cvpr2025-decafnet_amd')
lb = pkg._lib

ap = argparse.ArgumentParser()
ap.add_argument('--repeats', type=int, default=7)
ap.add_argument('--window', type=int, default=20, help='calls per sample')
ap.add_argument('--out', default=None, help='also write the printed lines to this file')
args = ap.parse_args()
assert torch.cuda.is_available(), 'needs the GPU: there is nothing to time without it'
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def med(v):
    return sorted(v)[len(v) // 2]


def alternate(paths, window):
    """{name: fn} -> {name: [us per call]}: warm-up, then `repeats` samples of `window` calls each, the paths taking turns"""
    for fn in paths.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(args.repeats):
        for k, fn in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(window):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / window)
    return times


# ---------------------------------------------------------------------------------------------- (i) the core
E, HEADS, B, SEED, SITE = 256, 4, 8, 0x9E3779B97F4A7C15 - (1 << 64), 2 << 16 | 6
lib, st = lb.lib(), lb.current_stream()
say(f'(i) sliding-window core, E {E} on {HEADS} heads, {B} sequences: us per call, median (min .. max) of {args.repeats} samples of {args.window} calls')
for T in (2304, 36):
    for W in (9, 19):
        g = torch.Generator().manual_seed(T + W)
        q, k, v = (torch.randn(B, T, E, generator=g).cuda() for _ in range(3))
        do = (torch.randn(B, T, E, generator=g) * 1e-3).cuda()
        lens = torch.tensor([T - (b * T) // (3 * B) for b in range(B)])
        mask = (torch.arange(T)[None] < lens[:, None]).cuda()
        o, dq, dk, dv = (torch.empty_like(q) for _ in range(4))
        P = lb.ptr

        def fwd_drop(p):
            return lambda: lb.check(lib.dcf_op_local_attn_drop(P(q), P(k), P(v), P(mask), P(o), B, T, E, HEADS, W, 0, SEED, SITE, p, st), 'fwd')

        def bwd_drop(p):
            return lambda: lb.check(lib.dcf_op_local_attn_drop_bwd(P(q), P(k), P(v), P(mask), P(do), P(dq), P(dk), P(dv), B, T, E, HEADS, W, 0, SEED,
                                                                   SITE, p, st), 'bwd')

        fwd = {'p=0.1': fwd_drop(0.1), 'p=0': fwd_drop(0.0),
               'released': lambda: lb.check(lib.dcf_op_local_attn(P(q), P(k), P(v), P(mask), P(o), B, T, E, HEADS, W, st), 'fwd0')}
        bwd = {'p=0.1': bwd_drop(0.1), 'p=0': bwd_drop(0.0),
               'released': lambda: lb.check(lib.dcf_op_local_attn_bwd(P(q), P(k), P(v), P(mask), P(do), P(dq), P(dk), P(dv), B, T, E, HEADS, W, st), 'bwd0')}
        for what, paths in (('forward ', fwd), ('backward', bwd)):
            t = alternate(paths, args.window)
            say(f'    T {T:5d} W {W:2d} {what}: ' + '; '.join(f'{n} {med(t[n]):7.1f} ({min(t[n]):.1f} .. {max(t[n]):.1f})' for n in paths) +
                f'; p=0.1 / released = {med(t["p=0.1"]) / med(t["released"]):.2f}, p=0 / released = {med(t["p=0"]) / med(t["released"]):.2f}')

# ---------------------------------------------------------------------------------------------- (i') the dense cores
say("(i') global self attention and cross attention (Lk 24), same widths: the new exports run plain vector-ALU kernels at p > 0")
for kind, T, Lk in (('cross', 2304, 24), ('cross', 36, 24), ('global', 288, 288), ('global', 36, 36)):
    g = torch.Generator().manual_seed(T + Lk)
    q = torch.randn(B, T, E, generator=g).cuda()
    k, v = (torch.randn(B, Lk, E, generator=g).cuda() for _ in range(2))
    do = (torch.randn(B, T, E, generator=g) * 1e-3).cuda()
    mask = (torch.arange(Lk)[None] < torch.tensor([Lk - (b * Lk) // (3 * B) for b in range(B)])[:, None]).cuda()
    o, dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    P = lb.ptr

    def fwd(p):
        if kind == 'global':
            return lambda: lb.check(lib.dcf_op_local_attn_drop(P(q), P(k), P(v), P(mask), P(o), B, T, E, HEADS, 0, 0, SEED, SITE, p, st), 'fwd')
        return lambda: lb.check(lib.dcf_op_xattn_drop(P(q), P(k), P(v), P(mask), P(o), B, T, Lk, E, HEADS, 0, SEED, SITE, p, st), 'fwd')

    def bwd(p):
        if kind == 'global':
            return lambda: lb.check(lib.dcf_op_global_attn_drop_bwd(P(q), P(k), P(v), P(mask), P(do), P(dq), P(dk), P(dv), B, T, E, HEADS, 0, SEED, SITE,
                                                                    p, st), 'bwd')
        return lambda: lb.check(lib.dcf_op_xattn_drop_bwd(P(q), P(k), P(v), P(mask), P(do), P(dq), P(dk), P(dv), B, T, Lk, E, HEADS, 0, SEED, SITE, p,
                                                          st), 'bwd')

    for what, mk in (('forward ', fwd), ('backward', bwd)):          # p = 0 runs the released export after the checks
        t = alternate({'p=0.1': mk(0.1), 'released': mk(0.0)}, args.window)
        say(f'    {kind:6s} T {T:5d} Lk {Lk:3d} {what}: ' + '; '.join(f'{n} {med(t[n]):8.1f} ({min(t[n]):.1f} .. {max(t[n]):.1f})' for n in t) +
            f'; p=0.1 / released = {med(t["p=0.1"]) / med(t["released"]):.2f}')

# ---------------------------------------------------------------------------------------------- (ii) the whole step on s1
import step_grad_ref as S  # noqa: E402
import test_gpu_train_step as TS  # noqa: E402

f = S.Fixture('s1')
batch, targets = TS.batch_of(f)


def train_step(attn):
    opt = TS.opt_of(pkg, f)
    for part in ('vid_net', 'fusion'):
        opt.model[part]['proj_pdrop'], opt.model[part]['path_pdrop'] = 0.2, 0.3
    opt.model['vid_net']['attn_pdrop'] = attn
    model = pkg.modeling.PtTransformerEarlyFusionIterative(opt, second_fusion=False)
    model.load_state_dict(f.sd)
    model = model.cuda()
    model.enable_dropout(seed=1, sites='all')
    return pkg.train.TrainStep(model, opt, itrs_per_epoch=1)


steps = {'attn_pdrop 0.1': train_step(0.1), 'attn_pdrop 0': train_step(0.0)}
t = alternate({n: (lambda ts=ts: ts.step(batch, targets)) for n, ts in steps.items()}, max(args.window // 4, 1))
say('(ii) TrainStep.step on the s1 fixture (D = E = 32, T = 40, three queries, window 3), proj 0.2, path 0.3, TCN 0.5')
for n in steps:
    say(f'    {n:15s} {med(t[n]) / 1e3:9.2f} ms per step (min {min(t[n]) / 1e3:.2f}, max {max(t[n]) / 1e3:.2f})')
say(f'    ratio {med(t["attn_pdrop 0.1"]) / med(t["attn_pdrop 0"]):.3f}')

# ---------------------------------------------------------------------------------------------- (iii) the step of the default model
NVID, K, LQ = 2, 2, 16
say(f'(iii) TrainStep.step of the synthetic default model (config.make_opt(text_in=320): D 1024, E 256, 8 levels, window 9, '
    f'T 2304, 5 text layers), {NVID} videos x {K} queries, {LQ} tokens; enable_dropout(sites="all"), the TCN at 0.5, every other rate 0')
g = torch.Generator().manual_seed(7)
D0, T0, TIN = 1024, 2304, 320          # (text_in 320, not 300: the differentiable convolutions take widths that are multiples of 32)
big = dict(vid=torch.randn(NVID, D0, T0, generator=g).cuda(), shallow=torch.randn(NVID, D0, T0, generator=g).cuda(),
           vid_masks=torch.ones(NVID, T0, dtype=torch.bool).cuda(), tokens=torch.randn(NVID * K, TIN, LQ, generator=g).cuda(),
           text_cls=torch.randn(NVID * K, D0, generator=g).cuda(), token_masks=torch.ones(NVID * K, 1, LQ, dtype=torch.bool).cuda(), text_size=[K] * NVID)
big_targets = torch.tensor([[100.0, 400.0], [900.0, 1000.0], [30.0, 60.0], [1500.0, 2200.0]]).cuda()


def default_step(attn):
    opt = pkg.config.make_opt(text_in=TIN)
    for part in ('vid_net', 'fusion', 'text_net'):
        opt.model[part]['attn_pdrop'] = attn
    model = pkg.modeling.create_model(opt)
    model.load_state_dict(pkg.synth.make_state_dict({k: list(v.shape) for k, v in model.state_dict().items()}, 2025))
    model = model.cuda()
    model.enable_dropout(seed=1, sites='all')
    return pkg.train.TrainStep(model, opt, itrs_per_epoch=1)


steps = {'attn_pdrop 0.1': default_step(0.1), 'attn_pdrop 0': default_step(0.0)}
t = alternate({n: (lambda ts=ts: ts.step(big, big_targets)) for n, ts in steps.items()}, 2)
for n in steps:
    say(f'    {n:15s} {med(t[n]) / 1e3:9.2f} ms per step (min {min(t[n]) / 1e3:.2f}, max {max(t[n]) / 1e3:.2f})')
say(f'    ratio {med(t["attn_pdrop 0.1"]) / med(t["attn_pdrop 0"]):.3f}')

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
