"""Time and memory of the training front end, dense against shared (``train.training_forward(front_end=...)``):

    (i)  the front end alone, forward + backward: ``autograd.masked_conv1d`` on the materialised (B', T, Cin) input (repeat, transpose,
         gate, concatenate -- the five steps of the dense path) against ``autograd.gated_vid_map``, at D = 1024, E = 256, msf,
         T = 2304, four videos x two queries, sn = 60, sratio = 0.3.  The shape is chosen here from BASELINE's widths and the
         reference's max_num_text = 2; the gates come from dcf_op_sidekick / dcf_op_gate on a drifting random shallow sequence.
         Printed with it: the algorithmic bytes and flops of both paths from the shapes, the share of 64-clip tiles no query keeps,
         and the peak allocated memory of each path (torch.cuda.max_memory_allocated over one forward + backward).
    (ii) ``TrainStep.step`` on the `s1` fixture of tests/golden (tests/step_grad_ref.py), both front ends.

The paths alternate in one process, device events around each sample, warm-up, REPEATS samples each; median and range printed.

    python tools/front_grad_time.py [--repeats 7] [--window 5] [--out FILE]"""
import argparse
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
pkg = importlib.import_module('cvpr2025-decafnet_amd')
A, lb = pkg.autograd, pkg._lib

ap = argparse.ArgumentParser()
ap.add_argument('--repeats', type=int, default=7)
ap.add_argument('--window', type=int, default=5)
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


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


# ---------------------------------------------------------------------------------------------- (i) the front end alone
D, E, T, NVID, K, SN, SRATIO = 1024, 256, 2304, 4, 2, 60, 0.3
sizes = [K] * NVID
nq = sum(sizes)
g = torch.Generator().manual_seed(5)
vid = torch.randn(NVID, D, T, generator=g).cuda()
walk = torch.zeros(NVID, D, T)
step = torch.randn(NVID, D, T, generator=g)
walk[..., 0] = step[..., 0]
for i in range(1, T):
    walk[..., i] = 0.97 * walk[..., i - 1] + 0.25 * step[..., i]
shallow = walk.cuda()
text_cls = torch.randn(nq, D, generator=g).cuda()
vm = torch.ones(T, dtype=torch.bool, device='cuda')
lib, st = lb.lib(), lb.current_stream()
gates, masks = [], []
for b in range(NVID):
    correl = torch.empty(K, T, device='cuda')
    lb.check(lib.dcf_op_sidekick(lb.ptr(shallow[b].contiguous()), lb.ptr(text_cls[b * K:(b + 1) * K].contiguous()), lb.ptr(correl), D, T, K, 1, st), 'dcf_op_sidekick')
    gate, mo = torch.empty(K, T, device='cuda'), torch.empty(K, T, dtype=torch.bool, device='cuda')
    lb.check(lib.dcf_op_gate(lb.ptr(correl), lb.ptr(vm), lb.ptr(gate), lb.ptr(mo), T, K, SN, SRATIO, 1, st), 'dcf_op_gate')
    gates.append(gate), masks.append(mo)
gate, mask = torch.cat(gates), torch.cat(masks)
weight = torch.nn.Parameter(torch.randn(E, 2 * D, 1, generator=g).cuda() * (2 * D) ** -0.5)
bias = torch.nn.Parameter(torch.randn(E, generator=g).cuda() * 0.1)
dY = torch.randn(nq, T, E, generator=g).cuda() * 1e-3
kv = torch.tensor(sizes, device='cuda')


def dense():
    weight.grad = bias.grad = None
    rep = lambda z: z.transpose(1, 2).contiguous().repeat_interleave(kv, dim=0)
    x = torch.cat([rep(vid) * gate[..., None], rep(shallow)], dim=2)
    A.masked_conv1d(x, mask, weight, bias).backward(dY)


def shared():
    weight.grad = bias.grad = None
    A.gated_vid_map(vid, shallow, gate, mask, None, sizes, weight, bias).backward(dY)


ntiles = (T + 63) // 64
kept = sum(bool(gate[b * K:(b + 1) * K, 64 * f:64 * f + 64].any()) for b in range(NVID) for f in range(ntiles))
skipped = 1.0 - kept / (NVID * ntiles)
Cin = 2 * D
flops = {'dense': 2 * 2.0 * nq * T * Cin * E,                                             # forward GEMM + weight-gradient GEMM on B' T rows
         'shared': 2 * 2.0 * NVID * T * D * E * ((1.0 - skipped) + 1.0) + 6.0 * nq * T * E}      # the products once per video (+ combine / row sums)
# fp32 passes: dense reads the features (2 tensors), writes and re-reads x five times over (repeat, gate, cat, mask, the two GEMMs),
# shared reads the features in each direction and moves the (nvid, T, E) products / row sums and the (B', T, E) rows
byts = {'dense': 4.0 * (2 * NVID * D * T + 7.0 * nq * T * Cin + 2.0 * nq * T * E),
        'shared': 4.0 * (2 * 2 * NVID * D * T + 4.0 * 2 * NVID * T * E + 2.0 * nq * T * E)}
say(f'(i) front end alone, forward + backward: D {D}, E {E}, msf, T {T}, {NVID} videos x {K} queries, sn {SN}, sratio {SRATIO}; '
    f'{100 * skipped:.1f} % of the {NVID * ntiles} 64-clip tiles are kept by no query; gate keeps {gate.sum(1).int().tolist()} clips per row')
t = alternate({'dense': dense, 'shared': shared}, args.window)
peaks = {'dense': peak_of(dense), 'shared': peak_of(shared)}
for k in ('dense', 'shared'):
    say(f'    {k:7s} {med(t[k]):9.1f} us (min {min(t[k]):.1f}, max {max(t[k]):.1f}); algorithmic {flops[k] / 1e9:7.2f} GFLOP, {byts[k] / 1e6:8.1f} MB; '
        f'peak allocated {peaks[k] / 2 ** 20:8.1f} MiB')
say(f'    dense / shared = {med(t["dense"]) / med(t["shared"]):.2f} in time, {peaks["dense"] / peaks["shared"]:.2f} in peak memory')

# ---------------------------------------------------------------------------------------------- (ii) the whole step on s1
import step_grad_ref as S  # noqa: E402
import test_gpu_train_step as TS  # noqa: E402

f = S.Fixture('s1')
batch, targets = TS.batch_of(f)
steps = {fe: pkg.train.TrainStep(f.model(pkg).cuda(), TS.opt_of(pkg, f), itrs_per_epoch=1, front_end=fe) for fe in ('dense', 'shared')}
t = alternate({fe: (lambda ts=ts: ts.step(batch, targets)) for fe, ts in steps.items()}, args.window)
say(f'(ii) TrainStep.step on the s1 fixture (D = E = 32, T = 40, three queries)')
for k in ('dense', 'shared'):
    say(f'    {k:7s} {med(t[k]) / 1e3:9.2f} ms per step (min {min(t[k]) / 1e3:.2f}, max {max(t[k]) / 1e3:.2f})')

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
