"""Time and memory of the shared training front end on float16 clip features against the same values as fp32
(include/decafnet_hip_front_half.h against include/decafnet_hip_front.h), at shape (i) of tools/front_grad_time.py: D = 1024, E = 256,
msf, T = 2304, four videos x two queries, sn = 60, sratio = 0.3, the same gates.  The features are binary16-valued in both paths.

    forward    dcf_op_vidmap_shared_h against dcf_op_vidmap_shared
    backward   dcf_op_vidmap_shared_bwd_h against dcf_op_vidmap_shared_bwd
    round trip ``autograd.gated_vid_map`` forward + backward on the float16 pair against what a float16 batch paid before the half
               operators existed: the ``.float()`` of both tensors, then the fp32 call on the copies
    memory     torch.cuda.max_memory_allocated over one round trip of each (the float16 features themselves are resident before)

Printed with them: the algorithmic bytes and flops of both paths from the shapes.  The paths alternate in one process, device events
around each sample, warm-up, REPEATS samples each; median and range printed.

    python tools/front_half_time.py [--repeats 7] [--window 5] [--out FILE]"""
import argparse
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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


# ---------------------------------------------------------------------------------------------- the operands of front_grad_time.py (i)
D, E, T, NVID, K, SN, SRATIO = 1024, 256, 2304, 4, 2, 60, 0.3
sizes = [K] * NVID
nq = sum(sizes)
g = torch.Generator().manual_seed(5)
vid_h = torch.randn(NVID, D, T, generator=g).half().cuda()
walk = torch.zeros(NVID, D, T)
step = torch.randn(NVID, D, T, generator=g)
walk[..., 0] = step[..., 0]
for i in range(1, T):
    walk[..., i] = 0.97 * walk[..., i - 1] + 0.25 * step[..., i]
shallow_h = walk.half().cuda()
vid32, shallow32 = vid_h.float(), shallow_h.float()
text_cls = torch.randn(nq, D, generator=g).cuda()
vm = torch.ones(T, dtype=torch.bool, device='cuda')
lib, st = lb.lib(), lb.current_stream()
gates, masks = [], []
for b in range(NVID):
    correl = torch.empty(K, T, device='cuda')
    lb.check(lib.dcf_op_sidekick_h(lb.ptr(shallow_h[b].contiguous()), lb.ptr(text_cls[b * K:(b + 1) * K].contiguous()), lb.ptr(correl), D, T, K, 1, st),
             'dcf_op_sidekick_h')
    gate, mo = torch.empty(K, T, device='cuda'), torch.empty(K, T, dtype=torch.bool, device='cuda')
    lb.check(lib.dcf_op_gate(lb.ptr(correl), lb.ptr(vm), lb.ptr(gate), lb.ptr(mo), T, K, SN, SRATIO, 1, st), 'dcf_op_gate')
    gates.append(gate), masks.append(mo)
gate, mask = torch.cat(gates), torch.cat(masks)
weight = torch.nn.Parameter(torch.randn(E, 2 * D, 1, generator=g).cuda() * (2 * D) ** -0.5)
bias = torch.nn.Parameter(torch.randn(E, generator=g).cuda() * 0.1)
dY = torch.randn(nq, T, E, generator=g).cuda() * 1e-3
W2 = weight.detach().reshape(E, 2 * D).contiguous()
Y, dW, db = torch.empty(nq, T, E, device='cuda'), torch.empty(E, 2 * D, device='cuda'), torch.empty(E, device='cuda')
host_nq = torch.tensor(sizes, dtype=torch.int32)
p = lb.ptr


def op_forward(name, v, s):
    lb.check(getattr(lib, name)(p(v), p(s), p(W2), p(bias), p(gate), p(mask), None, p(host_nq), p(Y), NVID, D, T, E, 0, st), name)


def op_backward(name, v, s):
    lb.check(getattr(lib, name)(p(v), p(s), p(gate), p(mask), None, p(host_nq), p(dY), p(dW), p(db), NVID, D, T, E, 0, 0, st), name)


def trip(v, s):
    weight.grad = bias.grad = None
    A.gated_vid_map(v, s, gate, mask, None, sizes, weight, bias).backward(dY)


paths = {
    'forward': {'fp32': lambda: op_forward('dcf_op_vidmap_shared', vid32, shallow32), 'half': lambda: op_forward('dcf_op_vidmap_shared_h', vid_h, shallow_h)},
    'backward': {'fp32': lambda: op_backward('dcf_op_vidmap_shared_bwd', vid32, shallow32),
                 'half': lambda: op_backward('dcf_op_vidmap_shared_bwd_h', vid_h, shallow_h)},
    'round trip': {'fp32': lambda: trip(vid_h.float(), shallow_h.float()), 'half': lambda: trip(vid_h, shallow_h)},
}

# the bits first: a timing of two paths that disagree would compare nothing
op_forward('dcf_op_vidmap_shared', vid32, shallow32)
op_backward('dcf_op_vidmap_shared_bwd', vid32, shallow32)
want = (Y.clone(), dW.clone(), db.clone())
lb.check(lib.dcf_debug_set_option(b'half_native', 2), 'dcf_debug_set_option')          # native, or the call fails
op_forward('dcf_op_vidmap_shared_h', vid_h, shallow_h)
op_backward('dcf_op_vidmap_shared_bwd_h', vid_h, shallow_h)
assert all(torch.equal(a, b) for a, b in zip((Y, dW, db), want)), 'the half operators do not return the bits of the fp32 operators'

ntiles = (T + 63) // 64
kept = sum(bool(gate[b * K:(b + 1) * K, 64 * f:64 * f + 64].any()) for b in range(NVID) for f in range(ntiles))
skipped = 1.0 - kept / (NVID * ntiles)
feat = 2.0 * NVID * D * T                                                                   # feature values, both tensors
gemm = 2.0 * NVID * T * D * E * ((1.0 - skipped) + 1.0)                                      # one f16 product over the kept expert tiles + the shallow half
flops = {'forward': {'fp32': 3 * gemm, 'half': 2 * gemm}, 'backward': {'fp32': 3 * gemm, 'half': 2 * gemm}}
rows = 4.0 * (2 * NVID * T * E + nq * T * E)                                                 # the products / row sums (nvid, T, E) twice and the (B', T, E) rows
byts = {'forward': {'fp32': 4 * feat + rows, 'half': 2 * feat + rows}, 'backward': {'fp32': 4 * feat + 2 * rows, 'half': 2 * feat + 2 * rows}}
for k in ('fp32', 'half'):
    flops.setdefault('round trip', {})[k] = flops['forward'][k] + flops['backward'][k]
    byts.setdefault('round trip', {})[k] = byts['forward'][k] + byts['backward'][k] + (6 * feat if k == 'fp32' else 0.0)      # the upcast: 2 B read, 4 B written
say(f'front end on float16 features: D {D}, E {E}, msf, T {T}, {NVID} videos x {K} queries, sn {SN}, sratio {SRATIO}; '
    f'{100 * skipped:.1f} % of the {NVID * ntiles} 64-clip tiles are kept by no query; features {2 * feat / 1e6:.1f} MB as float16, {4 * feat / 1e6:.1f} MB as fp32')
say('    (matrix flops count every f16 product issued: three per k-step in the fp32 form, two in the half form; the round trip of the fp32 '
    'path adds the upcast pass, 2 + 4 bytes per value)')
for what, pair in paths.items():
    t = alternate(pair, args.window)
    peaks = {k: peak_of(fn) for k, fn in pair.items()}
    for k in ('fp32', 'half'):
        say(f'    {what:10s} {k:4s} {med(t[k]):9.1f} us (min {min(t[k]):.1f}, max {max(t[k]):.1f}); algorithmic {flops[what][k] / 1e9:7.2f} GFLOP, '
            f'{byts[what][k] / 1e6:8.1f} MB; peak allocated {peaks[k] / 2 ** 20:8.1f} MiB')
    say(f'    {what:10s} fp32 / half = {med(t["fp32"]) / med(t["half"]):.2f} in time, {peaks["fp32"] / max(peaks["half"], 1):.2f} in peak memory')
lb.check(lib.dcf_debug_set_option(b'half_native', -1), 'dcf_debug_set_option')

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
