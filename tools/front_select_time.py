"""Time and saved-tensor bytes of vid_map of the training step on the expert rows of the selected clips (``autograd.selected_vid_map``,
include/decafnet_hip_front_select.h) against the same stage on dense expert features (``autograd.gated_vid_map``,
include/decafnet_hip_front.h), at the bench shape: one video of T = 16384 clips, D = 1024, E = 256, msf, 8 queries, sn = 60,
sratio = 0.3, the gates of dcf_op_sidekick / dcf_op_gate on seeded features; fp32 and float16 features.  The queries are independent
random vectors, so eight of them keep 1 - 0.7^8 = 94 % of the blocks between them; ``--queries 1`` is the other end (30 %).

    round trip   forward + backward through autograd, the weight and the bias asking for their gradients
    forward / backward   the exports alone, and the float16 backward with the rows 2 bytes off the 16-byte grid (2-byte loads)
    saved        the bytes of the tensors each autograd function keeps for its backward (counted from the tensors themselves)
    host         the host time of a round trip: the wall clock over calls that are only enqueued (a sync before and after the loop)
    selection    dcf_op_select_clips_videos and the host read of the counts, which only the selected path pays; the gather that emulates an
                 expert encoder (dcf_op_gather_clip_rows_videos) is timed apart: a caller with an online encoder does not run it

The two paths alternate in one process, device events around each sample, warm-up, REPEATS samples of WINDOW calls; median and range
printed.  Before any timing the results of the two paths are compared (they differ in the summation order of the expert half only).

    python tools/front_select_time.py [--queries 8] [--repeats 7] [--window 5] [--out FILE]"""
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
A, lb = pkg.autograd, pkg._lib

ap = argparse.ArgumentParser()
ap.add_argument('--queries', type=int, default=8)
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


D, E, T, NVID, K, SN, SRATIO = 1024, 256, 16384, 1, args.queries, 60, 0.3
sizes = [K] * NVID
nq = sum(sizes)
g = torch.Generator().manual_seed(7)
vid_h = torch.randn(NVID, D, T, generator=g).half().cuda()
shallow_h = torch.randn(NVID, D, T, generator=g).half().cuda()
text_cls = torch.randn(nq, D, generator=g).cuda()
vm = torch.ones(NVID, T, dtype=torch.bool, device='cuda')
lib, st, p = lb.lib(), lb.current_stream(), lb.ptr
gates, masks = [], []
for b in range(NVID):
    correl = torch.empty(K, T, device='cuda')
    lb.check(lib.dcf_op_sidekick_h(p(shallow_h[b].contiguous()), p(text_cls[b * K:(b + 1) * K].contiguous()), p(correl), D, T, K, 1, st), 'dcf_op_sidekick_h')
    gate, mo = torch.empty(K, T, device='cuda'), torch.empty(K, T, dtype=torch.bool, device='cuda')
    lb.check(lib.dcf_op_gate(p(correl), p(vm[b].contiguous()), p(gate), p(mo), T, K, SN, SRATIO, 1, st), 'dcf_op_gate')
    gates.append(gate), masks.append(mo)
gate, mask = torch.cat(gates), torch.cat(masks)
host_nq = torch.tensor(sizes, dtype=torch.int32)
nq_ptr = ctypes.cast(host_nq.data_ptr(), lb._IP)
clips, pos = torch.empty(NVID, T, dtype=torch.int32, device='cuda'), torch.empty(NVID, T, dtype=torch.int32, device='cuda')
counts = torch.empty(NVID, dtype=torch.int32, device='cuda')


def select():
    lb.check(lib.dcf_op_select_clips_videos(p(gate), p(vm), T, NVID, nq_ptr, p(clips), p(pos), p(counts), st), 'dcf_op_select_clips_videos')
    return counts.cpu().tolist()                                    # the ONE host read of the pattern


cnt = select()
first = [0]
for c in cnt:
    first.append(first[-1] + c)
n_rows = first[-1]
host_first = (ctypes.c_int32 * (NVID + 1))(*first)


def gather(x, rows, name):
    ptrs = (ctypes.c_void_p * NVID)(*[x[b].data_ptr() for b in range(NVID)])
    lb.check(getattr(lib, name)(ptrs, T, p(clips), T, NVID, host_first, D, p(rows), st), name)
    return rows


rows_h = gather(vid_h, torch.empty(n_rows, D, dtype=torch.float16, device='cuda'), 'dcf_op_gather_clip_rows_videos_h')
feats = {'fp32': (vid_h.float(), shallow_h.float(), rows_h.float()), 'float16': (vid_h, shallow_h, rows_h)}
weight = torch.nn.Parameter(torch.randn(E, 2 * D, 1, generator=g).cuda() * (2 * D) ** -0.5)
bias = torch.nn.Parameter(torch.randn(E, generator=g).cuda() * 0.1)
dY = torch.randn(nq, T, E, generator=g).cuda() * 1e-3


def trip(kind, v, s, r):
    weight.grad = bias.grad = None
    y = A.gated_vid_map(v, s, gate, mask, None, sizes, weight, bias) if kind == 'dense' else \
        A.selected_vid_map(r, first, pos, s, gate, mask, None, sizes, weight, bias)
    y.backward(dY)
    return y


def saved_bytes(kind, v, s, r):
    y = A.gated_vid_map(v, s, gate, mask, None, sizes, weight, bias) if kind == 'dense' else \
        A.selected_vid_map(r, first, pos, s, gate, mask, None, sizes, weight, bias)
    seen, total = set(), 0
    for t in y.grad_fn.saved_tensors:
        if t.data_ptr() not in seen:
            seen.add(t.data_ptr())
            total += t.numel() * t.element_size()
    return total


say(f'vid_map of the training step, dense against selected expert features: D {D}, E {E}, msf, T {T}, {NVID} video x {K} queries, sn {SN}, '
    f'sratio {SRATIO}; the queries keep {n_rows} of {NVID * T} clips ({100.0 * n_rows / (NVID * T):.1f} %)')
for name, (v, s, r) in feats.items():
    yd = trip('dense', v, s, r).detach().clone()
    gd = (weight.grad.clone(), bias.grad.clone())
    ys = trip('selected', v, s, r).detach()
    rel = lambda a, b: float((a - b).abs().max()) / float(b.abs().max())
    say(f'  {name}: selected against dense, max |difference| / max |dense|: Y {rel(ys, yd):.2e}, dW {rel(weight.grad, gd[0]):.2e}, db {rel(bias.grad, gd[1]):.2e}')
    assert rel(ys, yd) < 1e-5 and rel(weight.grad, gd[0]) < 1e-5 and torch.equal(bias.grad, gd[1]), 'the two paths disagree: nothing to time'
    t = alternate({'dense': lambda: trip('dense', v, s, r), 'selected': lambda: trip('selected', v, s, r)}, args.window)
    sb = {k: saved_bytes(k, v, s, r) for k in ('dense', 'selected')}
    for k in ('dense', 'selected'):
        say(f'    round trip {k:8s} {med(t[k]):9.1f} us (min {min(t[k]):.1f}, max {max(t[k]):.1f}); saved for the backward {sb[k] / 2 ** 20:8.1f} MiB')
    say(f'    round trip dense / selected = {med(t["dense"]) / med(t["selected"]):.2f} in time, {sb["dense"] / sb["selected"]:.2f} in saved bytes')
# the exports alone
W2 = weight.detach().reshape(E, 2 * D).contiguous()
Y, dW, db = torch.empty(nq, T, E, device='cuda'), torch.empty(E, 2 * D, device='cuda'), torch.empty(E, device='cuda')
off = torch.empty(n_rows * D + 8, dtype=torch.float16, device='cuda')
rows_off = off[1:1 + n_rows * D].view(n_rows, D)
rows_off.copy_(rows_h)


def sel_fwd(name, r, s):
    lb.check(getattr(lib, name)(p(r), host_first, p(pos), p(s), p(W2), p(bias), p(gate), p(mask), None, nq_ptr, p(Y), NVID, D, T, E, st), name)


def sel_bwd(name, r, s):
    lb.check(getattr(lib, name)(p(r), host_first, p(pos), p(s), p(gate), p(mask), None, nq_ptr, p(dY), p(dW), p(db), NVID, D, T, E, 0, st), name)


def sh_fwd(name, v, s):
    lb.check(getattr(lib, name)(p(v), p(s), p(W2), p(bias), p(gate), p(mask), None, nq_ptr, p(Y), NVID, D, T, E, 0, st), name)


def sh_bwd(name, v, s):
    lb.check(getattr(lib, name)(p(v), p(s), p(gate), p(mask), None, nq_ptr, p(dY), p(dW), p(db), NVID, D, T, E, 0, 0, st), name)


v32, s32, r32 = feats['fp32']
ops = {'forward': {'dense fp32': lambda: sh_fwd('dcf_op_vidmap_shared', v32, s32), 'selected fp32': lambda: sel_fwd('dcf_op_vidmap_selected', r32, s32),
                   'dense float16': lambda: sh_fwd('dcf_op_vidmap_shared_h', vid_h, shallow_h),
                   'selected float16': lambda: sel_fwd('dcf_op_vidmap_selected_h', rows_h, shallow_h)},
       'backward': {'dense fp32': lambda: sh_bwd('dcf_op_vidmap_shared_bwd', v32, s32), 'selected fp32': lambda: sel_bwd('dcf_op_vidmap_selected_bwd', r32, s32),
                    'dense float16': lambda: sh_bwd('dcf_op_vidmap_shared_bwd_h', vid_h, shallow_h),
                    'selected float16': lambda: sel_bwd('dcf_op_vidmap_selected_bwd_h', rows_h, shallow_h),
                    'selected float16, rows + 2 B': lambda: sel_bwd('dcf_op_vidmap_selected_bwd_h', rows_off, shallow_h)}}
for what, group in ops.items():
    t = alternate(group, args.window)
    for k in group:
        say(f'    {what:8s} {k:28s} {med(t[k]):9.1f} us (min {min(t[k]):.1f}, max {max(t[k]):.1f})')
pairs = {k: (lambda k=k: (ops['forward'][k](), ops['backward'][k]())) for k in ops['forward']}
t = alternate(pairs, args.window)
for k in pairs:
    say(f'    forward then backward export, {k:18s} {med(t[k]):9.1f} us (min {min(t[k]):.1f}, max {max(t[k]):.1f})')
for name, (v, s, r) in feats.items():                              # what the host spends on a round trip
    for kind in ('dense', 'selected'):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            trip(kind, v, s, r)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        say(f'    host time of a round trip, {name:7s} {kind:8s}: {(t1 - t0) / 20 * 1e6:8.1f} us enqueue, {(t2 - t0) / 20 * 1e6:8.1f} us with the final sync')
t = alternate({'select': select, 'gather': lambda: gather(vid_h, rows_h, 'dcf_op_gather_clip_rows_videos_h')}, args.window)
say(f'  selection (compaction + the host read of the counts) {med(t["select"]):.1f} us (min {min(t["select"]):.1f}, max {max(t["select"]):.1f}); '
    f'gather of the float16 rows from dense features (emulation only) {med(t["gather"]):.1f} us')

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
