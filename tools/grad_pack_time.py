"""Time of packing the default model's 449 gradients (14 512 236 elements) times 1 / world into the bucket arena of dist.GradReducer:

    (a) this package, device only: dcf_dist_pack_grads over the reducer's bucket tables, the tables already on the device
    (b) this package as a step runs it: GradReducer._launch per bucket (the host pass that gathers the gradients' addresses, the
        comparison with the table of the step before, the launch)
    (c) what it replaces: one torch.mul(grad, 1 / world, out=slice) per tensor, the copy DistributedDataParallel's reducer makes
        (pure torch: the same on a tree without the kernel)

Each sample is a window of WINDOW consecutive packs between device events, after warm-up; the paths alternate, REPEATS samples each,
median and range printed.  Then the launches of (a) from the library profiler (device events around each launch; for a kernel of a
few microseconds the events' own cost is a visible part of that figure -- a kernel trace of this tool gives the kernel alone) against
8 B per element as GB/s and as a share of the measured HBM copy rate (6.29 TB/s).  No process group: nothing is reduced here.

    python tools/grad_pack_time.py [--window 20] [--repeats 7] [--bucket-bytes N] [--out FILE]"""
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
D, lb = pkg.dist, pkg._lib
HBM_COPY = 6.29e12                      # B/s, measured float4 copy (the HBM row of the micro-architecture notes)

ap = argparse.ArgumentParser()
ap.add_argument('--window', type=int, default=20)
ap.add_argument('--repeats', type=int, default=7)
ap.add_argument('--bucket-bytes', type=int, default=D.DEFAULT_BUCKET_BYTES)
ap.add_argument('--out', default=None, help='also write the printed lines to this file')
args = ap.parse_args()
assert torch.cuda.is_available(), 'needs the GPU: there is nothing to time without it'
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


torch.manual_seed(0)
model = pkg.modeling.create_model(pkg.config.make_opt()).cuda()
params = [p for p in model.parameters() if p.requires_grad]
g = torch.Generator(device='cuda').manual_seed(1)
grads = [torch.randn(p.shape, device='cuda', generator=g) * 0.01 for p in params]
n_el = sum(p.numel() for p in params)
SCALE = 0.5


def give_grads():
    for p, x in zip(params, grads):
        p.grad = x


red = D.GradReducer(params, None, args.bucket_bytes)
K = len(red.plan['buckets'])
give_grads()
for k in range(K):
    red._launch(k)                      # builds and uploads the tables (scale 1: one rank)
lib = lb.lib()


def path_a():
    st = lb.current_stream()
    for t in red._tables:
        lb.check(lib.dcf_dist_pack_grads(*t.args(), SCALE, st), 'dcf_dist_pack_grads')


def path_b():
    for k in range(K):
        red._launch(k)


def path_c():
    for x, v in zip(grads, red.views):
        torch.mul(x, SCALE, out=v)


# the three paths write the same bits (b packs with scale 1 here: compared with a copy)
path_a()
got = red.arena.clone()
path_c()
assert torch.equal(got.view(torch.int32), red.arena.view(torch.int32)), 'dcf_dist_pack_grads and torch.mul differ'
path_b()
want = torch.zeros_like(red.arena)
for x, off in zip(grads, red.offsets):
    want[off:off + x.numel()] = x.reshape(-1)
assert torch.equal(want.view(torch.int32), red.arena.view(torch.int32)), 'the pack with scale 1 is not a copy'

paths = {'a': path_a, 'b': path_b, 'c': path_c}
say(f'default model: {len(params)} tensors, {n_el} elements, {K} bucket(s) of at most {args.bucket_bytes} bytes, arena {red.arena.numel()} floats; '
    f'window {args.window} packs, {args.repeats} samples per path, alternating')
for fn in paths.values():
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
names = {'a': f'dcf_dist_pack_grads, {K} launch(es), tables resident', 'b': 'GradReducer._launch per bucket (host pass + launch)',
         'c': f'torch.mul(out=) per tensor, {len(params)} launches'}
for k, v in times.items():
    say(f'({k}) {names[k]:55s} {med(v):9.1f} us per pack (min {min(v):.1f}, max {max(v):.1f})')
say(f'    (c) / (a) = {med(times["c"]) / med(times["a"]):.2f}   (c) / (b) = {med(times["c"]) / med(times["b"]):.2f}')

lib.dcf_profile_enable(1)
for _ in range(20):
    path_a()
torch.cuda.synchronize()
need = lib.dcf_profile_report(None, 0)
buf = ctypes.create_string_buffer(int(need) + 16)
lib.dcf_profile_report(buf, len(buf))
lib.dcf_profile_enable(0)
rep = json.loads(buf.value.decode())['dist_pack_grads']
us = 1e3 * rep['ms'] / rep['count'] * K                       # per pack of the whole set: K launches
b = 8.0 * n_el
say(f'    dist_pack_grads between its own device events: {us:8.1f} us per pack of the set ({rep["count"]} launches profiled), {b / 1e6:.1f} MB -> {b / us / 1e3:.0f} GB/s = '
    f'{100 * b / (us * 1e-6) / HBM_COPY:.0f} % of the HBM copy rate; the floor at that rate is {b / HBM_COPY * 1e6:.1f} us')

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
