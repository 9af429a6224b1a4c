"""Times of the training data path (data.FeatureBank / data.TrainLoader, dcf_op_assemble_rows) on the MI355X, recorded in
profiles/batch_assemble.md.  Nothing here is a gate.

1. Kernel: dcf_op_assemble_rows at B = 16, T_out = 2304, C = 1024, float16 and fp32, every window full (n = T_out) and a ragged
   set (n from 0.5 T_out to T_out, odd first rows), against a torch device-to-device ``copy_`` that moves the same bytes (the
   kernel's bytes are rows read + out + mask; the copy reads and writes half of that each) -- the ceiling of a pure move -- in the
   same run, alternating.  Each sample is a window of launches between device events.
2. Batch: the time per batch of ``TrainLoader`` with a bank and with ``bank=None`` (``collate_host`` + ``.cuda()``, features cached
   on the host as the reference caches them: a first pass over every video warms it), a device synchronise after every batch, on a
   generated tree of float16 files at the default widths (D = 1024, 300-channel tokens, videos of up to 2304 clips).
3. Step: ``TrainStep.step`` per iteration fed either way, batch included, at a tiny model and at the default one
   (``config.make_opt()``), ``front_end='shared'``.

    python tools/batch_assemble_time.py [--out FILE] [--videos 20] [--batch 16] [--step-batch 4] [--skip-default]"""
import argparse
import atexit
import importlib
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import train_data_tree as TT  # noqa: E402  (the generated tree of the tests, at other widths)

pkg = importlib.import_module('cvpr2025-decafnet_amd')
D, lb = pkg.data, pkg._lib

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=None, help='also append the printed lines to this file, as they come')
ap.add_argument('--videos', type=int, default=20)
ap.add_argument('--batch', type=int, default=16)
ap.add_argument('--step-batch', type=int, default=4, help='videos per step of the default model')
ap.add_argument('--window', type=int, default=20)
ap.add_argument('--repeats', type=int, default=15)
ap.add_argument('--skip-default', action='store_true', help='no step of the default model')
args = ap.parse_args()
assert torch.cuda.is_available(), 'needs the GPU: there is nothing to time without it'
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, 'w').close()


def say(s=''):
    print(s, flush=True)
    if args.out:
        with open(args.out, 'a') as f:
            f.write(s + '\n')


def stats(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def event_windows(fns, window, repeats):
    """{name: [us per call]}: the functions alternate, each sample ``window`` calls between device events"""
    for fn in fns.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(window):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / window)
    return times


# ------------------------------------------------------------------------------------------------------------------ 1. the kernel
B, T_OUT, C = 16, 2304, 1024
lib = lb.lib()
say(f'## kernel: B = {B}, T_out = {T_OUT}, C = {C}; window {args.window} launches, {args.repeats} samples per path, alternating')
for dtype in (torch.float16, torch.float32):
    es = torch.empty(0, dtype=dtype).element_size()
    rows = 24 * T_OUT + 1
    bank = torch.randn(rows, C, device='cuda').to(dtype)
    out = torch.empty(B, C, T_OUT, dtype=dtype, device='cuda')
    mask = torch.empty(B, T_OUT, dtype=torch.bool, device='cuda')
    g = np.random.default_rng(0)
    sets = {'full': [(int(g.integers(0, 24)) * T_OUT, T_OUT) for _ in range(B)],
            'ragged': [(int(g.integers(0, 24)) * T_OUT + 1, int(g.integers(T_OUT // 2, T_OUT + 1))) for _ in range(B)]}
    for tag, windows in sets.items():
        desc = torch.tensor([[r0 * C, n] for r0, n in windows], dtype=torch.int64, device='cuda')
        n_rows = sum(n for _, n in windows)
        nbytes = n_rows * C * es + out.numel() * es + mask.numel()
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device='cuda').random_()
        dst = torch.empty_like(src)

        def kernel():
            lb.check(lib.dcf_op_assemble_rows(lb.ptr(bank), es, lb.ptr(desc), B, C, T_OUT, lb.ptr(out), lb.ptr(mask), lb.current_stream()),
                     'dcf_op_assemble_rows')

        kernel()
        b0, (r0, n0) = B - 1, windows[-1]                                      # the timed launch computes the slicing
        assert torch.equal(out[b0, :, :n0], bank[r0:r0 + n0].t()) and not bool(out[b0, :, n0:].any()) and int(mask[b0].sum()) == n0
        t = event_windows({'kernel': kernel, 'copy': lambda: dst.copy_(src)}, args.window, args.repeats)
        (km, klo, khi), (cm, clo, chi) = stats(t['kernel']), stats(t['copy'])
        say(f'{str(dtype)[6:]:8s} {tag:6s} {nbytes / 1e6:7.1f} MB moved ({n_rows} rows read): kernel {km:7.1f} us (min {klo:.1f}, max {khi:.1f}) = '
            f'{nbytes / km / 1e3:6.0f} GB/s; copy_ of the same bytes {cm:7.1f} us (min {clo:.1f}, max {chi:.1f}) = {nbytes / cm / 1e3:6.0f} GB/s; '
            f'kernel / copy rate = {cm / km:.2f}')
    del bank, out, mask, src, dst

# ------------------------------------------------------------------------------------------------------------------ 2. the batch
say()
say(f'## batch: {args.videos} videos of up to {T_OUT} clips, D = {C}, float16 files, batch_size {args.batch}; a synchronise after every batch')
root = tempfile.mkdtemp(prefix='dcf_batch_time_')
atexit.register(shutil.rmtree, root, ignore_errors=True)
arrays, data = TT.random_tree(1, args.videos, C, 300, T_OUT, 48)
TT.write_tree(root, arrays, half=True)
del arrays
cfg = TT.cfg_of(root, dict(data, feature_dtype='stored'))
EPOCHS = 12


def batch_times(banked, batch_size, epochs=EPOCHS):
    td = D.VideoCentricTrainData(cfg, num_epochs=epochs, seed=0)
    t0 = time.perf_counter()
    if banked:
        bank = D.FeatureBank(td)
    else:
        bank = None
        for v in td.videos:                                                # warm host caches
            td.video_streams(v)
    torch.cuda.synchronize()
    fill = time.perf_counter() - t0
    loader = D.TrainLoader(td, bank, batch_size)
    times = []
    for e in range(epochs):
        it = loader.epoch(e)
        while True:
            t0 = time.perf_counter()
            got = next(it, None)
            torch.cuda.synchronize()
            if got is None:
                break
            times.append((time.perf_counter() - t0) * 1e3)
    return times[2:], fill, bank, len(td)


res = {}
for banked in (True, False, True, False):                                     # alternating, two passes each
    t, fill, bank, n = batch_times(banked, args.batch)
    res.setdefault(banked, []).extend(t)
    if banked:
        nb = bank.nbytes
    say(f'  {"banked" if banked else "host  "} pass: {len(t)} batches, {n} samples per epoch, '
        f'{"bank fill" if banked else "host cache warm-up"} {fill:.2f} s' + (f', bank {nb / 1e6:.0f} MB' if banked else ''))
    del bank
(bm, blo, bhi), (hm, hlo, hhi) = stats(res[True]), stats(res[False])
say(f'banked loader {bm:8.2f} ms per batch (min {blo:.2f}, max {bhi:.2f}, {len(res[True])} batches); host route {hm:8.2f} ms per batch '
    f'(min {hlo:.2f}, max {hhi:.2f}, {len(res[False])} batches); host / banked = {hm / bm:.1f}')

# ------------------------------------------------------------------------------------------------------------------ 3. the step
say()
say('## step: TrainStep.step per iteration, the batch included, front_end shared; a synchronise after every step')


def step_times(opt, the_cfg, batch_size, input_vid_len, vid_stride, steps, warm):
    """{banked: [ms per step]}: two TrainSteps on equal models, one fed each way, stepping in turn"""
    runs = {}
    for banked in (True, False):
        td = D.VideoCentricTrainData(the_cfg, num_epochs=steps + warm, seed=0)
        bank = D.FeatureBank(td) if banked else None
        if not banked:
            for v in td.videos:
                td.video_streams(v)
        loader = D.TrainLoader(td, bank, batch_size, input_vid_len=input_vid_len, vid_stride=vid_stride)
        model = pkg.modeling.create_model(opt)
        model.load_state_dict(pkg.synth.make_state_dict({k: list(v.shape) for k, v in model.state_dict().items()}, 2025))
        runs[banked] = (loader, pkg.train.TrainStep(model.cuda(), opt, itrs_per_epoch=max(len(loader), 1), front_end='shared'))
    out = {True: [], False: []}
    for e in range(steps + warm):
        for banked, (loader, ts) in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            batch, targets = next(loader.epoch(e))
            ts.step(batch, targets)
            torch.cuda.synchronize()
            if e >= warm:
                out[banked].append((time.perf_counter() - t0) * 1e3)
    return out


tiny_kw = dict(D=32, E=32, TE=32, text_in=32, n_levels=3, win=3, n_heads=2, sn=8, sratio=0.5, norm=True, max_seq_len=64, text_layers=2,
               text_max_len=24, text_use_abs_pe=True, n_stem=1, vid_stride=2, msf=True)
tiny_root = tempfile.mkdtemp(prefix='dcf_batch_time_tiny_')
atexit.register(shutil.rmtree, tiny_root, ignore_errors=True)
arrays, tiny_data = TT.random_tree(2, 8, 32, 32, 80, 9)
TT.write_tree(tiny_root, arrays, half=True)
cases = [('tiny (D 32, T 80, 4 videos per step)', pkg.config.make_opt(**tiny_kw), TT.cfg_of(tiny_root, dict(tiny_data, feature_dtype='stored')), 4, 80, 2, 20, 5)]
if not args.skip_default:
    # the training text embedding takes token widths that are multiples of 32: 512-channel tokens instead of the default 300
    big_root = tempfile.mkdtemp(prefix='dcf_batch_time_big_')
    atexit.register(shutil.rmtree, big_root, ignore_errors=True)
    arrays, big_data = TT.random_tree(3, 2 * args.step_batch, C, 512, T_OUT, 48)
    TT.write_tree(big_root, arrays, half=True)
    cases.append((f'default (config.make_opt(text_in=512), T {T_OUT}, {args.step_batch} videos per step)', pkg.config.make_opt(text_in=512),
                  TT.cfg_of(big_root, dict(big_data, feature_dtype='stored')), args.step_batch, T_OUT, 1, 6, 2))
del arrays
for name, opt, the_cfg, bs, T, vs, steps, warm in cases:
    t = step_times(opt, the_cfg, bs, T, vs, steps, warm)
    (bm, blo, bhi), (hm, hlo, hhi) = stats(t[True]), stats(t[False])
    say(f'{name}: fed from the bank {bm:9.2f} ms per step (min {blo:.2f}, max {bhi:.2f}); from the host route {hm:9.2f} ms (min {hlo:.2f}, max {hhi:.2f}); '
        f'{len(t[True])} steps each, in turn, after {warm} warm-up steps')
