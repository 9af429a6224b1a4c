"""Time of selected-clip inference on several videos per forward (include/decafnet_hip_select_videos.h) against the one-video pattern
called once per video and against the dense several-video forward, on the probe model of bench.py (D = 1024, E = 256, 8 levels,
window 9, sn = 60, sratio = 0.3, synthetic weights) at T = 16 384, 8 videos of one and of four queries each:

    select x8     model.select_clips per video: 8 calls, 8 host reads
    select_v      model.select_clips_videos: one call, one host read
    compact x8    dcf_op_select_clips on each video's gate, outputs allocated once: 8 launches, no host read
    compact_v     dcf_op_select_clips_videos on the same gates: one launch of 8 workgroups
    dense_v       model.forward_videos on dense (1, D, T) expert features
    selected x8   model.forward_selected per video on its (count, D) rows
    selected_v    model.forward_videos_selected on the packed rows of all videos
    gather_v      model.gather_clip_rows_videos: the emulation path that makes the packed rows from dense features

The paths take turns in one process, device events around each sample of --window calls after a warm-up; the median and the range of
--repeats samples are printed, with count / vid_len, the bytes of expert features each forward reads and the kernel name of the
packed expert product (the library's per-launch profile).  The one-video paths are the parent commit's code.  Nothing is asserted.

    python tools/select_videos_time.py [--repeats 7] [--window 5] [--half] [--out FILE]"""
import argparse
import ctypes
import importlib
import json
import os
import sys

import torch

os.environ.setdefault('DCF_PROF_SHAPES', '1')      # the profile labels of the split-operand GEMMs carry [count x M x N x K]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module('cvpr2025-decafnet_amd')

ap = argparse.ArgumentParser()
ap.add_argument('--repeats', type=int, default=7)
ap.add_argument('--window', type=int, default=5, help='calls per sample')
ap.add_argument('--T', type=int, default=16384)
ap.add_argument('--videos', type=int, default=8)
ap.add_argument('--half', action='store_true', help='float16 features (vid, shallow and the rows)')
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


def kernels_of(fn):
    """the library's per-launch profile of one call of fn: {kernel name: launches}"""
    lib = pkg._lib.lib()
    lib.dcf_profile_enable(1)
    fn()
    torch.cuda.synchronize()
    need = lib.dcf_profile_report(None, 0)
    buf = ctypes.create_string_buffer(int(need) + 16)
    lib.dcf_profile_report(buf, len(buf))
    lib.dcf_profile_enable(0)
    return {k: v['count'] for k, v in json.loads(buf.value.decode()).items()}


T, D, NV = args.T, 1024, args.videos
kw = dict(D=D, E=256, TE=256, text_in=512, n_levels=8, win=9, n_heads=4, sn=60, sratio=0.3, msf=True, norm=True, max_seq_len=2304,
          text_layers=5, text_max_len=48, fusion_layers=2)
opt = pkg.config.make_opt(**kw)
opt.model['max_batch'] = 16
model = pkg.modeling.create_model(opt)
model.load_state_dict(pkg.synth.make_state_dict({k: list(v.shape) for k, v in model.state_dict().items()}, 2025))
model = model.cuda().eval().requires_grad_(False)
esz = 2 if args.half else 4
lb, lib = pkg._lib, pkg._lib.lib()
say(f'probe model D {D} E 256, {NV} videos of T {T} (every clip valid), features {"float16" if args.half else "fp32"}, max_batch 16; us per call, '
    f'median (min .. max) of {args.repeats} samples of {args.window} calls')
for nq in (1, 4):
    if NV * nq > 16:
        say(f'nq {nq}: {NV * nq} queries run as chunks of 16 (a chunk may span videos)')
    videos = []
    for v in range(NV):
        inp = pkg.synth.make_inputs(D, T, T, nq, 512, 16, 5000 + 10 * nq + v)
        tm = [model.encode_text(t[None].cuda(), torch.ones(1, 1, t.size(-1), dtype=torch.bool, device='cuda')) for t in inp['tokens']]
        vid, sh = inp['vid'].cuda(), inp['shallow_vid'].cuda()
        if args.half:
            vid, sh = vid.half(), sh.half()
        videos.append((vid, sh, inp['vid_masks'].cuda(), tuple(t for t, _ in tm), inp['text_cls'].cuda(), tuple(m for _, m in tm)))
    sels = [model.select_clips(a[1], a[2], a[4]) for a in videos]
    rows1 = [model.gather_clip_rows(a[0], s) for a, s in zip(videos, sels)]
    batch = model.select_clips_videos(videos)
    if batch.counts != [s.count for s in sels]:
        say(f'    (the counts of the one call {batch.counts} differ from the per-video calls {[s.count for s in sels]})')
    rows = model.gather_clip_rows_videos([a[0] for a in videos], batch)
    masks = torch.stack([a[2].reshape(-1) for a in videos]).contiguous()
    o1 = [tuple(torch.empty(n, dtype=torch.int32, device='cuda') for n in (T, T, 1)) for _ in range(NV)]
    ov = tuple(torch.empty(n, dtype=torch.int32, device='cuda') for n in (NV * T, NV * T, NV))
    nqs = (ctypes.c_int32 * NV)(*([nq] * NV))

    def compact_each():
        for v in range(NV):
            lb.check(lib.dcf_op_select_clips(lb.ptr(sels[v].gate), lb.ptr(masks[v]), T, nq, lb.ptr(o1[v][0]), lb.ptr(o1[v][1]), lb.ptr(o1[v][2]),
                                             lb.current_stream()), 'dcf_op_select_clips')

    def compact_videos():
        lb.check(lib.dcf_op_select_clips_videos(lb.ptr(batch.gate), lb.ptr(masks), T, NV, nqs, lb.ptr(ov[0]), lb.ptr(ov[1]), lb.ptr(ov[2]),
                                                lb.current_stream()), 'dcf_op_select_clips_videos')

    def selected_each():
        for a, s, r in zip(videos, sels, rows1):
            model.forward_selected(r, s, a[1], a[2], a[3], a[5])

    paths = {'select x8': lambda: [model.select_clips(a[1], a[2], a[4]) for a in videos],
             'select_v': lambda: model.select_clips_videos(videos),
             'compact x8': compact_each, 'compact_v': compact_videos,
             'dense_v': lambda: model.forward_videos(videos),
             'selected x8': selected_each,
             'selected_v': lambda: model.forward_videos_selected(rows, batch, videos),
             'gather_v': lambda: model.gather_clip_rows_videos([a[0] for a in videos], batch)}
    t = alternate(paths, args.window)
    say(f'nq {nq} per video, {NV * nq} queries: count / vid_len {batch.n_rows / (NV * T):.3f} (per video {min(batch.counts) / T:.3f} .. '
        f'{max(batch.counts) / T:.3f}); expert features read: dense {NV * D * T * esz / 1e6:.1f} MB, selected {batch.n_rows * D * esz / 1e6:.1f} MB')
    for name in paths:
        say(f'    {name:<12} {med(t[name]):10.1f} ({min(t[name]):.1f} .. {max(t[name]):.1f})')
    model.forward_videos(videos)
    say(f'    the dense forward was issued {"as a HIP graph" if model.graph_active() else "eagerly"}, the selected ones always eagerly')
    packed = [k for k in kernels_of(lambda: model.forward_videos_selected(rows, batch, videos)) if f'x{batch.n_rows}x' in k]
    single = [k for k in kernels_of(lambda: model.forward_selected(rows1[0], sels[0], videos[0][1], videos[0][2], videos[0][3], videos[0][5]))
              if f'x{sels[0].count}x' in k]
    say(f'    packed expert product ({batch.n_rows} rows): {packed or "no kernel name carries the shape"}; one video ({sels[0].count} rows): '
        f'{single or "no kernel name carries the shape"}')
assert model.numerics_status() & 1 == 0

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
