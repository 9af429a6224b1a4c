"""Time of selected-clip inference (include/decafnet_hip_select.h) against the dense eval forward, on the probe model of bench.py
(D = 1024, E = 256, 8 levels, window 9, sn = 60, sratio = 0.3, synthetic weights) at T = 16 384 with one and with four queries:

    dense      model(vid, shallow, ..., eval=True) on dense (1, D, T) expert features
    select     model.select_clips(shallow, mask, text_cls): scores, gate, compaction and the one host read of the count
    selected   model.forward_selected(rows, selection, shallow, ...) on the (count, D) rows of the selected clips
    gather     model.gather_clip_rows(vid, selection): the emulation path that makes those rows from dense features
    compact    dcf_op_select_clips alone on the selection's gate, outputs allocated once: the compaction kernel without the host read

The five paths take turns in one process, device events around each sample of --window calls after a warm-up; the median and the range
of --repeats samples are printed, with count / vid_len and the bytes of expert features each forward reads.  Nothing is asserted.

    python tools/select_time.py [--repeats 7] [--window 10] [--half] [--out FILE]"""
import argparse
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module('cvpr2025-decafnet_amd')

ap = argparse.ArgumentParser()
ap.add_argument('--repeats', type=int, default=7)
ap.add_argument('--window', type=int, default=10, help='calls per sample')
ap.add_argument('--T', type=int, default=16384)
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


T, D = args.T, 1024
kw = dict(D=D, E=256, TE=256, text_in=512, n_levels=8, win=9, n_heads=4, sn=60, sratio=0.3, msf=True, norm=True, max_seq_len=2304,
          text_layers=5, text_max_len=48, fusion_layers=2)
opt = pkg.config.make_opt(**kw)
model = pkg.modeling.create_model(opt)
model.load_state_dict(pkg.synth.make_state_dict({k: list(v.shape) for k, v in model.state_dict().items()}, 2025))
model = model.cuda().eval().requires_grad_(False)
esz = 2 if args.half else 4
say(f'probe model D {D} E 256, T {T} (every clip valid), features {"float16" if args.half else "fp32"}; us per call, median (min .. max) of '
    f'{args.repeats} samples of {args.window} calls')
say(f'{"nq":>3} {"dense":>24} {"select":>24} {"selected":>24} {"gather":>22} {"compact":>22} {"count/vid_len":>14} {"expert MB dense":>16} {"selected":>9}')
for nq in (1, 4):
    inp = pkg.synth.make_inputs(D, T, T, nq, 512, 16, 4000 + nq)
    tm = [model.encode_text(t[None].cuda(), torch.ones(1, 1, t.size(-1), dtype=torch.bool, device='cuda')) for t in inp['tokens']]
    texts, tmasks = tuple(t for t, _ in tm), tuple(m for _, m in tm)
    vid, sh, vm, cls = (inp[k].cuda() for k in ('vid', 'shallow_vid', 'vid_masks', 'text_cls'))
    if args.half:
        vid, sh = vid.half(), sh.half()
    sel = model.select_clips(sh, vm, cls)
    rows = model.gather_clip_rows(vid, sel)
    lb, lib = pkg._lib, pkg._lib.lib()
    vmb = vm.reshape(-1).contiguous()
    c_clips, c_pos, c_count = (torch.empty(n, dtype=torch.int32, device='cuda') for n in (T, T, 1))
    compact = lambda: lb.check(lib.dcf_op_select_clips(lb.ptr(sel.gate), lb.ptr(vmb), T, nq, lb.ptr(c_clips), lb.ptr(c_pos), lb.ptr(c_count),
                                                       lb.current_stream()), 'dcf_op_select_clips')
    paths = {'dense': lambda: model(vid, sh, vm, texts, cls, tmasks, eval=True),
             'select': lambda: model.select_clips(sh, vm, cls),
             'selected': lambda: model.forward_selected(rows, sel, sh, vm, texts, tmasks),
             'gather': lambda: model.gather_clip_rows(vid, sel), 'compact': compact}
    t = alternate(paths, args.window)
    cell = lambda n, w: f'{med(t[n]):9.1f} ({min(t[n]):.1f} .. {max(t[n]):.1f})'.rjust(w)
    say(f'{nq:>3} {cell("dense", 24)} {cell("select", 24)} {cell("selected", 24)} {cell("gather", 22)} {cell("compact", 22)} {sel.count / T:>14.3f} '
        f'{D * T * esz / 1e6:>16.1f} {sel.count * D * esz / 1e6:>9.1f}')
    say(f'    nq {nq}: select + selected = {med(t["select"]) + med(t["selected"]):.1f} us against dense {med(t["dense"]):.1f} us; the dense forward was '
        f'issued {"as a HIP graph" if (model(vid, sh, vm, texts, cls, tmasks, eval=True), model.graph_active())[1] else "eagerly"}, '
        f'the selected one always eagerly')
assert model.numerics_status() & 1 == 0

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
