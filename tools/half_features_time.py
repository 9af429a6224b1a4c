"""Time of the eval forward on fp32 and on binary16 clip features (include/decafnet_hip_half.h), at the benchmark shape D = 1024,
E = 256, T = 16 384:

    (i)   the front-end launches alone -- the shallow halves of vid_map with the scores on their side, the gate, the expert halves (and,
          where a path has one, the scoring kernels or the upcast) -- for 1 and for 8 videos of one query: the device events the engine
          records around each launch under dcf_profile_enable, summed per forward;
    (ii)  the whole 8-video forward (``forward_videos``, static output buffers, the engine's own graph policy), features resident;
    (iii) ``GroundingEvaluator.forward`` per video from pageable host tensors (``prepare`` = pad + upload + encode_text, then the
          forward), host clock around the call and a device synchronise: fp32 features; features stored as float16; fp32 features
          cast on the host by ``feature_dtype='float16'``;
    (iv)  what rounding fp32 features to binary16 does to the results, on the e2e fixtures of tests/golden and on one case with
          unit-length clips: max |delta| of the logits over the valid points and how many of the top-5 proposals (soft-NMS, by rank)
          keep their segment.  Recorded, not asserted.

The paths alternate in one process; warm-up first; ``--repeats`` samples each; median (min, max).

    python tools/half_features_time.py [--repeats 7] [--out FILE.json] [--T 16384]"""
import argparse
import ctypes
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
pkg = importlib.import_module('cvpr2025-decafnet_amd')
lb = pkg._lib

ap = argparse.ArgumentParser()
ap.add_argument('--repeats', type=int, default=7)
ap.add_argument('--T', type=int, default=16384)
ap.add_argument('--out', default=None, help='write the samples as JSON to this file')
args = ap.parse_args()
assert torch.cuda.is_available(), 'needs the GPU: there is nothing to time without it'
lib = lb.lib()
result = {'T': args.T, 'repeats': args.repeats, 'device': torch.cuda.get_device_name(0)}


def med(v):
    return sorted(v)[len(v) // 2]


def line(tag, v, unit='us'):
    print(f'    {tag:34s} {med(v):10.1f} {unit} (min {min(v):.1f}, max {max(v):.1f})', flush=True)


KW = dict(D=1024, E=256, TE=256, text_in=512, n_levels=8, win=9, n_heads=4, sn=60, sratio=0.3, msf=True, norm=True, max_seq_len=2304,
          text_layers=5, text_max_len=48, fusion_layers=2)
T = args.T


def make_model(kw, seed=2025):
    opt = pkg.config.make_opt(**kw)
    model = pkg.modeling.create_model(opt)
    model.load_state_dict(pkg.synth.make_state_dict({k: list(v.shape) for k, v in model.state_dict().items()}, seed))
    return opt, model.cuda().eval().requires_grad_(False)


opt, model = make_model(KW)
model.reuse_output_buffers = True
FRONT = ('chanmajor', 'gate_topk', 'sidekick_score', 'half_to_f32')


def videos_of(n, dtype):
    out = []
    for j in range(n):
        inp = pkg.synth.make_inputs(KW['D'], T, T if j != 5 else T - 383, 1, KW['text_in'], 32, 2025 + 3 + 100000 * j)
        tm = [model.encode_text(t[None].cuda(), torch.ones(1, 1, t.size(-1), dtype=torch.bool, device='cuda')) for t in inp['tokens']]
        vid, sh = inp['vid'].half(), inp['shallow_vid'].half()                  # both paths read the same binary16-representable values
        out.append((vid.to(dtype).cuda(), sh.to(dtype).cuda(), inp['vid_masks'].cuda(), tuple(t for t, _ in tm), inp['text_cls'].cuda(),
                    tuple(m for _, m in tm)))
    return out


def front_ms(videos):
    """one forward under the per-launch profiler -> (ms of the front-end launches, their names)"""
    lb.check(lib.dcf_profile_enable(1), 'dcf_profile_enable')
    model.forward_videos(videos)
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(1 << 16)
    lib.dcf_profile_report(buf, len(buf))
    lb.check(lib.dcf_profile_enable(0), 'dcf_profile_enable')
    rep = json.loads(buf.value.decode())
    front = {k: v for k, v in rep.items() if any(s in k for s in FRONT)}
    return sum(v['ms'] for v in front.values()), {k: round(v['ms'] * 1e3, 1) for k, v in front.items()}


# ---------------------------------------------------------------------------------------------- (i) and (ii)
for n in (1, 8):
    sets = {'fp32': videos_of(n, torch.float32), 'half': videos_of(n, torch.float16)}
    for v in sets.values():
        for _ in range(2):
            front_ms(v)
    times, names = {k: [] for k in sets}, {}
    for _ in range(args.repeats):
        for k, v in sets.items():
            ms, names[k] = front_ms(v)
            times[k].append(ms * 1e3)
        assert model.last_feature_dtype is torch.float16
    print(f'(i) front-end launches of one forward, {n} video(s) x 1 query, D {KW["D"]}, E {KW["E"]}, T {T}: sum of the per-launch device events', flush=True)
    for k in sets:
        line(k, times[k])
        print(f'        launches (us, last sample): {names[k]}', flush=True)
    result[f'front_{n}'] = dict(times_us=times, launches_us=names)
    if n == 8:
        for v in sets.values():                                      # eager, capture, replay
            for _ in range(4):
                model.forward_videos(v)
        torch.cuda.synchronize()
        whole = {k: [] for k in sets}
        for _ in range(args.repeats):
            for k, v in sets.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                model.forward_videos(v)                              # (the other path's graph was replaced: this call captures again)
                model.forward_videos(v)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(5):
                    model.forward_videos(v)
                e1.record()
                e1.synchronize()
                whole[k].append(e0.elapsed_time(e1) * 1e3 / 5)
        print(f'(ii) whole forward of 8 videos x 1 query (graph_active = {model.graph_active()}), per forward', flush=True)
        for k in sets:
            line(k, whole[k])
        result['forward_8'] = dict(times_us=whole)
    del sets
    torch.cuda.empty_cache()

# ---------------------------------------------------------------------------------------------- (iii) the evaluator from host memory
opt.model['max_vid_len'] = T
g = torch.Generator().manual_seed(9)
host = dict(vid=torch.randn(KW['D'], T - 100, generator=g), shallow_vid=torch.randn(KW['D'], T - 100, generator=g),
            text=(torch.randn(KW['text_in'], 32, generator=g),), text_cls=torch.randn(1, KW['D'], generator=g), fps=30.0, clip_stride=16,
            clip_size=32, duration=1e5, clip_id='host')
host16 = dict(host, vid=host['vid'].half(), shallow_vid=host['shallow_vid'].half())
paths = {'fp32 features': (pkg.evaluator.GroundingEvaluator(opt, model), host),
         'float16 features as stored': (pkg.evaluator.GroundingEvaluator(opt, model), host16),
         "fp32 features, feature_dtype='float16'": (pkg.evaluator.GroundingEvaluator(opt, model, feature_dtype='float16'), host)}
for ev, data in paths.values():
    for _ in range(2):
        ev.forward(data)
torch.cuda.synchronize()
ev_times = {k: [] for k in paths}
prep = {k: [] for k in paths}
for _ in range(args.repeats):
    for k, (ev, data) in paths.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        args_, _, _ = ev.prepare(data)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        model(*args_, eval=True)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        prep[k].append((t1 - t0) * 1e6)
        ev_times[k].append((t2 - t0) * 1e6)
print(f'(iii) GroundingEvaluator: prepare + forward of one video x 1 query from pageable host tensors, D {KW["D"]}, T {T} (host clock, synchronised)', flush=True)
for k in paths:
    line(k, ev_times[k])
    line('    of which prepare', prep[k])
result['evaluator'] = dict(total_us=ev_times, prepare_us=prep)
del model, paths
torch.cuda.empty_cache()

# ---------------------------------------------------------------------------------------------- (iv) the effect of rounding
from conftest import Golden  # noqa: E402


def proposals(ev, data):
    return ev.predict(data)


def rounding(tag, kw, meta, shapes, unit=False):
    o = pkg.config.make_opt(**kw)
    o.model['max_vid_len'] = meta['T']
    m = pkg.modeling.create_model(o)
    m.load_state_dict(pkg.synth.make_state_dict(shapes, meta['wseed']))
    m = m.cuda().eval().requires_grad_(False)
    inp = pkg.synth.make_inputs(meta.get('feat_dim', kw['D']), meta['T'], meta['vid_len'], meta['nq'], kw['text_in'], meta['lq'], meta['iseed'])
    vid, sh = inp['vid'][0, :, :meta['vid_len']], inp['shallow_vid'][0, :, :meta['vid_len']]
    if unit:
        vid, sh = torch.nn.functional.normalize(vid, dim=0), torch.nn.functional.normalize(sh, dim=0)
    data = dict(vid=vid, shallow_vid=sh, text=tuple(inp['tokens']), text_cls=inp['text_cls'], fps=30.0, clip_stride=16, clip_size=32,
                duration=1e5, clip_id=tag)
    ev = pkg.evaluator.GroundingEvaluator(o, m)
    a = ev.predict(data)
    la, _, ma = [x.clone() for x in m._last_flat]
    b = ev.predict(dict(data, vid=vid.half(), shallow_vid=sh.half()))
    lb_, _, mb = [x.clone() for x in m._last_flat]
    assert m.last_feature_dtype is torch.float16
    both = ma & mb
    dmax = float((la - lb_)[both].abs().max())
    keep = 0
    total = 0
    for qa, qb in zip(a, b):
        n = min(5, len(qa['segments']), len(qb['segments']))
        total += min(5, len(qa['segments']))
        keep += int(((qa['segments'][:n].cpu() - qb['segments'][:n].cpu()).abs().amax(1) <= 1e-3).sum()) if n else 0
    rec = dict(max_abs_dlogit=dmax, max_abs_logit=float(la[both].abs().max()), masks_equal=bool(torch.equal(ma, mb)), top5_same_segment=keep, top5_total=total)
    print(f'    {tag:18s} max |d logit| {dmax:.3e} (max |logit| {rec["max_abs_logit"]:.2f}), masks equal {rec["masks_equal"]}, '
          f'top-5 proposals with the same segment {keep} / {total}', flush=True)
    return rec


print('(iv) fp32 features against the same features rounded to binary16 (not asserted)', flush=True)
result['rounding'] = {}
for name in ('c1', 'pe', 'nomsf', 'scat', 'sfonly', 'affine'):
    gfix = Golden(f'e2e_{name}.npz')
    result['rounding'][name] = rounding(name, gfix.js('opt_kwargs'), gfix.js('meta'), gfix.js('shapes'))
gfix = Golden('e2e_c1.npz')
result['rounding']['c1, unit clips'] = rounding('c1, unit clips', gfix.js('opt_kwargs'), gfix.js('meta'), gfix.js('shapes'), unit=True)

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(result, fh, indent=1)
