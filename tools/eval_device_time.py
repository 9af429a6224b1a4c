"""Time per video of ``GroundingEvaluator.run`` on the MI355X by three routes, recorded in profiles/eval_device.md.  Nothing here is a
gate.

    host      the host-fed route: per-video dicts of host tensors (loaded once and kept in a list, as the reference caches features),
              ``RecallCounter``: pad on the host, two uploads, one pinned copy and one event wait per video, the metric in numpy
    bank      ``data.EvalBank`` items with a host ``RecallCounter``: windows assembled on the GPU, still the copy and the wait per video
    device    ``data.EvalBank`` items with ``DeviceRecallCounter``: nothing is read back before the end of the pass

A generated tree at the widths of BASELINE config 3: T = 16 384 clips, D = 1024, 4 queries per video, 16 videos, float16 files read with
``feature_dtype='stored'``.  Every sample is one whole pass over the videos between a device synchronise before and the counter's
``metrics()`` (a host read, so a synchronise) after, on a host clock; the routes alternate, after one warm-up pass each, and the three
tables are compared before anything is reported.

    python tools/eval_device_time.py [--out FILE] [--videos 16] [--T 16384] [--nq 4] [--repeats 7]"""
import argparse
import atexit
import importlib
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module('cvpr2025-decafnet_amd')

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=None, help='also append the printed lines to this file, as they come')
ap.add_argument('--videos', type=int, default=16)
ap.add_argument('--T', type=int, default=16384)
ap.add_argument('--nq', type=int, default=4)
ap.add_argument('--repeats', type=int, default=7)
ap.add_argument('--tiny', action='store_true', help='a small model instead of the BASELINE config 3 one (a rehearsal of the script)')
args = ap.parse_args()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, 'w').close()


def say(s=''):
    print(s, flush=True)
    if args.out:
        with open(args.out, 'a') as f:
            f.write(s + '\n')


# BASELINE.md section 2 probe hyper-parameters (bench.py's), or the tiny model of the tests
KW = dict(D=32, E=32, TE=32, text_in=32, n_levels=3, win=3, n_heads=2, sn=8, sratio=0.5, norm=True, max_seq_len=64, text_layers=2,
          text_max_len=24, text_use_abs_pe=True, n_stem=1, msf=True) if args.tiny else \
     dict(D=1024, E=256, TE=256, text_in=512, n_levels=8, win=9, n_heads=4, sn=60, sratio=0.3, msf=True, norm=True, max_seq_len=2304,
          text_layers=5, text_max_len=48, fusion_layers=2, max_vid_len=args.T)      # (max_vid_len as tools/post_time.py sets it)
FPS, CLIP = 30.0, 16


def write_tree(root):
    """float16 feature files of args.videos videos of args.T clips with args.nq queries each -> the ``opt.data`` dict"""
    g = np.random.default_rng(7)
    D, Ct = KW['D'], KW['text_in']
    for d in ('vid', 'shallow', 'text'):
        os.makedirs(os.path.join(root, d))
    anno, cls = {}, {}
    duration = ((args.T - 1) * CLIP + CLIP) / FPS
    for k in range(args.videos):
        vid = f'v{k}'
        for d in ('vid', 'shallow'):
            np.save(os.path.join(root, d, vid + '.npy'), g.standard_normal((args.T, D), dtype=np.float32).astype(np.float16))
        qs = []
        for q in range(args.nq):
            a = float(g.uniform(0.05, 0.7) * duration)
            sent = f'query {q} of {vid}'
            qs.append({'segment': [a, float(min(a + g.uniform(0.02, 0.25) * duration, duration))], 'sentence': sent, 'sentence_id': f'{vid}_q{q}'})
            np.save(os.path.join(root, 'text', f'{vid}_q{q}.npy'), g.standard_normal((int(g.integers(6, 24)), Ct)).astype(np.float32))
            cls[sent] = g.standard_normal((1, D)).astype(np.float32)
        anno[vid] = {'fps': FPS, 'num_frames': int((args.T - 1) * CLIP + CLIP), 'num_clips': args.T, 'annotations': qs}
    with open(os.path.join(root, 'anno.json'), 'w') as fh:
        json.dump({'val': anno}, fh)
    np.save(os.path.join(root, 'cls_val.npy'), cls, allow_pickle=True)
    return dict(anno_file=os.path.join(root, 'anno.json'), eval_split=('val',), vid_feat_dir=[os.path.join(root, 'vid')],
                shallow_vid_feat_dir=[os.path.join(root, 'shallow')], text_feat_dir=os.path.join(root, 'text'),
                text_cls_fname=os.path.join(root, 'cls_{split}.npy'), vid_load='npy', shallow_vid_load='npy', downsample_rate=1,
                clip_size=CLIP, clip_stride=CLIP, feature_dtype='stored')


root = tempfile.mkdtemp(prefix='dcf_eval_time_')
atexit.register(shutil.rmtree, root, ignore_errors=True)
t0 = time.perf_counter()
ed = pkg.data.VideoCentricEvalData(write_tree(root))
host_samples = list(ed)                                                       # the host cache: every file is read once, here
say(f'## {len(host_samples)} videos of {args.T} clips, D = {KW["D"]}, {args.nq} queries each, float16 files; tree written and read in '
    f'{time.perf_counter() - t0:.1f} s')
assert torch.cuda.is_available(), 'needs the GPU: there is nothing to time without it'

opt = pkg.config.make_opt(**KW)
model = pkg.modeling.create_model(opt)
model.load_state_dict(pkg.synth.make_state_dict({k: list(v.shape) for k, v in model.state_dict().items()}, 2025))
model = model.cuda().eval().requires_grad_(False)
E = pkg.evaluator
ev = E.GroundingEvaluator(opt, model)
t0 = time.perf_counter()
bank = pkg.data.EvalBank(ed, vid_stride=ev.vid_stride)
torch.cuda.synchronize()
say(f'bank: {bank.nbytes / 1e6:.0f} MB, filled in {time.perf_counter() - t0:.1f} s')
ranks, threshs = opt['eval']['ranks'], opt['eval']['iou_threshs']
ROUTES = {'host': (host_samples, lambda: E.RecallCounter(ranks, threshs)), 'bank': (bank, lambda: E.RecallCounter(ranks, threshs)),
          'device': (bank, lambda: E.DeviceRecallCounter(ranks, threshs))}


def one_pass(route):
    dataset, make = ROUTES[route]
    counter = make()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev.run(dataset, counter=counter)
    m = counter.metrics()                                                     # the device counter's one read; a no-op wait on the others
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / len(host_samples), m, counter.n_queries


tables = {r: one_pass(r)[1:] for r in ROUTES}                                 # warm-up, and the three routes count the same
assert all(np.array_equal(tables[r][0], tables['host'][0]) and tables[r][1] == args.videos * args.nq for r in ROUTES), tables
times = {r: [] for r in ROUTES}
for _ in range(args.repeats):
    for r in ROUTES:
        times[r].append(one_pass(r)[0])
say(f'per video, {args.repeats} passes per route, alternating, after one warm-up pass each (n_streams = 1); metrics equal on all routes: '
    f'{(tables["host"][0] * 100).round(2).tolist()}')
for r, v in times.items():
    v = sorted(v)
    med = v[len(v) // 2]
    say(f'{r:7s} {med:8.3f} ms per video (min {v[0]:.3f}, max {v[-1]:.3f}) = {args.T / med / 1e3:6.2f} M clips/s')
