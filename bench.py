#!/usr/bin/env python3
"""Throughput of the DeCafNet grounding forward on MI355X (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--nq NQ] [--T 16384]
    python bench.py --gpus N ...                      # no WORLD_SIZE set: starts its own N ranks (one per GPU, RCCL)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...
    ... bench.py --gpus N --shard-T 65536        # BASELINE configs[3]: ONE long video sharded over the N ranks (RCCL)

Default workload = BASELINE.json configs[2] with the survey's probe hyper-parameters: a "step" is
one pass of the eval forward of PtTransformerEarlyFusionIterative over a batch of synthetic videos of T = 16384 clips
(D = 1024), NQ text queries each, inputs already resident in HBM, timed from model.forward entry to logits / offsets /
masks on the device.  With N > 1 every rank runs its own replica -- the path shards over independent
(video, query) units with no data-path collective (weak scaling); value = all clips of all ranks divided by the slowest
rank's time.  With --shard-T one video of that length is cut into N clip chunks (+ halo), two RCCL all-gathers per
forward (cvpr2025-decafnet_amd/dist.py), strong scaling; rank 0 checks the result against the unsharded forward.

Rank 0 prints ONE JSON line: the driver contract fields (metric, value, unit, higher_is_better, dtype, ms_per_step = wall time of
one timed step: exactly --steps steps are timed unless --min-timed-s asks for repeated blocks).  A plain run sets up, warms up,
times the steps and prints that line; --full adds, after the timed steps (rank 0 of the replica mode)
  roofline     : dominant kernel family (dense-conv GEMM), live HIP-event timing of every launch
  parity       : max |delta| of logits / offsets of one timed video against the CPU oracle (the checker)
  cpu_baseline : the CPU oracle (a port of the reference algorithm) timed on this host's cores (N = 1 only)
  stages       : per-kernel-family time of one step (same event timing)
  post         : proposal decode + NMS latency and the NMS index match against the oracle
  xattn_config2, mfma_sustained, nq8, one_forward_in_flight, one_video_per_call : the other configurations, each timed on its own
--dump-outputs DIR writes what the last timed step returned to its caller (logits / offsets / masks of every video, float32 .npy;
see dump_outputs); weights and inputs are seeded, so the same arguments give the same inputs on every run.
"""
import argparse
import ctypes
import hashlib
import importlib
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_F32_MFMA_TFLOPS = 157.3     # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 dense peak
PEAK_BF16_MFMA_TFLOPS = 2500.0   # MI355X_MICROARCH.md: bf16 / fp16 dense MFMA peak
PEAK_HBM_GBS = 8000.0            # HBM3E spec


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--nq', type=int, default=1, help='text queries per video')
    ap.add_argument('--T', type=int, default=16384)
    ap.add_argument('--vid-len', type=int, default=0, help='valid clips (default: T)')
    ap.add_argument('--max-batch', type=int, default=8)
    ap.add_argument('--videos', type=int, default=3,
                    help='videos per step: independent videos in flight on their own HIP streams (one model instance each)')
    ap.add_argument('--batch', type=int, default=8,
                    help='videos per forward (forward_videos: same-length videos batched through every kernel); a step then '
                         'holds --videos x --batch videos')
    ap.add_argument('--shard-T', type=int, default=0,
                    help='BASELINE configs[3]: one video of this many clips, clip-chunk sharded over the ranks (0 = replicas)')
    ap.add_argument('--min-timed-s', type=float, default=0.0,
                    help='repeat the timed block of --steps steps (each block barrier + synchronise bracketed) until this much time is covered '
                         '(default 0: one block, exactly --steps timed steps)')
    ap.add_argument('--full', action='store_true',
                    help='after the timed steps also measure / check everything else: per-kernel roofline and stages, parity against the '
                         'CPU oracle, CPU baseline, proposal decode + NMS, the other configurations (off: the headline figure only)')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='write the outputs of the last timed step as DIR/<name>.npy (float32, at most 64 MB in all)')
    ap.add_argument('--attn-mode', default='f16x3', choices=['f16x3', 'f16'],
                    help="attention products on the matrix cores: f16x3 (fp32 accurate, default) or f16 (one fp16 product: BASELINE configs[4]'s "
                         "'bf16 MFMA attention'; opt-in, the line's `parity` is its delta against the fp32 oracle)")
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--debug-gloo-one-gpu', action='store_true',
                    help='flow check of the multi-rank path on a one-GPU box: gloo rendezvous, every rank on cuda:0 (timings meaningless)')
    ap.add_argument('--no-post', action='store_true')
    ap.add_argument('--no-hybrid', action='store_true', help='--shard-T: clip chunks as recompute windows only (no pyramid cut)')
    ap.add_argument('--cpu-T', type=int, default=0, help='T of the CPU-baseline sample (default: same T)')
    return ap.parse_args()


def one_video_dispatches():
    """kernel dispatches of one one-video forward (the reference's calling pattern) from the committed rocprofv3 timeline of the
    same kernel sources (profiles/r*_dispatches.json, tools/run_trace.sh); None when the sources changed since"""
    import glob
    for c in sorted(glob.glob(os.path.join(ROOT, 'profiles', 'r*_dispatches.json')), reverse=True):
        try:
            with open(c) as fh:
                j = json.load(fh)
        except (OSError, ValueError):
            continue
        if j.get('csrc_sha16') == csrc_hash():
            return j.get('one_video_dispatches')
    return None


def probe_kwargs(T):
    # BASELINE.md section 2 probe hyper-parameters; the position encoding (max_seq_len 2304) is resampled to T (video_net.py:147-150)
    return dict(D=1024, E=256, TE=256, text_in=512, n_levels=8, win=9, n_heads=4, sn=60, sratio=0.3, msf=True,
                norm=True, max_seq_len=2304, text_layers=5, text_max_len=48, fusion_layers=2)


def csrc_hash():
    """sha256 over the kernel sources and the C ABI header: profiles/ artefacts that depend on the build carry it"""
    h = hashlib.sha256()
    d = os.path.join(ROOT, 'cvpr2025-decafnet_amd', 'csrc')
    for f in sorted(os.listdir(d)) + ['../../include/decafnet_hip.h']:
        with open(os.path.join(d, f), 'rb') as fh:
            h.update(f.encode() + b'\0' + fh.read())
    return h.hexdigest()[:16]


def cpu_model():
    try:
        for line in subprocess.run(['lscpu'], capture_output=True, text=True, timeout=10).stdout.splitlines():
            if line.startswith('Model name'):
                return line.split(':', 1)[1].strip()
    except Exception:
        pass
    return 'unknown'


def physical_cores():
    try:
        out = subprocess.run(['lscpu', '-p=core,socket'], capture_output=True, text=True, timeout=10).stdout
        cores = {l for l in out.splitlines() if l and not l.startswith('#')}
        avail = len(os.sched_getaffinity(0))
        return max(1, min(len(cores), avail))
    except Exception:
        return max(1, len(os.sched_getaffinity(0)))


def max_deltas(got, want, nq, L):
    dl = max(float((got[0][q][l].float().cpu() - want[0][q][l]).abs().max()) for q in range(nq) for l in range(L))
    do = max(float((got[1][q][l].float().cpu() - want[1][q][l]).abs().max()) for q in range(nq) for l in range(L))
    mk = all(bool(torch.equal(got[2][q][l].cpu(), want[2][q][l])) for q in range(nq) for l in range(L))
    return dl, do, mk


DUMP_BUDGET_BYTES = 64 << 20


def dump_outputs(path, videos):
    """--dump-outputs: what the timed path handed its caller in the last timed step.  ``videos``: per video of the step, what
    forward(..., eval=True) returns for it (logits, offsets, masks: per query, per level (1, n_l[, 2])).  Written as
    logits (V, NQ, S), offsets (V, NQ, S, 2) and masks (V, NQ, S), float32, the levels concatenated along the point axis S.
    Above 64 MB in all, the same fixed, seeded sample of the points is kept in every array and its indices go to points.npy."""
    import numpy as np

    def flat(part):
        return torch.stack([torch.cat([x.reshape((-1,) + tuple(x.shape[2:])) for x in lv]) for lv in part]).float().cpu().numpy()

    arrs = {name: np.stack([flat(v[i]) for v in videos]) for i, name in enumerate(('logits', 'offsets', 'masks'))}
    S = arrs['logits'].shape[2]
    total = sum(a.nbytes for a in arrs.values())
    if total > DUMP_BUDGET_BYTES:
        keep = DUMP_BUDGET_BYTES // (total // S + 8)
        idx = np.sort(np.random.default_rng(0).choice(S, keep, replace=False))
        arrs = {k: np.ascontiguousarray(a[:, :, idx]) for k, a in arrs.items()}
        arrs['points'] = idx.astype(np.float64)
    os.makedirs(path, exist_ok=True)
    for k, a in arrs.items():
        np.save(os.path.join(path, k + '.npy'), a)
    return {'files': sorted(k + '.npy' for k in arrs), 'videos': len(videos), 'points': S, 'sampled_points': len(idx) if 'points' in arrs else None}


class Marks:
    """HIP-event marks on the current stream between the phases of dist.sharded_forward"""

    def __init__(self):
        self.rows = []
        self.cur = None

    def begin(self):
        self.cur = []

    def mark(self, name):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.cur.append((name, e))

    def end(self):
        self.rows.append(self.cur)

    def summary(self):
        acc = {}
        for row in self.rows:
            for (n0, e0), (_, e1) in zip(row, row[1:]):
                acc.setdefault(n0, []).append(e0.elapsed_time(e1) * 1e3)
        return {k: sum(v) / len(v) for k, v in acc.items()}


def run_sharded(args, pkg, dist, rank, world, dev):
    """BASELINE configs[3]: one long video, clip-chunk sharded over the ranks; two RCCL all-gathers per forward."""
    T, nq = args.shard_T, args.nq
    vid_len = args.vid_len or T
    kw = probe_kwargs(T)
    opt = pkg.config.make_opt(**kw)
    opt.model['max_batch'] = args.max_batch
    model = pkg.modeling.create_model(opt)
    sd = pkg.synth.make_state_dict({k: list(v.shape) for k, v in model.state_dict().items()}, 2025)
    model.load_state_dict(sd)
    model = model.to(dev).eval().requires_grad_(False)
    inp = pkg.synth.make_inputs(kw['D'], T, vid_len, nq, kw['text_in'], 32, 2025 + 4)      # the same video on every rank
    texts, tmasks = zip(*[model.encode_text(tok[None].to(dev), torch.ones(1, 1, tok.size(-1), dtype=torch.bool, device=dev))
                          for tok in inp['tokens']])
    d = pkg.dist
    L, win = kw['n_levels'], kw['win']
    arch = d.arch_of(model)                           # layer counts of THIS model: the halos are functions of them
    halo = d.receptive_field(L, win, **arch)
    # queries first, clips second (dist.shard_plan_2d): with NQ = 1 this is the pure T-shard of BASELINE configs[3]
    # ... and the clip axis itself with the pyramid cut at a level k where that computes fewer rows (dist.hybrid_plan; --no-hybrid: windows only)
    harch = None if args.no_hybrid else arch
    grid = d.shard_plan_2d(T, world, nq, L, win, halo, hybrid_arch=harch)
    hyb = grid.get('hybrid')
    groups = d.make_grid_groups(grid['t_shards'], grid['q_groups']) if dist is not None else None
    plan = grid['plan']
    lo, hi, w_lo, w_hi = plan[rank % grid['t_shards']]
    vid_w = inp['vid'][0][:, w_lo:w_hi].contiguous().to(dev)
    sh_w = inp['shallow_vid'][0][:, w_lo:w_hi].contiguous().to(dev)
    mask_full = inp['vid_masks'][0].to(dev)
    cls = inp['text_cls'].to(dev)
    be = d.HipBackend(model)
    marks = Marks()

    def step(timed=False):
        if timed:
            marks.begin()
        out = d.sharded_forward_2d(be, vid_w, sh_w, mask_full, grid, groups, rank, T, L, texts, cls, tmasks, timings=marks if timed else None)
        if timed:
            marks.end()
        return out

    for _ in range(3 + args.warmup):
        step()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = step()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        tt = torch.tensor([elapsed], device='cpu' if args.debug_gloo_one_gpu else dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    assert model.numerics_status() & 1 == 0, 'f16x3 GEMM range overflow flagged'
    dumped = dump_outputs(args.dump_outputs, [out]) if args.dump_outputs and rank == 0 else None
    for _ in range(min(args.steps, 5)):
        step(timed=True)
    torch.cuda.synchronize()
    phases = marks.summary()
    result = {
        'metric': 'clips/sec (grounding fwd, T=16384 D=1024)', 'value': vid_len * nq * args.steps / elapsed, 'unit': 'clips/s',
        'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': 1e3 * elapsed / args.steps,
        'higher_is_better': True, 'scaling': 'strong', 'vs_baseline': None, 'dtype': 'f32', 'data': 'synthetic',
        'config': {'workload': f'BASELINE configs[3]: ONE video of T={T} clips (D=1024, probe hyper-parameters, NQ={nq}) over {world} rank(s) as '
                               f'{grid["q_groups"]} query group(s) x {grid["t_shards"]} clip chunk(s): ' +
                               (f'pyramid cut at level {hyb["k"]} (levels <= k on a narrow window, levels above on a coarse window of the all-gathered '
                                f'level-k features: AG-F, AG-R), ' if hyb else f'owned chunk + {halo}-clip recompute halo per side, ') +
                               'RCCL all-gather of the sidekick scores (AG-1) and of the packed per-level outputs (AG-2) inside a clip-chunk group, '
                               'one more of the full-length outputs across the query groups (AG-3)',
                   'T': T, 'vid_len': vid_len, 'nq': nq, 'window_clips_rank0': plan[0][3] - plan[0][2], 'window_clips_max': max(p[3] - p[2] for p in plan),
                   'owned_clips': plan[0][1] - plan[0][0], 'halo': halo, 'parallelism': f'query groups x{grid["q_groups"]}, T-shard x{grid["t_shards"]}',
                   'rows_per_rank_over_even_share': grid['rows_factor'], 'split_level': hyb['k'] if hyb else None,
                   'backend': 'gloo (flow check)' if args.debug_gloo_one_gpu else ('nccl = RCCL' if world > 1 else 'single rank')},
        'phases_us_rank0': phases,
        'collectives_us_rank0': {'ag1_scores': phases.get('ag1'), 'ag2_outputs': phases.get('ag2'), 'ag3_query_groups': phases.get('ag3'),
                                 'agF_level_k_features': phases.get('agF'), 'agR_refined_map': phases.get('agR')},
    }
    # the sharded result against the unsharded forward of the same video on rank 0
    if rank == 0:
        full = model(inp['vid'].to(dev), inp['shallow_vid'].to(dev), inp['vid_masks'].to(dev), texts, cls, tmasks, eval=True)
        dl, do, mk = max_deltas(out, [[[x.cpu() for x in lv] for lv in part] for part in full], nq, L)
        result['parity'] = {'against': 'unsharded forward of the same video on rank 0 (itself checked against the CPU oracle by '
                                       'tests/test_gpu_e2e.py::test_config4_unsharded_T65536_vs_oracle)',
                            'max_abs_logit': dl, 'max_abs_offset': do, 'masks_equal': mk}
        assert mk and dl < 2e-4 and do < 2e-4, f'sharded forward differs from the unsharded one: {dl} {do} {mk}'
        if dumped:
            result['dump_outputs'] = dumped
        print(json.dumps(result), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def spawn_ranks(args):
    """`python bench.py --gpus N` with no WORLD_SIZE in the environment: the parent starts N fresh child processes (one per
    GPU, RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set -- what torch.distributed.run would set), relays their output and
    exits with the worst child's return code.  The parent has touched no GPU at this point (importing torch does not
    initialise HIP), and it never exec()s: the children are ordinary subprocesses (train.py:42-46 is the reference's launch)."""
    import socket
    import threading

    def start():
        # a free rendezvous port on the loopback interface.  The probe socket is closed before rank 0 binds the port (seconds later, once it
        # has imported torch), so another process can take it in between: a run whose ranks die at the rendezvous is started once more
        # on a fresh port (below) instead of failing the bench.
        with socket.socket() as s:
            s.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
            s.bind(('127.0.0.1', 0))
            port = s.getsockname()[1]
        env0 = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), WORLD_SIZE=str(args.gpus),
                    LOCAL_WORLD_SIZE=str(args.gpus), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY', '0'))
        procs = []
        for r in range(args.gpus):
            env = dict(env0, RANK=str(r), LOCAL_RANK=str(r))
            # rank 0 prints the ONE JSON line on stdout; whatever another rank prints goes to stderr, not away
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                          stdout=subprocess.PIPE if r == 0 else sys.stderr, stderr=None))
        chunks = []
        reader = threading.Thread(target=lambda: chunks.append(procs[0].stdout.read()), daemon=True)
        reader.start()
        return procs, chunks, reader, time.time()

    procs, chunks, reader, t_start = start()
    retried = False
    failed_at = None
    while any(p.poll() is None for p in procs):          # a rank that dies leaves the others at a barrier: end them after a grace period
        if failed_at is None and any(p.poll() not in (None, 0) for p in procs):
            failed_at = time.time()
            if not retried and failed_at - t_start < 30:   # died before or at the rendezvous (the port was taken?): one fresh start
                for p in procs:
                    if p.poll() is None:
                        p.kill()
                for p in procs:
                    p.wait()
                sys.stderr.write('bench.py: a rank exited %.0f s after its start; starting the ranks once more on a new port\n' % (failed_at - t_start))
                procs, chunks, reader, t_start = start()
                retried, failed_at = True, None
                continue
        if failed_at is not None and time.time() - failed_at > 60:
            for p in procs:
                if p.poll() is None:
                    p.kill()
        time.sleep(0.2)
    reader.join(timeout=10)
    sys.stdout.write(b''.join(chunks).decode(errors='replace'))
    sys.stdout.flush()
    worst = 0
    for p in procs:
        rc = p.returncode
        if rc != 0 and (worst == 0 or abs(rc) > abs(worst)):
            worst = rc
    sys.exit(worst if worst >= 0 else 128 - worst)


def main():
    args = parse()
    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        return spawn_ranks(args)                         # before any GPU call in this process
    rank = int(os.environ.get('RANK', 0))
    world = int(os.environ.get('WORLD_SIZE', 1))
    local_rank = int(os.environ.get('LOCAL_RANK', 0))
    if args.gpus != world:
        sys.stderr.write(f'bench.py: --gpus {args.gpus} but WORLD_SIZE is {world}.  One process per GPU: either plain\n'
                         f'  python bench.py --gpus {args.gpus} ...          (starts its own {args.gpus} ranks), or\n'
                         f'  python -m torch.distributed.run --nnodes=1 --nproc-per-node {args.gpus} --master-addr 127.0.0.1 '
                         f'--master-port 29511 bench.py --gpus {args.gpus} ...\n')
        sys.exit(2)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29511')
        if args.debug_gloo_one_gpu:
            dist.init_process_group('gloo')
            local_rank = 0
        else:                                            # before any other GPU call
            dist.init_process_group('nccl', device_id=torch.device('cuda', local_rank))
    assert torch.cuda.is_available(), 'bench.py needs an MI355X'
    torch.cuda.set_device(local_rank)
    dev = torch.device('cuda', local_rank)
    pkg = importlib.import_module('cvpr2025-decafnet_amd')
    lib = pkg._lib.lib()
    if args.shard_T:
        return run_sharded(args, pkg, dist, rank, world, dev)

    T = args.T
    vid_len = args.vid_len or T
    kw = probe_kwargs(T)
    opt = pkg.config.make_opt(**kw)
    opt.model['max_batch'] = args.max_batch
    opt.model['attn_mode'] = args.attn_mode
    model = pkg.modeling.create_model(opt)
    shapes = {k: list(v.shape) for k, v in model.state_dict().items()}
    sd = pkg.synth.make_state_dict(shapes, 2025)
    model.load_state_dict(sd)
    model = model.to(dev).eval().requires_grad_(False)
    model.reuse_output_buffers = True      # static output buffers: the repeated forward replays one captured HIP graph
    inp = pkg.synth.make_inputs(kw['D'], T, vid_len, args.nq, kw['text_in'], 32, 2025 + 3 + rank)
    vid, shallow, vmask = inp['vid'].to(dev), inp['shallow_vid'].to(dev), inp['vid_masks'].to(dev)
    text_cls = inp['text_cls'].to(dev)
    texts, tmasks = [], []
    for tok in inp['tokens']:
        t, m = model.encode_text(tok[None].to(dev), torch.ones(1, 1, tok.size(-1), dtype=torch.bool, device=dev))
        texts.append(t)
        tmasks.append(m)
    texts, tmasks = tuple(texts), tuple(tmasks)

    def lane_inputs(mdl, seed0):
        """the --batch - 1 further videos of a lane (its first video is given): argument tuples of forward"""
        extra = []
        for j in range(1, max(1, args.batch)):
            ij = pkg.synth.make_inputs(kw['D'], T, vid_len, args.nq, kw['text_in'], 32, seed0 + 100000 * j)
            tj, mj = zip(*[mdl.encode_text(tok[None].to(dev), torch.ones(1, 1, tok.size(-1), dtype=torch.bool, device=dev))
                           for tok in ij['tokens']])
            extra.append((ij['vid'].to(dev), ij['shallow_vid'].to(dev), ij['vid_masks'].to(dev), tuple(tj), ij['text_cls'].to(dev), tuple(mj)))
        return extra

    first = (vid, shallow, vmask, texts, text_cls, tmasks)
    batch0 = [first] + lane_inputs(model, 2025 + 3 + rank)

    def step1():
        """one forward on the current stream; returns, per video of the forward, what forward(..., eval=True) returns"""
        if args.batch > 1:
            return model.forward_videos(batch0)
        return [model(vid, shallow, vmask, texts, text_cls, tmasks, eval=True)]

    # A step = one batch of `--videos` x `--batch` different synthetic videos: `--videos` independent forwards (own model
    # instance = own workspace + HIP graph) on their own streams, each carrying `--batch` videos.
    others = []
    for k in range(1, max(1, args.videos)):
        mk = model.replica()                        # same parameters, own engine / workspace / graph
        mk.reuse_output_buffers = True
        ik = pkg.synth.make_inputs(kw['D'], T, vid_len, args.nq, kw['text_in'], 32, 2025 + 3 + rank + 1000 * k)
        tk, mkk = zip(*[mk.encode_text(tok[None].to(dev), torch.ones(1, 1, tok.size(-1), dtype=torch.bool, device=dev))
                        for tok in ik['tokens']])
        ak = (ik['vid'].to(dev), ik['shallow_vid'].to(dev), ik['vid_masks'].to(dev), tuple(tk), ik['text_cls'].to(dev), tuple(mkk))
        others.append((mk, ak, torch.cuda.Stream(), [ak] + lane_inputs(mk, 2025 + 3 + rank + 1000 * k)))
    stream0 = torch.cuda.Stream() if others else None
    torch.cuda.synchronize()

    def step():
        """one step; returns the outputs of every video of the step, forward by forward (step1's structure)"""
        if not others:
            return step1()
        with torch.cuda.stream(stream0):
            outs = step1()
        for mk, a, sk, bk in others:
            with torch.cuda.stream(sk):
                if args.batch > 1:
                    outs += mk.forward_videos(bk)
                else:
                    outs.append(mk(*a, eval=True))
        return outs

    # setup, not steps: the engine runs a new argument set eagerly once, captures its HIP graph on the second call and
    # replays from the third; a few more replays let the allocator and the clocks settle whatever --warmup is
    for _ in range(6):
        step()
    torch.cuda.synchronize()
    launch_modes = sorted({m_.graph_active() for m_ in [model] + [o[0] for o in others]})
    for _ in range(args.warmup):
        step()
    # Timed region: blocks of EXACTLY --steps steps, each bracketed by barrier + synchronise on both sides and reduced with
    # MAX over the ranks.  One block of the default K is ~0.25 s; blocks are repeated until --min-timed-s is covered (every
    # rank runs the same number: the decision is taken on the reduced time) and `value` is the mean over the blocks, with
    # every block's time in `block_ms`.
    def timed_block():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            o = step()
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dist is not None:
            tt = torch.tensor([dt], device='cpu' if args.debug_gloo_one_gpu else dev, dtype=torch.float64)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            dt = float(tt.item())
        return dt, o

    blocks = []
    while True:
        dt, out = timed_block()
        blocks.append(dt)
        if sum(blocks) >= args.min_timed_s or len(blocks) >= 64:
            break
    elapsed = sum(blocks) / len(blocks)                  # seconds per block of --steps steps
    # the f16x3 GEMMs flag any accumulator that left the finite range (operands beyond the fp16 range): must be clean
    for mk in [model] + [o[0] for o in others]:
        assert mk.numerics_status() & 1 == 0, 'f16x3 GEMM range overflow flagged: the timed outputs are not valid'
    # outputs of the LAST timed step (rank-local), before anything else runs on the reused output buffers
    dumped = dump_outputs(args.dump_outputs, out) if args.dump_outputs and rank == 0 else None
    timed_out = [[[x.clone() for x in lv] for lv in part] for part in out[0]] if args.full else None     # its first video
    n_lanes = 1 + len(others)
    n_videos = n_lanes * max(1, args.batch)
    clips_per_step = n_videos * vid_len * args.nq
    value = world * clips_per_step * args.steps / elapsed
    launch_note = {0: 'eager kernel launches', 1: 'HIP graph replay', 2: 'HIP graph (just captured)'}

    result = {
        'metric': 'clips/sec (grounding fwd, T=16384 D=1024)', 'value': value, 'unit': 'clips/s', 'n_gpus': world,
        'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': 1e3 * elapsed / args.steps,
        'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None, 'dtype': 'f32', 'data': 'synthetic',
        'dtype_note': 'fp32 in, fp32 out, fp32 accumulate; dense convolutions in "f16x3": every fp32 operand carried as two fp16 planes '
                      '(22 significant bits), three v_mfma_f32_32x32x16_f16 products per multiply-add -- error of an fp32 FMA chain',
        'timed_blocks': len(blocks), 'timed_region_s': sum(blocks), 'block_ms': [1e3 * b for b in blocks],
        'config': {'workload': f'BASELINE configs[2]: T={T} D=1024 full multi-scale pyramid + sidekick top-k 30% + expert path, '
                               f'NQ={args.nq} queries/video, {n_videos} independent videos per step: {n_lanes} forwards in flight on {n_lanes} HIP streams x '
                               f'{max(1, args.batch)} videos per forward, one replica of this per GPU',
                   'T': T, 'vid_len': vid_len, 'D': 1024, 'E': 256, 'TE': 256, 'levels': 8, 'win': 9, 'heads': 4,
                   'fusion_layers': 2, 'sn': 60, 'sratio': 0.3, 'msf': True, 'norm': True, 'Lq': 32, 'nq': args.nq,
                   'max_batch': args.max_batch, 'videos_per_step': n_videos, 'forwards_in_flight': n_lanes, 'videos_per_forward': max(1, args.batch), 'parallelism': f'replicas x{world}',
                   'launch': ' / '.join(launch_note[m_] for m_ in launch_modes) + ' (dcf_graph_active after the setup calls; DCF_NO_GRAPH=1 = eager)',
                   'csrc_sha16': csrc_hash(),
                   'attn_mode': args.attn_mode + (' (fp32-accurate operand split)' if args.attn_mode == 'f16x3' else ' (ONE fp16 product per multiply-add in QK^T / PV: opt-in, not fp32 accurate; see parity)'),
                   # what torch.distributed saw: a SCALE run proves from this that RCCL ran with N ranks
                   'dist': ({'world_size': dist.get_world_size(), 'backend': dist.get_backend(),
                             'note': "backend 'nccl' is RCCL on ROCm; replicas only: the barrier and the MAX-reduce of the timing are its collectives"}
                            if dist is not None else {'world_size': 1, 'backend': None})},
    }

    if dumped:
        result['dump_outputs'] = dumped
    if rank == 0 and args.full:
        # ---- live per-kernel timing: the same steps again with every launch bracketed by HIP events
        lib.dcf_profile_enable(1)
        for _ in range(args.steps):
            step1()                                  # one forward on the current stream: undisturbed per-kernel times
        torch.cuda.synchronize()
        need = lib.dcf_profile_report(None, 0)
        buf = ctypes.create_string_buffer(int(need) + 16)
        lib.dcf_profile_report(buf, len(buf))
        lib.dcf_profile_enable(0)
        prof = json.loads(buf.value.decode())
        tot_ms = sum(v['ms'] for v in prof.values())
        stages = {k: {'ms_per_step': v['ms'] / args.steps, 'launches_per_step': v['count'] / args.steps,
                      'share': v['ms'] / tot_ms,
                      'tflops': (v['flops'] / (v['ms'] * 1e-3) / 1e12) if v['ms'] > 0 else 0.0,
                      'alg_GBps': (v['bytes'] / (v['ms'] * 1e-3) / 1e9) if v['ms'] > 0 else 0.0}
                  for k, v in sorted(prof.items(), key=lambda kv: -kv[1]['ms'])}
        # dominant kernel = the dense-conv GEMM family.  f16x3 (default): two fp16 planes per operand, 3 fp16 MFMA products
        # per fp32 multiply-add => fp32-equivalent peak 2500 / 3 TFLOP/s; opt.model.gemm_mode = 'bf16x6': 2500 / 6; 'fp32': native 157.3.
        fam = 'gemm_f16x3' if any(k.startswith('gemm_f16x3') for k in prof) else \
              ('gemm_bf16x6' if any(k.startswith('gemm_bf16x6') for k in prof) else 'gemm_f32')
        gk = [k for k in prof if k.startswith(fam)]
        d = {f: sum(prof[k][f] for k in gk) for f in ('ms', 'flops', 'bytes', 'count')}
        terms = {'gemm_bf16x6': 6, 'gemm_f16x3': 3, 'gemm_f32': 0}[fam]
        peak = PEAK_BF16_MFMA_TFLOPS / terms if terms else PEAK_F32_MFMA_TFLOPS
        ach = d['flops'] / (d['ms'] * 1e-3) / 1e12
        result['roofline'] = {
            'kernel': '%s family (all %d tile/operand instantiations, %.0f%% of the step)' % (fam, len(gk), 100 * d['ms'] / tot_ms),
            'bound': 'mfma', 'achieved': ach, 'peak': peak, 'unit': 'TFLOP/s', 'frac': ach / peak, 'traffic': None,
            'launches': d['count'], 'avg_launch_us': 1e3 * d['ms'] / d['count'],
            'alg_flops_per_launch': d['flops'] / d['count'], 'alg_bytes_per_launch': d['bytes'] / d['count'],
            'peak_note': ('fp16 / bf16 dense MFMA peak 2500 TFLOP/s / %d 16-bit MFMA products per fp32 multiply-add (fp32-accurate operand split)' % terms)
                         if terms else 'native fp32 MFMA dense peak',
            'frac_of_native_f32_mfma_peak': ach / PEAK_F32_MFMA_TFLOPS,
            'non_gemm_share': 1.0 - d['ms'] / tot_ms,
            # engine stages: one profiler scope each (a scope may hold several dispatches: the TCN's layers, the text side ...);
            # dispatches_per_forward below is the rocprofv3 count
            'stages_per_forward': sum(v['count'] for v in prof.values()) / args.steps, 'dispatches_per_forward': None,
            'note': 'HIP events around every launch of this kernel family, same K steps re-run right after the timed region; '
                    'achieved = algorithmic 2*M*N*K flops / event time',
        }
        # HBM-side bytes per launch of this kernel family: rocprofv3 PMC passes cannot run inside this process, so the
        # figure comes from the committed summary of tools/pmc_traffic.sh -- valid only for the SAME kernel sources (hash) and
        # the default workload; null otherwise
        traffic_note = None
        try:
            if (args.T, args.nq, args.batch, args.vid_len) != (16384, 1, 8, 0):
                raise KeyError('non-default workload (the PMC passes ran eight videos per forward, T = 16384, NQ = 1)')
            import glob
            cands = sorted(glob.glob(os.path.join(ROOT, 'profiles', 'r*_pmc_traffic.json')) +
                           glob.glob(os.path.join(ROOT, 'profiles', 'r*_pmc_gemm_traffic.json')), reverse=True)
            summ, path = None, None
            for c in cands:                                      # newest round first
                with open(c) as fh:
                    j_ = json.load(fh)
                if j_.get('csrc_sha16') == csrc_hash():
                    summ, path = j_, os.path.relpath(c, ROOT)
                    break
            if summ is None:
                raise KeyError('no profiles/r*_pmc*_traffic.json was collected on these kernel sources (csrc_sha16 %s)' % csrc_hash())
            pmc = summ.get({6: 'gemm_bf16s', 3: 'gemm_f16x3', 0: 'gemm_f32'}[terms])
            if not pmc:
                raise KeyError('%s holds no entry for this GEMM family' % path)
            result['roofline']['traffic'] = pmc['hbm_bytes_per_launch']
            gbps = pmc['hbm_bytes_per_launch'] / (1e-6 * result['roofline']['avg_launch_us']) / 1e9
            result['roofline']['hbm_view'] = {'achieved': gbps, 'peak': PEAK_HBM_GBS, 'unit': 'GB/s', 'frac': gbps / PEAK_HBM_GBS,
                                              'note': 'HBM-side bytes per launch (PMC) / average launch time of the GEMM family'}
            traffic_note = ('bytes per launch, FETCH_SIZE x2 + WRITE_SIZE from two rocprofv3 --pmc passes (%s, tools/pmc_traffic.sh, same csrc hash)' % path)
            if 'forward' in summ:                                # byte budget of the whole forward, every kernel family
                fw = summ['forward']
                result['roofline']['dispatches_per_forward'] = fw.get('dispatches')
                result['roofline']['dispatches_note'] = 'kernel dispatches of one 8-video forward in the rocprofv3 trace of the PMC pass (%s)' % path
                result['hbm_budget'] = {'bytes_per_forward': fw['hbm_bytes'], 'videos_per_forward': fw['videos'],
                                        'bytes_per_clip': fw['hbm_bytes'] / (fw['videos'] * args.T),
                                        'compulsory_bytes_per_clip': 8219, 'by_kernel': fw['by_kernel'], 'source': path}
        except (OSError, ValueError, KeyError) as e:
            traffic_note = 'traffic is null: %s' % (e.args[0] if e.args else e)
        result['roofline']['traffic_note'] = traffic_note
        result['config']['gemm_mode'] = {6: 'bf16x6 split MFMA (fp32 accurate)', 3: 'f16x3 split MFMA (fp32 accurate)', 0: 'native fp32 MFMA'}[terms]
        xa = prof.get('xattn_core')
        if xa:
            result['xattn_in_forward'] = {'bound': 'hbm', 'achieved': xa['bytes'] / (xa['ms'] * 1e-3) / 1e9, 'peak': PEAK_HBM_GBS,
                                          'unit': 'GB/s', 'frac': xa['bytes'] / (xa['ms'] * 1e-3) / 1e9 / PEAK_HBM_GBS,
                                          'avg_launch_us': 1e3 * xa['ms'] / xa['count']}
        # BASELINE config 2 (T=4096, E=1024, Lk=33 cross-attention core), measured as SURVEY 8d prescribes: 100
        # back-to-back launches over rotating buffers > 512 MB, 8 queries per launch (268 MB of q/ctx traffic)
        extras = not args.no_post and world == 1          # single-GPU run only: the other ranks would wait at the barrier
        if extras:
            sys.path.insert(0, os.path.join(ROOT, 'tools'))
            import xattn_bench
            # run twice, keep the second: the first call works on ~800 MB of freshly hipMalloc'ed buffers and is 20 % slower
            xattn_bench.run(4096, 1024, 16, Lk=33, B=8, reps=100)
            x = xattn_bench.run(4096, 1024, 16, Lk=33, B=8, reps=100)
            result['xattn_config2'] = {'bound': 'hbm', 'achieved': x['cold']['GBps'], 'peak': PEAK_HBM_GBS, 'unit': 'GB/s',
                                       'frac': x['cold']['GBps'] / PEAK_HBM_GBS, 'warm_GBps': x['warm']['GBps'],
                                       'us_per_launch': x['cold']['us'], 'alg_bytes_per_clip': 8 * 1024,
                                       'workload': 'T=4096 E=1024 heads=16 Lk=33, 8 queries/launch, f16x3 split on MFMA 16x16x16 f16'}
        if extras:
            # the matrix rate this device sustains (bare MFMA loops on every CU): what a kernel that never idled its matrix pipes would reach
            import ctypes as _ct
            ncu, ns32, ns16 = _ct.c_int32(0), _ct.c_float(0.), _ct.c_float(0.)
            pkg._lib.check(pkg._lib.lib().dcf_calib_mfma_rate(0, 1 << 15, _ct.byref(ncu), _ct.byref(ns32)))
            pkg._lib.check(pkg._lib.lib().dcf_calib_mfma_rate(1, 1 << 16, _ct.byref(ncu), _ct.byref(ns16)))
            dense = ncu.value * 4 * 2.0 * 32 * 32 * 16 / (ns32.value * 1e-9) / 1e12          # fp16 TFLOP/s, 32x32x16
            result['mfma_sustained'] = {
                'ns_per_mfma_32x32x16': ns32.value, 'ns_per_mfma_16x16x32': ns16.value, 'cus': ncu.value,
                'clock_GHz_under_load': 32.0 / ns32.value, 'dense_f16_tflops': dense, 'f16x3_tflops': dense / 3.0,
                'frac_of_sustained': result['roofline']['achieved'] / (dense / 3.0),
                'note': 'dcf_calib_mfma_rate: bare v_mfma_f32_32x32x16_f16 loops, one wave per SIMD on every CU, right after the timed steps; '
                        'frac_of_sustained = roofline.achieved / (that rate / 3 products); roofline.peak stays the nominal 2500 / 3'}
        result['stages'] = stages
        result['event_ms_per_step'] = tot_ms / args.steps

        # ---- the same video with 8 queries per forward (how Evaluator calls the model: all queries of a video at once)
        if extras and args.nq == 1:
            inp8 = pkg.synth.make_inputs(kw['D'], T, vid_len, 8, kw['text_in'], 32, 2025 + 11)
            cls8 = inp8['text_cls'].to(dev)
            t8, m8 = zip(*[model.encode_text(tok[None].to(dev), torch.ones(1, 1, tok.size(-1), dtype=torch.bool, device=dev))
                           for tok in inp8['tokens']])
            for _ in range(3):
                model(vid, shallow, vmask, t8, cls8, m8, eval=True)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(5):
                model(vid, shallow, vmask, t8, cls8, m8, eval=True)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t1) / 5
            result['nq8'] = {'value': vid_len * 8 / dt, 'unit': 'clips/s', 'ms_per_step': 1e3 * dt, 'launch': launch_note[model.graph_active()],
                             'note': 'one forward over the same video with 8 queries (batched through every kernel), rank 0 only'}

        # ---- the same workload with ONE forward in flight, and the reference's calling pattern: one video per call on
        # torch's default stream (the engine hops off the uncapturable NULL stream, so this replays a graph too)
        if extras:
            for _ in range(3):
                step1()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(args.steps):
                step1()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t1) / args.steps
            result['one_forward_in_flight'] = {'value': max(1, args.batch) * vid_len * args.nq / dt, 'unit': 'clips/s', 'ms_per_forward': 1e3 * dt,
                                               'launch': launch_note[model.graph_active()],
                                               'note': f'a single forward at a time on the default stream, {max(1, args.batch)} video(s) per forward, rank 0 only'}
            for _ in range(4):
                model(vid, shallow, vmask, texts, text_cls, tmasks, eval=True)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(args.steps):
                model(vid, shallow, vmask, texts, text_cls, tmasks, eval=True)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t1) / args.steps
            result['one_video_per_call'] = {'value': vid_len * args.nq / dt, 'unit': 'clips/s', 'ms_per_forward': 1e3 * dt,
                                            'launch': launch_note[model.graph_active()],
                                            'note': 'the reference\'s calling pattern (model.py:496: one video per call), default stream, rank 0 only'}
            # ... with its own roofline: the same forward under the per-launch HIP-event profiler
            lib.dcf_profile_enable(1)
            for _ in range(5):
                model(vid, shallow, vmask, texts, text_cls, tmasks, eval=True)
            torch.cuda.synchronize()
            need = lib.dcf_profile_report(None, 0)
            buf = ctypes.create_string_buffer(int(need) + 16)
            lib.dcf_profile_report(buf, len(buf))
            lib.dcf_profile_enable(0)
            p1 = json.loads(buf.value.decode())
            g1 = [k for k in p1 if k.startswith(fam)]
            d1 = {f: sum(p1[k][f] for k in g1) for f in ('ms', 'flops', 'count')}
            t1_ms = sum(v['ms'] for v in p1.values())
            a1 = d1['flops'] / (d1['ms'] * 1e-3) / 1e12
            result['one_video_per_call']['roofline'] = {
                'kernel': '%s family, one video per forward (%.0f%% of the forward)' % (fam, 100 * d1['ms'] / t1_ms), 'bound': 'mfma',
                'achieved': a1, 'peak': peak, 'unit': 'TFLOP/s', 'frac': a1 / peak, 'stages_per_forward': sum(v['count'] for v in p1.values()) / 5,
                'dispatches_per_forward': one_video_dispatches(),
                'event_ms_per_forward': t1_ms / 5, 'non_gemm_share': 1.0 - d1['ms'] / t1_ms}

        # ---- proposal decode + NMS (reported separately) and the NMS index match
        if extras:
            from oracle import nms_oracle
            model(vid, shallow, vmask, texts, text_cls, tmasks, eval=True)      # _last_flat of the first video
            fl, fo, fm = model._last_flat
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            reps = 5
            for _ in range(reps):
                segs, scores, counts = pkg.nms.collect_segments(fl, fo, fm, T, 8)
            torch.cuda.synchronize()
            t_collect = (time.perf_counter() - t1) / reps
            n = int(counts[0])
            s_d, c_d = segs[:1, :n].contiguous(), scores[:1, :n].contiguous()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(reps):
                keep, kc = pkg.nms.nms_device(s_d, c_d, None, n, n, 0.5)
            torch.cuda.synchronize()
            t_nms = (time.perf_counter() - t1) / reps
            t1 = time.perf_counter()
            for _ in range(reps):
                dets, inds, oc = pkg.nms.softnms_device(s_d, c_d, None, n, n, 0.1, 0.9, 0.001, 2)
            torch.cuda.synchronize()
            t_soft = (time.perf_counter() - t1) / reps
            s_cpu, c_cpu = s_d[0].cpu(), c_d[0].cpu()
            ref_keep = nms_oracle.nms(s_cpu, c_cpu, 0.5)
            d2 = torch.zeros(n, 3)
            ref_soft = nms_oracle.softnms(s_cpu, c_cpu, d2, 0.1, 0.9, 0.001, 2)
            t1 = time.perf_counter()
            nms_oracle.nms(s_cpu, c_cpu, 0.5)
            t_cpu_nms = time.perf_counter() - t1
            # forward + decode + the Evaluator's default NMS (soft-NMS, 5 segments kept, voting) for one video, end to end
            opt.model['max_vid_len'] = T                 # the harness pads to max_vid_len (a multiple of the chunk size, worker_v2.py:778)
            ev = pkg.evaluator.GroundingEvaluator(opt, model)
            meta = dict(fps=30.0, clip_stride=16, clip_size=32, duration=1e9)
            for _ in range(3):                                                  # warm-up: allocator, first-call setup
                model(vid, shallow, vmask, texts, text_cls, tmasks, eval=True)
                ev.generate_proposals(model._last_flat, T, meta)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(4 * reps):
                model(vid, shallow, vmask, texts, text_cls, tmasks, eval=True)
                ev.generate_proposals(model._last_flat, T, meta)                # ends with the one D2H copy of the kept segments
            torch.cuda.synchronize()
            t_seq = (time.perf_counter() - t1) / (4 * reps)
            # the evaluator's loop (GroundingEvaluator.run): the proposals of video i are waited for after video i + 1 is launched
            t1 = time.perf_counter()
            prev = None
            for _ in range(4 * reps):
                model(vid, shallow, vmask, texts, text_cls, tmasks, eval=True)
                h = ev.launch_proposals(model._last_flat, T, meta)
                if prev is not None:
                    ev.finish_proposals(prev)
                prev = h
            ev.finish_proposals(prev)
            torch.cuda.synchronize()
            t_e2e = (time.perf_counter() - t1) / (4 * reps)
            result['post'] = {
                'candidates': n, 'collect_ms_per_video': 1e3 * t_collect, 'nms_ms': 1e3 * t_nms, 'softnms_full_ms': 1e3 * t_soft,
                'cpu_oracle_nms_ms': 1e3 * t_cpu_nms,
                'nms_index_match': bool(torch.equal(keep[0, :int(kc)].cpu(), ref_keep)),
                'softnms_index_match': bool(torch.equal(inds[0, :int(oc)].cpu(), ref_soft)),
                'softnms_dets_bitwise': bool(torch.equal(dets[0, :int(oc)].cpu(), d2[:len(ref_soft)])),      # (segment, decayed score) of every pick, bit for bit
                'forward_collect_nms': {'value': vid_len * args.nq / t_e2e, 'unit': 'clips/s', 'ms_per_video': 1e3 * t_e2e,
                                        'ms_per_video_unpipelined': 1e3 * t_seq,
                                        'note': 'one video per call: forward + _collect_segments + batched_nms (soft-NMS, max_num_segs 5, voting 0.95) '
                                                '+ D2H of the kept segments, SURVEY 8d; the host waits for the proposals of a video after launching '
                                                'the next one (GroundingEvaluator.run); unpipelined = wait before the next launch'},
            }

        # ---- parity of the TIMED outputs and the CPU baseline: the oracle (port of the reference algorithm) on this host
        if not args.no_cpu_baseline and world == 1:      # rank 0 at N = 1 only
            from oracle import decafnet_ref as R
            texts_cpu, tm_cpu = zip(*[R.encode_text(sd, opt.model, tok[None], torch.ones(1, 1, tok.size(-1), dtype=torch.bool))
                                      for tok in inp['tokens']])

            def oracle_forward(cinp, tc, mc):
                with torch.no_grad():
                    return R.forward_eval(sd, opt.model, cinp['vid'], cinp['shallow_vid'], cinp['vid_masks'], list(tc), cinp['text_cls'], list(mc))

            ncores = physical_cores()
            torch.set_num_threads(ncores)
            want = oracle_forward(inp, texts_cpu, tm_cpu)                           # also the warm-up of the timed runs
            dl, do, mk = max_deltas(timed_out, want, args.nq, 8)
            result['parity'] = {'against': 'CPU oracle (oracle/decafnet_ref.py, fp32) on the first video of the last timed step',
                                'max_abs_logit': dl, 'max_abs_offset': do, 'masks_equal': mk,
                                'max_logit_magnitude': max(float(x.abs().max()) for x in want[0][0]), 'bound': 1e-3}
            assert mk and dl < 1e-3 and do < 1e-3, f'timed outputs differ from the oracle: {dl} {do} {mk}'

            def best_of(n, fn):
                best = 1e30
                for _ in range(n):
                    t1 = time.perf_counter()
                    fn()
                    best = min(best, time.perf_counter() - t1)
                return best

            # thread sweep on the SAME sample (one whole video): MKLDNN convolutions of this size stop scaling long before a
            # 64-core socket is full, so the reported baseline is the best setting, not "all cores"
            sweep = {}
            for nt in sorted({1, 8, 16, 32, 64, ncores}):
                if nt > ncores:
                    continue
                torch.set_num_threads(nt)
                oracle_forward(inp, texts_cpu, tm_cpu)                               # warm-up at this thread count
                s_ = best_of(2, lambda: oracle_forward(inp, texts_cpu, tm_cpu))
                sweep[str(nt)] = {'clips_per_s': vid_len * args.nq / s_, 's': s_}
            best_nt = max(sweep, key=lambda k: sweep[k]['clips_per_s'])
            cpu_s = sweep[best_nt]['s']
            result['cpu_baseline'] = {
                'value': vid_len * args.nq / cpu_s, 'unit': 'clips/s', 'cores': int(best_nt), 'kind': 'port',
                'sample': f'1 video x {args.nq} query, T={T} (the bench video): oracle/decafnet_ref.py forward_eval (torch {torch.__version__} CPU fp32, MKLDNN), '
                          f'per thread count one warm-up then best of 2; value = the fastest setting (torch.set_num_threads({best_nt})), {cpu_s:.2f} s',
                'cpu': cpu_model(), 'physical_cores_available': ncores, 'thread_sweep': sweep,
            }
            result['cpu_baseline']['crosscheck'] = ('build container, 8 threads, T=16384, warm, 11 interleaved repetitions (profiles/r03_cpu_crosscheck.json, '
                                                    'tools/cpu_crosscheck.py): oracle / real reference = 0.96x by the medians, 1.08x by the best runs (shared cores: single '
                                                    'runs spread 1.0 .. 4.0 s, which is where round 2\'s 0.76x from two blocks of three came from); outputs agree to 1.3e-6')
        # the north star's other thresholds, inside the object the driver keeps whole
        chk = {}
        if 'xattn_config2' in result:
            chk['xattn_config2'] = {k: result['xattn_config2'][k] for k in ('frac', 'us_per_launch', 'achieved', 'unit')}
        if 'mfma_sustained' in result:
            chk['mfma_sustained'] = {k: result['mfma_sustained'][k] for k in ('clock_GHz_under_load', 'f16x3_tflops', 'frac_of_sustained')}
        if 'hbm_budget' in result:
            chk['hbm_bytes_per_clip'] = result['hbm_budget']['bytes_per_clip']
        if 'one_video_per_call' in result:
            o1 = result['one_video_per_call']
            chk['one_video_per_call'] = {'ms_per_forward': o1['ms_per_forward'], 'clips_per_s': o1['value'],
                                         'gemm_frac': o1.get('roofline', {}).get('frac'),
                                         'dispatches_per_forward': o1.get('roofline', {}).get('dispatches_per_forward')}
        if 'post' in result:
            chk['nms_index_match'] = result['post']['nms_index_match']
            chk['softnms_index_match'] = result['post']['softnms_index_match']
            chk['softnms_dets_bitwise'] = result['post']['softnms_dets_bitwise']
        if 'parity' in result:
            chk['parity_max_abs_logit'] = result['parity']['max_abs_logit']
            chk['parity_max_abs_offset'] = result['parity']['max_abs_offset']
        if 'cpu_baseline' in result:
            chk['gpu_over_cpu'] = result['value'] / result['cpu_baseline']['value']
        if 'roofline' in result:
            result['roofline']['checks'] = chk
    if rank == 0:
        print(json.dumps(result), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
