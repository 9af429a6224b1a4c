"""Time the backward of the sliding-window attention core (csrc/attn_grad.hip) at the encoder shapes of the bench workload, next to
the forward op and to torch-ROCm's own autograd through a banded formulation of the same attention.

    python tools/attn_grad_time.py [--level 3] [--out profiles/attn_grad_times.json]

Shapes come from bench.py's configuration (E, heads, window, T = 16384, 8 videos per step): pyramid level 0 and one upper level
(T >> level).  dQ alone (k_attn_bwd_q), dK + dV (k_attn_bwd_q without its second pass, then k_attn_bwd_kv) and all three; 50 calls
after 10 warm-up calls between device events, ours and torch's alternating.  Each shape runs in a child process of its own under a
time limit, so a step that hangs ends there.  Prints one JSON line per shape."""
import argparse
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARM, CALLS = 10, 50
STEP_LIMIT = 120        # seconds per shape


def timed(torch, fn):
    for _ in range(WARM):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / CALLS * 1e3        # microseconds per call


def banded(torch, q, k, v, mask, heads, window):
    """softmax over the band as torch sees it: K and V unfolded `window` times (what makes it unusable at training sizes)"""
    import torch.nn.functional as F
    B, T, C = q.shape
    d, half = C // heads, window // 2
    sp = lambda z: z.view(B, T, heads, d).permute(0, 2, 1, 3)
    kw = F.pad(sp(k), (0, 0, half, half)).unfold(2, window, 1)             # (B, h, T, d, w)
    vw = F.pad(sp(v), (0, 0, half, half)).unfold(2, window, 1)
    s = torch.einsum('bhtd,bhtdw->bhtw', sp(q) * d ** -0.25, kw * d ** -0.25)
    pos = torch.arange(T, device=q.device)[:, None] + torch.arange(-half, half + 1, device=q.device)[None]
    s = s.masked_fill(~((pos >= 0) & (pos < T)), float('-inf'))
    s = s + (~F.pad(mask, (half, half)).unfold(1, window, 1))[:, None] * -1e4
    p = torch.softmax(s, -1) * mask[:, None, :, None]
    return torch.einsum('bhtw,bhtdw->bhtd', p, vw).permute(0, 2, 1, 3).reshape(B, T, C)


def one(B, T, C, heads, window):
    import torch
    pkg = importlib.import_module('cvpr2025-decafnet_amd')
    l, L = pkg._lib, pkg._lib.lib()
    st = l.current_stream()
    gen = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(B, T, C, generator=gen).cuda() for _ in range(3))
    do = (torch.randn(B, T, C, generator=gen) * 1e-3).cuda()
    lens = torch.tensor([T - (T // 4) * (b % 2) for b in range(B)])
    mask = (torch.arange(T)[None] < lens[:, None]).cuda()
    o, dq, dk, dv = (torch.empty_like(q) for _ in range(4))
    P = l.ptr
    fwd = lambda: l.check(L.dcf_op_local_attn(P(q), P(k), P(v), P(mask), P(o), B, T, C, heads, window, st))
    bwd = lambda a, b_, c: (lambda: l.check(L.dcf_op_local_attn_bwd(P(q), P(k), P(v), P(mask), P(do), P(a), P(b_), P(c), B, T, C, heads, window, st)))
    qr, kr, vr = (z.clone().requires_grad_(True) for z in (q, k, v))

    def t_bwd():
        return torch.autograd.grad(banded(torch, qr, kr, vr, mask, heads, window), (qr, kr, vr), do)

    r = {'B': B, 'T': T, 'C': C, 'heads': heads, 'window': window}
    for rep in range(2):
        r[f'fwd_us_{rep}'] = timed(torch, fwd)
        r[f'dq_us_{rep}'] = timed(torch, bwd(dq, None, None))
        r[f'dkdv_us_{rep}'] = timed(torch, bwd(None, dk, dv))
        r[f'all_us_{rep}'] = timed(torch, bwd(dq, dk, dv))
        r[f'torch_banded_fwd_plus_bwd_us_{rep}'] = timed(torch, t_bwd)
    print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--level', type=int, default=3, help='the upper pyramid level timed next to level 0')
    ap.add_argument('--out', default=None)
    ap.add_argument('--one', nargs=5, type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        return one(*args.one)
    import bench
    kw = bench.probe_kwargs(16384)
    rows = []
    for level in (0, args.level):
        cmd = ['timeout', '-k', '10', str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), '--one', '8', str(16384 >> level), str(kw['E']),
               str(kw['n_heads']), str(kw['win'])]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:                 # a fault, an abort or the time limit: nothing more is started on the GPU
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit(p.returncode)
        line = p.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        rows.append(dict(json.loads(line), level=level))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
