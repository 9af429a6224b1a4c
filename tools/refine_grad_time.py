"""Time the operators of csrc/refine_grad.hip and the whole refinement TCN forward + backward through autograd.tcn.

    python tools/refine_grad_time.py [--out profiles/refine_grad_times.json]

Shapes: B*T0 = 16 384 (B = 1) and 131 072 (B = 8, the bench workload's eight videos of 16 384 rows), L = 8 pyramid levels, 32 channels.
Timed: dcf_op_refine_in / _bwd, dcf_op_tcn_layer / _bwd of the layer of dilation 16 without dropout and with p = 0.5, the backward
with dX alone, and autograd.tcn forward and forward + backward (L layers, p = 0.5).  Every figure is 50 calls after 10 warm-up calls
between device events, in two rounds that alternate over all timed functions (the two rounds are reported side by side: their
difference is the noise).  `gflops` counts two flops per multiply-add of the layer's products (4 096 per row in the forward, 12 288 in
the backward, recomputation included) over the time of round 0.  Each shape runs in a child process under a time limit, so a step
that hangs ends there.  Prints one JSON line."""
import argparse
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARM, CALLS = 10, 50
STEP_LIMIT = 300        # seconds
SHAPES = [(1, 16384, 8), (8, 16384, 8)]
SEED = 0x5DEECE66D1234567


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


def one(B, T0, L):
    import torch
    pkg = importlib.import_module('cvpr2025-decafnet_amd')
    l, lib, A = pkg._lib, pkg._lib.lib(), pkg.autograd
    st, P = l.current_stream(), l.ptr
    gen = torch.Generator().manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=gen).cuda()
    torch.manual_seed(1)
    net = pkg.modeling.TCN(L, 32, 32, L).cuda()
    S = sum(T0 >> i for i in range(L))
    lg = rnd(B, S).requires_grad_(True)
    lens = torch.tensor([T0 - (T0 // 4) * (b % 2) for b in range(B)])
    mask = (torch.arange(T0)[None] < lens[:, None]).cuda()
    x, dy = rnd(B, T0, 32), rnd(B, T0, 32) * 1e-3
    y, dx = torch.empty_like(x), torch.empty_like(x)
    lay, dil, li = net.layers[4], 16, 4
    W = [t.detach().contiguous() for t in (lay.conv_dilated.weight, lay.conv_dilated.bias, lay.conv_1x1.weight, lay.conv_1x1.bias,
                                           lay.norm.weight, lay.norm.bias)]
    G = [torch.empty_like(t) for t in W]
    win, bin_ = net.conv_1x1.weight.detach().reshape(32, L).contiguous(), net.conv_1x1.bias.detach().contiguous()
    dl, dwin, dbin = torch.empty(B, S, device='cuda'), torch.empty_like(win), torch.empty_like(bin_)
    lgd = lg.detach()

    def fwd(p):
        return lambda: l.check(lib.dcf_op_tcn_layer(P(x), P(mask), *(P(t) for t in W), P(y), B, T0, dil, SEED, p, li, 0, st))

    def bwd(p, params=True):
        g = [P(t) if params else None for t in G]
        return lambda: l.check(lib.dcf_op_tcn_layer_bwd(P(x), P(mask), *(P(t) for t in W), P(dy), P(dx), *g, B, T0, dil, SEED, p, li, 0, 0, st))

    ops = {
        'refine_in': lambda: l.check(lib.dcf_op_refine_in(P(lgd), P(mask), P(win), P(bin_), P(y), B, T0, L, st)),
        'refine_in_bwd': lambda: l.check(lib.dcf_op_refine_in_bwd(P(lgd), P(mask), P(win), P(dy), P(dl), P(dwin), P(dbin), B, T0, L, 0, st)),
        'layer': fwd(0.0), 'layer_drop': fwd(0.5), 'layer_bwd': bwd(0.0), 'layer_bwd_drop': bwd(0.5), 'layer_bwd_dx': bwd(0.0, False),
    }
    params = list(net.parameters())
    drop = (SEED, 0.5, 0)

    def tcn_fwd():
        with torch.no_grad():
            A.tcn(lgd, mask, net, drop)

    def tcn_fwd_bwd():
        torch.autograd.grad(A.tcn(lg, mask, net, drop), [lg] + params, dy)

    r = {'B': B, 'T0': T0, 'L': L, 'rows': B * T0}
    for rep in range(2):
        for name, fn in ops.items():
            r[f'{name}_us_{rep}'] = timed(torch, fn)
        r[f'tcn_fwd_us_{rep}'] = timed(torch, tcn_fwd)
        r[f'tcn_fwd_bwd_us_{rep}'] = timed(torch, tcn_fwd_bwd)
    rows = B * T0
    r['layer_gflops'] = 2.0 * 4096 * rows / r['layer_us_0'] * 1e-3
    r['layer_bwd_gflops'] = 2.0 * 12288 * rows / r['layer_bwd_us_0'] * 1e-3
    r['layer_bwd_over_fwd'] = r['layer_bwd_us_0'] / r['layer_us_0']
    print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--one', nargs=3, type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        return one(*args.one)
    results = []
    for shape in SHAPES:
        cmd = ['timeout', '-k', '10', str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), '--one'] + [str(v) for v in shape]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:             # a fault, an abort or the time limit: nothing more is started on the GPU
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit(p.returncode)
        results.append(json.loads(p.stdout.strip().splitlines()[-1]))
    line = json.dumps({'shapes': results})
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(json.loads(line), f, indent=1)


if __name__ == '__main__':
    main()
