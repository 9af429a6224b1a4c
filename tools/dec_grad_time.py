"""Time the operators of csrc/xattn_grad.hip and one whole TransformerDecoder layer forward + backward through
autograd.transformer_decoder at the fusion shape of the bench workload, next to torch-ROCm autograd through the plain
softmax(Q K^T) V formulation of the attention core.

    python tools/dec_grad_time.py [--out profiles/dec_grad_times.json]

The shape comes from bench.py's configuration: 8 videos x 16 384 rows, E = 256, 4 heads, a text of Lk = 33
tokens per video, text dimension TE.  Timed: dcf_op_xattn, dcf_op_xattn_bwd with dQ alone and with all three outputs, dcf_op_adaln,
dcf_op_adaln_bwd, the eager core forward + backward, and the decoder layer forward + backward.  Every figure is 50 calls after 10
warm-up calls between device events, in two rounds that alternate over all timed functions (the two rounds are reported side by
side: their difference is the noise).  `gbs` is the bytes the operator must move (each operand read once, each result written once;
masks and the text not counted) over the time of round 0; `gflops` counts two flops per multiply-add of the Lk x d products (two in
the forward, five in the backward, three with dQ alone).  The measurement runs in a child process under a time limit, so a step that
hangs ends there.  Prints one JSON line."""
import argparse
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARM, CALLS = 10, 50
STEP_LIMIT = 400        # seconds


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


def eager_core(torch, q, k, v, mask, heads):
    """softmax(Q K^T) V of blocks.py:374-389 in eager torch on token-major GPU tensors"""
    B, T, C = q.shape
    d = C // heads
    split = lambda z: z.reshape(B, -1, heads, d).transpose(1, 2)
    s = (split(q) * d ** -0.25) @ (split(k) * d ** -0.25).transpose(2, 3)
    p = torch.softmax(s.masked_fill(~mask[:, None, None, :], float('-inf')), dim=-1)
    return (p @ split(v)).transpose(1, 2).reshape(B, T, C)


def one(B, T, E, heads, Lk, TE):
    import torch
    pkg = importlib.import_module('cvpr2025-decafnet_amd')
    l, L, A = pkg._lib, pkg._lib.lib(), pkg.autograd
    st, P = l.current_stream(), l.ptr
    gen = torch.Generator().manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=gen).cuda()
    q, k, v, do = rnd(B, T, E), rnd(B, Lk, E), rnd(B, Lk, E), rnd(B, T, E) * 1e-3
    kvm = torch.ones(B, Lk, dtype=torch.bool)
    kvm[1::2, Lk - Lk // 4:] = False
    kvm = kvm.cuda()
    o, dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    lens = torch.tensor([T - (T // 4) * (b % 2) for b in range(B)])
    mask = (torch.arange(T)[None] < lens[:, None]).cuda()
    h, dh = rnd(B, T, 2 * E), torch.empty(B, T, 2 * E, device='cuda')
    F4, rows = 4.0, B * T
    pair = 2.0 * rows * Lk * E                                  # flops of one Lk x d product over all heads
    ops = {   # name -> (call, bytes it must move, flops)
        'xattn': (lambda: l.check(L.dcf_op_xattn(P(q), P(k), P(v), P(kvm), P(o), B, T, Lk, E, heads, st)), F4 * 2 * rows * E, 2 * pair),
        'xattn_bwd_dq': (lambda: l.check(L.dcf_op_xattn_bwd(P(q), P(k), P(v), P(kvm), P(do), P(dq), None, None, B, T, Lk, E, heads, st)),
                         F4 * 3 * rows * E, 3 * pair),
        'xattn_bwd': (lambda: l.check(L.dcf_op_xattn_bwd(P(q), P(k), P(v), P(kvm), P(do), P(dq), P(dk), P(dv), B, T, Lk, E, heads, st)),
                      F4 * 3 * rows * E, 5 * pair),
        'adaln': (lambda: l.check(L.dcf_op_adaln(P(q), P(mask), P(h), P(o), rows, E, 1, st)), F4 * 4 * rows * E, 0.0),
        'adaln_bwd': (lambda: l.check(L.dcf_op_adaln_bwd(P(q), P(mask), P(h), P(do), P(dq), P(dh), rows, E, 1, st)), F4 * 6 * rows * E, 0.0),
    }
    qr, kr, vr = (z.clone().requires_grad_(True) for z in (q, k, v))

    def eager():
        torch.autograd.grad(eager_core(torch, qr, kr, vr, kvm, heads), [qr, kr, vr], do)

    torch.manual_seed(1)
    blk = pkg.modeling.TransformerDecoder(E, TE, heads).cuda()
    with torch.no_grad():
        blk.drop_path_ffn.scale.fill_(0.5)
    text = rnd(B, Lk, TE).requires_grad_(True)
    params = list(blk.parameters())

    def layer():
        y, _ = A.transformer_decoder(qr, mask, text, kvm, blk)
        torch.autograd.grad(y, [qr, text] + params, do)

    with torch.no_grad():
        diff = float((A.cross_attention(q, k, v, kvm, heads) - eager_core(torch, q, k, v, kvm, heads)).abs().max())
    r = {'B': B, 'T': T, 'E': E, 'heads': heads, 'Lk': Lk, 'TE': TE, 'core_vs_eager_max_abs_diff': diff}
    for rep in range(2):
        for name, (fn, _, _) in ops.items():
            r[f'{name}_us_{rep}'] = timed(torch, fn)
        r[f'eager_core_fwd_bwd_us_{rep}'] = timed(torch, eager)
        r[f'decoder_fwd_bwd_us_{rep}'] = timed(torch, layer)
    for name, (_, nbytes, flops) in ops.items():
        r[f'{name}_gbs'] = nbytes / r[f'{name}_us_0'] * 1e-3
        if flops:
            r[f'{name}_gflops'] = flops / r[f'{name}_us_0'] * 1e-3
    r['xattn_bwd_over_fwd'] = r['xattn_bwd_us_0'] / r['xattn_us_0']
    print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--one', nargs=6, type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        return one(*args.one)
    import bench
    kw = bench.probe_kwargs(16384)
    cmd = ['timeout', '-k', '10', str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), '--one', '8', '16384', str(kw['E']),
           str(kw['n_heads']), '33', str(kw['TE'])]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:                 # a fault, an abort or the time limit: nothing more is started on the GPU
        sys.stderr.write(p.stdout + p.stderr)
        sys.exit(p.returncode)
    line = p.stdout.strip().splitlines()[-1]
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(json.loads(line), f, indent=1)


if __name__ == '__main__':
    main()
