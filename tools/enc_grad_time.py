"""Time the operator pairs of csrc/enc_grad.hip and one whole TransformerEncoder block forward + backward through
autograd.transformer_encoder at the encoder shapes of the bench workload, next to the same block written in eager torch-ROCm.

    python tools/enc_grad_time.py [--out profiles/enc_grad_times.json]

Shapes come from bench.py's configuration (E, heads, window; T = 16384, 8 videos per step): pyramid level 0 (stride 1, 8 x 16384
rows) and level 1 (stride 2, 8 x 16384 -> 8192 rows).  Every figure is 50 calls after 10 warm-up calls between device events, in
two rounds that alternate over all timed functions (the two rounds are reported side by side: their difference is the noise).  For
the streaming kernels `gbs` is the bytes the operator must move (each operand read once, each result written once; masks and
parameters not counted) over the time of round 0.  The eager block is the CPU checker's functions run on GPU tensors (conv1d with
groups, max_pool1d, an unfolded band for the attention), forward + backward through torch's autograd.  Each level runs in a child
process of its own under a time limit, so a step that hangs ends there.  Prints one JSON line per level."""
import argparse
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
WARM, CALLS = 10, 50
STEP_LIMIT = 240        # seconds per level


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


def eager_block(torch, blk, x, mask, stride, heads, window):
    """TransformerEncoder.forward (blocks.py:578-591) in eager torch on token-major GPU tensors, parameters from `blk`"""
    import torch.nn.functional as F
    from attn_grad_time import banded
    cm = lambda z: z.transpose(1, 2)
    ln = lambda z, n: F.layer_norm(z, z.shape[-1:], n.weight.reshape(-1), n.bias.reshape(-1), 1e-5)
    lin = lambda z, c: F.linear(z, c.weight.squeeze(-1), c.bias)
    mf = mask[..., None].to(x.dtype)
    x = x * mf
    skip = x
    if stride == 2:
        xc = cm(x)
        fill = xc * cm(mf) + (1 - cm(mf)) * xc.amin(dim=-1, keepdim=True).detach()
        skip = cm(F.max_pool1d(fill, 3, 2, 1) * F.max_pool1d(cm(mf), 3, 2, 1))
    xn = cm(ln(x, blk.ln_attn) * mf)
    a = blk.attn
    q, k, v = (cm(F.conv1d(xn, getattr(a, f'{n}_conv').conv.weight, None, stride, 1, 1, xn.size(1))) for n in 'qkv')
    mo = mask[:, ::stride]
    mof = mo[..., None].to(x.dtype)
    q, k, v = ln(q, a.q_norm), ln(k, a.k_norm), ln(v, a.v_norm)
    h = lin(banded(torch, lin(q, a.attn.query), lin(k, a.attn.key), lin(v, a.attn.value), mo, heads, window), a.attn.proj)
    x = skip * mof + blk.drop_path_attn.scale.reshape(-1) * h
    h = lin(F.gelu(lin(ln(x, blk.ln_ffn), blk.ffn.fc)), blk.ffn.proj) * mof
    return x + blk.drop_path_ffn.scale.reshape(-1) * h


def one(B, T, C, heads, window, stride):
    import torch
    pkg = importlib.import_module('cvpr2025-decafnet_amd')
    l, L, A = pkg._lib, pkg._lib.lib(), pkg.autograd
    st, P = l.current_stream(), l.ptr
    To = T // stride
    gen = torch.Generator().manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=gen).cuda()
    x, w = rnd(B, T, C), rnd(3, C, 3)
    lens = torch.tensor([T - (T // 4) * (b % 2) for b in range(B)])
    mask = (torch.arange(T)[None] < lens[:, None]).cuda()
    mo = mask[:, ::stride].contiguous()
    y3, dy3 = torch.empty(3, B, To, C, device='cuda'), rnd(3, B, To, C) * 1e-3
    dx, dw = torch.empty_like(x), torch.empty_like(w)
    yp, dyp, mop = torch.empty(B, T // 2, C, device='cuda'), rnd(B, T // 2, C) * 1e-3, torch.empty(B, T // 2, dtype=torch.bool, device='cuda')
    hid, dhid = 3 * rnd(B, To, 4 * C), rnd(B, To, 4 * C) * 1e-3
    ohid = torch.empty_like(hid)
    r_, h_, dy_ = rnd(B, To, C), rnd(B, To, C), rnd(B, To, C) * 1e-3
    ls = (0.5 + 0.25 * rnd(C))
    o1, o2, dls = torch.empty_like(r_), torch.empty_like(r_), torch.empty_like(ls)
    F4 = 4.0
    ops = {   # name -> (call, bytes it must move)
        'dwconv3': (lambda: l.check(L.dcf_op_dwconv3(P(x), P(mask), P(w), P(y3), B, T, C, 3, stride, st)), F4 * C * B * (T + 3 * To)),
        'dwconv3_bwd': (lambda: l.check(L.dcf_op_dwconv3_bwd(P(x), P(mask), P(w), P(dy3), P(dx), P(dw), B, T, C, 3, stride, 0, st)),
                        F4 * C * B * (2 * T + 2 * 3 * To)),      # dY is read by the data and by the weight kernel
        'dwconv3_bwd_dx': (lambda: l.check(L.dcf_op_dwconv3_bwd(P(x), P(mask), P(w), P(dy3), P(dx), None, B, T, C, 3, stride, 0, st)),
                           F4 * C * B * (T + 3 * To)),
        'dwconv3_bwd_dw': (lambda: l.check(L.dcf_op_dwconv3_bwd(P(x), P(mask), P(w), P(dy3), None, P(dw), B, T, C, 3, stride, 0, st)),
                           F4 * C * B * (T + 3 * To)),
        'maxpool': (lambda: l.check(L.dcf_op_masked_maxpool(P(x), P(mask), P(yp), P(mop), B, T, C, st)), F4 * C * B * (2 * T + T // 2)),
        'maxpool_bwd': (lambda: l.check(L.dcf_op_masked_maxpool_bwd(P(x), P(mask), P(dyp), P(dx), B, T, C, st)), F4 * C * B * (3 * T + T // 2)),
        'gelu': (lambda: l.check(L.dcf_op_gelu(P(hid), P(ohid), hid.numel(), st)), F4 * 2 * hid.numel()),
        'gelu_bwd': (lambda: l.check(L.dcf_op_gelu_bwd(P(hid), P(dhid), P(ohid), hid.numel(), st)), F4 * 3 * hid.numel()),
        'layerscale': (lambda: l.check(L.dcf_op_layerscale_residual(P(r_), P(mo), P(h_), None, P(ls), P(o1), B * To, C, st)), F4 * 3 * r_.numel()),
        'layerscale_bwd': (lambda: l.check(L.dcf_op_layerscale_residual_bwd(P(dy_), P(h_), P(mo), None, P(ls), P(o1), P(o2), P(dls), B * To, C, 0, st)),
                           F4 * 4 * r_.numel()),
    }
    torch.manual_seed(1)
    blk = pkg.modeling.TransformerEncoder(C, stride, heads, window).cuda()
    with torch.no_grad():
        blk.drop_path_attn.scale.fill_(0.5)
        blk.drop_path_ffn.scale.fill_(0.5)
    up = rnd(B, To, C) * 1e-3
    params = list(blk.parameters())
    xr = x.clone().requires_grad_(True)

    def ours():
        y, _ = A.transformer_encoder(xr, mask, blk)
        torch.autograd.grad(y, [xr] + params, up)

    def eager():
        y = eager_block(torch, blk, xr, mask, stride, heads, window)
        torch.autograd.grad(y, [xr] + params, up)

    with torch.no_grad():       # the two blocks compute the same thing
        ya, yb = A.transformer_encoder(x, mask, blk)[0], eager_block(torch, blk, x, mask, stride, heads, window)
        valid = mo[..., None]
    r = {'B': B, 'T': T, 'C': C, 'heads': heads, 'window': window, 'stride': stride,
         'block_vs_eager_max_abs_diff_valid_rows': float(((ya - yb) * valid).abs().max())}
    for rep in range(2):
        for name, (fn, _) in ops.items():
            r[f'{name}_us_{rep}'] = timed(torch, fn)
        r[f'block_fwd_bwd_us_{rep}'] = timed(torch, ours)
        r[f'eager_block_fwd_bwd_us_{rep}'] = timed(torch, eager)
    for name, (_, nbytes) in ops.items():
        r[f'{name}_gbs'] = nbytes / r[f'{name}_us_0'] * 1e-3
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
    rows = []
    for level, stride in ((0, 1), (1, 2)):
        cmd = ['timeout', '-k', '10', str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), '--one', '8', '16384', str(kw['E']),
               str(kw['n_heads']), str(kw['win']), str(stride)]
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
