"""Time the backward of MaskedConv1D / channel LayerNorm (csrc/conv_grad.hip) at the head shape of the bench workload and next
to torch-ROCm's own autograd on the same tensors.

    python tools/conv_grad_time.py [--rows 130560] [--out profiles/conv_grad_times.json]

rows = 32 640 x 4 (four queries of the bench video), C = 256 and 288, k = 3, plus both output convolutions (N = 1, 2).  Each
export: 50 calls after 10 warm-up calls between device events; torch's `autograd.grad` through F.conv1d / the restated LayerNorm
is timed the same way, the two alternating.  Prints one JSON object; the weight gradient's TFLOP/s (2 rows N kC) is set
against the nominal f16x3 peak and against the rate dcf_calib_mfma_rate sustains."""
import argparse
import ctypes
import importlib
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARM, CALLS = 10, 50


def timed(fn):
    for _ in range(WARM):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / CALLS * 1e3        # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=32640 * 4)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    pkg = importlib.import_module('cvpr2025-decafnet_amd')
    l, L = pkg._lib, pkg._lib.lib()
    st = l.current_stream()
    ncu, ns = ctypes.c_int32(), ctypes.c_float()
    l.check(L.dcf_calib_mfma_rate(0, 1 << 15, ctypes.byref(ncu), ctypes.byref(ns)))
    # one v_mfma_f32_32x32x16_f16 = 2 * 32 * 32 * 16 flop per SIMD, 4 SIMDs per CU; f16x3 spends three of them per multiply-add
    per_mfma = 2 * 32 * 32 * 16
    nominal = per_mfma / (32 / 2.4e9) * 4 * ncu.value / 3 / 1e12
    sustained = per_mfma / (ns.value * 1e-9) * 4 * ncu.value / 3 / 1e12
    out = {'rows': args.rows, 'n_cus': ncu.value, 'ns_per_mfma': ns.value, 'f16x3_peak_tflops_nominal': nominal, 'f16x3_peak_tflops_sustained': sustained,
           'cases': []}
    B, T = 4, args.rows // 4
    gen = torch.Generator().manual_seed(0)
    for C, N in ((256, 256), (288, 288), (256, 1), (288, 2)):
        x = torch.randn(B, T, C, generator=gen).cuda()
        w = (torch.randn(N, C, 3, generator=gen) / (3 * C) ** 0.5).cuda()
        dy = (torch.randn(B, T, N, generator=gen) * 1e-4).cuda()
        mask = (torch.arange(T)[None] < torch.tensor([T, T, T * 3 // 4, T // 2])[:, None]).cuda()
        dx, dw, db = torch.empty_like(x), torch.empty_like(w), torch.empty(N, device='cuda')
        f_data = lambda: l.check(L.dcf_op_conv_bwd_data(l.ptr(dy), l.ptr(mask), l.ptr(w), l.ptr(dx), B, T, C, N, 3, st))
        f_wgt = lambda: l.check(L.dcf_op_conv_bwd_weight(l.ptr(x), l.ptr(mask), l.ptr(dy), l.ptr(dw), l.ptr(db), B, T, C, N, 3, 0, st))
        xc = (x * mask[..., None]).transpose(1, 2).contiguous().requires_grad_(True)      # torch's layout, mask applied outside the timing
        wr = w.clone().requires_grad_(True)
        dyc = dy.transpose(1, 2).contiguous()

        def t_data():
            return torch.autograd.grad(F.conv1d(xc, wr, None, padding=1), xc, dyc)

        def t_wgt():
            return torch.autograd.grad(F.conv1d(xc, wr, None, padding=1), wr, dyc)

        def t_fwd():
            with torch.no_grad():
                return F.conv1d(xc, wr, None, padding=1)
        r = {'op': 'conv_k3', 'C': C, 'N': N}
        for rep in range(2):                       # alternate ours / torch's
            r[f'ours_data_us_{rep}'], r[f'torch_data_plus_fwd_us_{rep}'] = timed(f_data), timed(t_data)
            r[f'ours_weight_us_{rep}'], r[f'torch_weight_plus_fwd_us_{rep}'] = timed(f_wgt), timed(t_wgt)
        r['torch_fwd_us'] = timed(t_fwd)
        flops = 2.0 * args.rows * N * 3 * C
        best = min(r['ours_weight_us_0'], r['ours_weight_us_1'])
        r['weight_tflops'] = flops / (best * 1e-6) / 1e12
        r['weight_fraction_of_nominal_peak'] = r['weight_tflops'] / nominal
        r['weight_fraction_of_sustained'] = r['weight_tflops'] / sustained
        out['cases'].append(r)
        print(json.dumps(r), flush=True)
    for C in (256, 288):
        rows = args.rows
        x = torch.randn(rows, C, generator=gen).cuda()
        w, b = (1 + 0.1 * torch.randn(C, generator=gen)).cuda(), (0.1 * torch.randn(C, generator=gen)).cuda()
        do = (torch.randn(rows, C, generator=gen) * 1e-4).cuda()
        dx, dw, db = torch.empty_like(x), torch.empty_like(w), torch.empty_like(b)
        f_ln = lambda: l.check(L.dcf_op_layernorm_bwd(l.ptr(x), l.ptr(w), l.ptr(b), l.ptr(do), l.ptr(dx), l.ptr(dw), l.ptr(db), rows, C, 1, 0, st))
        xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))

        def ln(x_, w_, b_):
            x_ = x_ - x_.mean(-1, keepdim=True)
            x_ = x_ / torch.sqrt((x_ * x_).mean(-1, keepdim=True) + 1e-5)
            return torch.relu(x_ * w_ + b_)

        def t_ln():
            return torch.autograd.grad(ln(xr, wr, br), (xr, wr, br), do)

        def t_fwd():
            with torch.no_grad():
                return ln(xr, wr, br)
        r = {'op': 'layernorm_relu', 'C': C}
        for rep in range(2):
            r[f'ours_us_{rep}'], r[f'torch_plus_fwd_us_{rep}'] = timed(f_ln), timed(t_ln)
        r['torch_fwd_us'] = timed(t_fwd)
        r['ours_gbps'] = 3.0 * rows * C * 4 / (min(r['ours_us_0'], r['ours_us_1']) * 1e-6) / 1e9
        out['cases'].append(r)
        print(json.dumps(r), flush=True)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
