"""Time of the k5 / stride-2 gradient pair of csrc/conv_grad.hip (dcf_op_conv5s2_bwd_data + dcf_op_conv5s2_bwd_weight) at the bench's
embedding shape (B * T = 16 384 input rows, E = 256) and, as the yardstick, of the k = 3 pair (dcf_op_conv_bwd_data + _weight) at the same
number of OUTPUT rows (8 192), between device events, alternating rounds, median of the rounds (profiles/backbone_grad.md).

    python tools/backbone_grad_time.py [--rows 16384] [--E 256] [--iters 50] [--rounds 5]
"""
import argparse
import importlib
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=16384)
    ap.add_argument('--E', type=int, default=256)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    pkg = importlib.import_module('cvpr2025-decafnet_amd')
    l, L = pkg._lib, pkg._lib.lib()
    E, T, To = a.E, a.rows, a.rows // 2
    gen = torch.Generator().manual_seed(1)
    x5, x3 = torch.randn(1, T, E, generator=gen).cuda(), torch.randn(1, To, E, generator=gen).cuda()
    dy = (torch.randn(1, To, E, generator=gen) * 1e-3).cuda()
    w5, w3 = (torch.randn(E, E, 5, generator=gen) / (5 * E) ** 0.5).cuda(), (torch.randn(E, E, 3, generator=gen) / (3 * E) ** 0.5).cuda()
    m5, m3 = torch.ones(1, T, dtype=torch.bool).cuda(), torch.ones(1, To, dtype=torch.bool).cuda()
    dx5, dx3, dw5, dw3 = torch.empty_like(x5), torch.empty_like(x3), torch.empty_like(w5), torch.empty_like(w3)
    st = l.current_stream()
    runs = {
        'k5s2 bwd_data': lambda: l.check(L.dcf_op_conv5s2_bwd_data(l.ptr(dy), l.ptr(m5), l.ptr(w5), l.ptr(dx5), 1, T, E, E, st)),
        'k5s2 bwd_weight': lambda: l.check(L.dcf_op_conv5s2_bwd_weight(l.ptr(x5), l.ptr(m5), l.ptr(dy), l.ptr(dw5), 1, T, E, E, 0, st)),
        'k3 bwd_data': lambda: l.check(L.dcf_op_conv_bwd_data(l.ptr(dy), l.ptr(m3), l.ptr(w3), l.ptr(dx3), 1, To, E, E, 3, st)),
        'k3 bwd_weight': lambda: l.check(L.dcf_op_conv_bwd_weight(l.ptr(x3), l.ptr(m3), l.ptr(dy), l.ptr(dw3), None, 1, To, E, E, 3, 0, st)),
    }
    times = {k: [] for k in runs}
    for fn in runs.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for k, fn in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1000.0 / a.iters)
    for k, v in times.items():
        print(f'BGTIME {k}: median {statistics.median(v):.1f} us  min {min(v):.1f}  max {max(v):.1f}  ({a.rounds} rounds x {a.iters} calls, rows {T}, E {E})')
    print(f"BGTIME pair k5s2 {statistics.median(times['k5s2 bwd_data']) + statistics.median(times['k5s2 bwd_weight']):.1f} us, "
          f"pair k3 {statistics.median(times['k3 bwd_data']) + statistics.median(times['k3 bwd_weight']):.1f} us")


if __name__ == '__main__':
    main()
