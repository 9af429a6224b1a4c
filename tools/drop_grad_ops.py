"""The six operators of the training extension at the bench shape (E = 256, T = 16384, eight rows), 20 calls each after 3 warm-up calls;
run under
rocprofv3 --kernel-trace --stats (profiles/drop_grad.md, section 2)."""
import importlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module('cvpr2025-decafnet_amd')
L, lib = pkg._lib, pkg._lib.lib()
B, T, E = 8, 16384, 256
p_ = L.ptr
st = L.current_stream()
seed, site, psite = 0x1234567890ABCDEF, 3 << 16 | 2, 3 << 16 | 4
x = torch.randn(B, T, E, device='cuda')
h2, g2 = torch.randn(B, T, 2 * E, device='cuda'), torch.empty(B, T, 2 * E, device='cuda')
h4, gy4, y4 = torch.randn(B, T, 4 * E, device='cuda'), torch.randn(B, T, 4 * E, device='cuda'), torch.empty(B, T, 4 * E, device='cuda')
r, gy, y, dr, dh = (torch.randn(B, T, E, device='cuda') for _ in range(5))
ls, dls = torch.randn(E, device='cuda'), torch.empty(E, device='cuda')
m = (torch.arange(T, device='cuda')[None] < torch.tensor([T, T - 100, T, T // 2, T, T, T - 1, T], device='cuda')[:, None]).to(torch.uint8).contiguous()
for p, pp in ((0.1, 0.1), (0.0, 0.0)):
    for i in range(23):
        L.check(lib.dcf_op_dropout(p_(h2), p_(g2), B, T, 2 * E, 0, seed, site, p, st))
        L.check(lib.dcf_op_gelu_dropout(p_(h4), p_(y4), B, T, 4 * E, 0, seed, site, p, st))
        L.check(lib.dcf_op_gelu_dropout_bwd(p_(h4), p_(gy4), p_(y4), B, T, 4 * E, 0, seed, site, p, st))
        L.check(lib.dcf_op_drop_residual(p_(r), None, p_(x), p_(m), p_(ls), p_(y), B, T, E, 0, seed, site, p, psite, pp, st))
        L.check(lib.dcf_op_drop_residual_bwd(p_(gy), p_(x), None, p_(m), p_(ls), p_(dr), p_(dh), p_(dls), B, T, E, 0, seed, site, p, psite, pp, 0, st))
        if p == 0.0:                                       # the plain pairs they replace / reduce to
            L.check(lib.dcf_op_gelu(p_(h4), p_(y4), h4.numel(), st))
            L.check(lib.dcf_op_gelu_bwd(p_(h4), p_(gy4), p_(y4), h4.numel(), st))
    torch.cuda.synchronize()
print('done')
