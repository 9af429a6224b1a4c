"""GPU checks of the backward of MaskedConv1D and of the channel LayerNorm (csrc/conv_grad.hip: dcf_op_conv_bwd_data,
dcf_op_conv_bwd_weight, dcf_op_layernorm_bwd) and of the autograd functions and the head composed of them (autograd.py).

The yardstick is the project's gradient rule (tests/test_gpu_objective_grad.py), per gradient tensor:

    e_gpu <= max(4 * e_ref, 2^-21 * max |g_64|),   e = max |g - g_64|

with g_64 the fp64 result (the reference's fp64 `backward()` for the fixture, tests/conv_grad_ref.py elsewhere) and e_ref the
error of fp32 torch on the CPU (the reference module's fp32 `backward()` for the fixture; F.conv1d / the restated LayerNorm
under fp32 autograd elsewhere).  Every check prints a `CGERR` line (e_gpu / bound among the figures); the worst per case are in
profiles/conv_grad.md.

In the operator cases dY is random on EVERY row, padded ones included, and masks have holes.  In the LayerNorm cases elements
whose fp64 pre-ReLU output lies within 1e-4 of the kink carry no upstream gradient (fp32 and fp64 may land on different sides
there); exact zeros (w = b = 0 in one channel) are kept: they must block the gradient.

Measured on an MI355X (profiles/conv_grad.md): weight gradients at most 0.59 of the bound, LayerNorm at most 0.43, the composed head
at most 0.73.  The k3 data gradient at C = N = 256 / 288 -- the forward's own tap-3 f16x3 GEMM, 144 / 162 dependent accumulations of
one fp32 accumulator -- sits AT the bound: e_gpu / bound 1.000 (B 4, T 63: 3.281e-9 against 3.282e-9), 0.93, 0.86, 0.85.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import Golden, load_pkg
import conv_grad_ref as R
from test_conv_grad_cpu import FIXTURES, fixture_case

pytestmark = pytest.mark.gpu
FLOOR = 2.0 ** -21
E2E_TOL = dict(rtol=2e-4, atol=2e-4)          # what tests/test_gpu_e2e.py used before its gates moved to the rule


def check(tag, got, g64, g32):
    got, g64, g32 = got.detach().cpu().double(), g64.detach().double(), g32.detach().double()
    assert got.shape == g64.shape == g32.shape, (tag, got.shape, g64.shape, g32.shape)
    assert bool(torch.isfinite(got).all()), tag
    e_ref, e_gpu, top = float((g32 - g64).abs().max()), float((got - g64).abs().max()), float(g64.abs().max())
    bound = max(4 * e_ref, FLOOR * top)
    print(f'CGERR {tag}: max|g64| {top:.3e} e_ref {e_ref:.3e} e_gpu {e_gpu:.3e} bound {bound:.3e} ratio {e_gpu / bound if bound else 0.0:.3f}')
    assert e_gpu <= bound, (tag, e_gpu, bound)
    return bound


def holes(B, T, gen):
    """a mask with holes: single invalid rows inside every sequence and, in the odd sequences, a fully padded tail"""
    m = torch.rand(B, T, generator=gen) > 0.15
    for b in range(1, B, 2):
        m[b, T - T // 4:] = False
    return m


class Lib:
    def __init__(self):
        self.pkg = load_pkg()
        self.L, self.l = self.pkg._lib.lib(), self.pkg._lib

    def conv_bwd(self, x, mask, w, dy, accumulate=0, dw0=None, db0=None, want_db=True):
        B, T, Cin = x.shape
        N, _, k = w.shape
        l, st = self.l, self.l.current_stream()
        dx = torch.full_like(x, float('nan'))
        dw = dw0.clone() if accumulate else torch.full_like(w, float('nan'))
        db = (db0.clone() if accumulate else torch.full((N,), float('nan'), device=x.device)) if want_db else None
        l.check(self.L.dcf_op_conv_bwd_data(l.ptr(dy), l.ptr(mask), l.ptr(w), l.ptr(dx), B, T, Cin, N, k, st), 'bwd_data')
        l.check(self.L.dcf_op_conv_bwd_weight(l.ptr(x), l.ptr(mask), l.ptr(dy), l.ptr(dw), l.ptr(db), B, T, Cin, N, k, accumulate, st), 'bwd_weight')
        return dx, dw, db

    def ln_bwd(self, x, w, b, do, relu, accumulate=0, dw0=None, db0=None):
        rows, C = x.shape
        l, st = self.l, self.l.current_stream()
        dx = torch.full_like(x, float('nan'))
        dw = dw0.clone() if accumulate else torch.full_like(w, float('nan'))
        db = db0.clone() if accumulate else torch.full_like(b, float('nan'))
        l.check(self.L.dcf_op_layernorm_bwd(l.ptr(x), l.ptr(w), l.ptr(b), l.ptr(do), l.ptr(dx), l.ptr(dw), l.ptr(db), rows, C, relu, accumulate, st),
                'layernorm_bwd')
        return dx, dw, db


@pytest.fixture(scope='module')
def lib():
    return Lib()


def conv_case(B, T, Cin, N, k, seed, masked=True):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, Cin, generator=gen)
    w = torch.randn(N, Cin, k, generator=gen) / (Cin * k) ** 0.5
    dy = torch.randn(B, T, N, generator=gen) * 1e-3          # every row, padded ones too
    mask = holes(B, T, gen) if masked else None
    return x, mask, w, dy


def conv_refs(x, mask, w, dy):
    """((dX, dW, db) in fp64 by the restatement, the same from fp32 autograd through F.conv1d on the CPU)"""
    m64 = mask
    g64 = R.conv_grads(x.double(), m64, w.double(), dy.double())
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    br = torch.zeros(w.size(0), requires_grad=True)
    xm = xr if mask is None else xr * mask[..., None].float()
    y = F.conv1d(xm.transpose(1, 2), wr, br, padding=(w.size(-1) - 1) // 2).transpose(1, 2)
    g32 = torch.autograd.grad((y * dy).sum(), (xr, wr, br))
    return g64, g32


SHAPES = [(64, 64, 3), (256, 256, 3), (288, 288, 3), (256, 1, 3), (288, 2, 3), (256, 1024, 1), (1024, 256, 1)]
SIZES = [(2, 200), (3, 1100), (1, 1), (4, 63)]


@pytest.mark.parametrize('B,T', SIZES)
@pytest.mark.parametrize('Cin,N,k', SHAPES)
def test_conv_gradients_match_fp64(lib, Cin, N, k, B, T):
    accumulate = (Cin + N + B) % 2
    x, mask, w, dy = conv_case(B, T, Cin, N, k, seed=Cin * 7 + N * 3 + k + B * T, masked=(B, T) != (1, 1) or Cin == 64)
    g64, g32 = conv_refs(x, mask, w, dy)
    gen = torch.Generator().manual_seed(1)
    dw0 = (torch.randn(w.shape, generator=gen) * float(g64[1].abs().max()) / 8).float()
    db0 = (torch.randn(N, generator=gen) * float(g64[2].abs().max()) / 8).float()
    c = lambda t: None if t is None else t.cuda()
    dx, dw, db = lib.conv_bwd(c(x), c(mask), c(w), c(dy), accumulate, c(dw0), c(db0))
    tag = f'conv C{Cin} N{N} k{k} B{B} T{T} acc{accumulate}'
    check(tag + ' dX', dx, g64[0], g32[0])
    if accumulate:
        dw, db = dw.cpu().double() - dw0.double(), db.cpu().double() - db0.double()
    check(tag + ' dW', dw, g64[1], g32[1])
    check(tag + ' db', db, g64[2], g32[2])
    if mask is not None:
        assert bool((dx.cpu()[~mask] == 0).all()), 'dX at a padded row is exactly 0'


@pytest.mark.parametrize('Cin,N', [(64, 64), (256, 2)])
def test_taps_stop_at_sequence_seams_and_masked_rows(lib, Cin, N):
    """rows next to a seam and one masked row hold values 100 times the rest: a tap that crossed the seam, or read the masked
    row, would move dW by far more than the bound"""
    B, T = 2, 64
    x, _, w, dy = conv_case(B, T, Cin, N, 3, seed=5, masked=False)
    mask = torch.ones(B, T, dtype=torch.bool)
    mask[0, 30] = False
    x[0, T - 1] *= 100
    x[1, 0] *= 100
    x[0, 30] *= 100
    g64, g32 = conv_refs(x, mask, w, dy)
    dx, dw, db = lib.conv_bwd(x.cuda(), mask.cuda(), w.cuda(), dy.cuda())
    bound = check(f'seam C{Cin} N{N} dW', dw, g64[1], g32[1])
    check(f'seam C{Cin} N{N} dX', dx, g64[0], g32[0])
    # the same rows as ONE sequence without a mask: what a kernel that ignored the seam / the mask would compute
    wrong_seam = R.conv_bwd_weight(x.double().reshape(1, B * T, Cin), mask.reshape(1, B * T), dy.double().reshape(1, B * T, N), 3)[0]
    wrong_mask = R.conv_bwd_weight(x.double(), None, dy.double(), 3)[0]
    assert float((wrong_seam - g64[1]).abs().max()) > 100 * bound and float((wrong_mask - g64[1]).abs().max()) > 100 * bound


def ln_case(rows, C, relu, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, C, generator=gen) * 1.5 + 0.3
    x[0] = 0.5                                             # a constant row: variance 0, rstd = eps^-1/2
    w = 1 + 0.3 * torch.randn(C, generator=gen)
    b = 0.2 * torch.randn(C, generator=gen)
    w[3], b[3] = 0.0, 0.0                                  # channel 3: the output is exactly 0 in every row
    do = torch.randn(rows, C, generator=gen) * 1e-2
    if relu:
        y64 = R.layer_norm(x.double(), w.double(), b.double())
        do[(y64.abs() < 1e-4) & (y64 != 0)] = 0.0
    return x, w, b, do


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('rows', [1, 5, 4097])
@pytest.mark.parametrize('C', [64, 256, 288, 1024])
def test_layernorm_backward_matches_fp64(lib, C, rows, relu):
    x, w, b, do = ln_case(rows, C, relu, seed=C + rows + relu)
    g64 = R.layer_norm_grads(x.double(), w.double(), b.double(), do.double(), bool(relu))
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    g32 = torch.autograd.grad((R.layer_norm(xr, wr, br, bool(relu)) * do).sum(), (xr, wr, br))
    accumulate = (C // 32 + rows) % 2
    gen = torch.Generator().manual_seed(2)
    dw0 = (torch.randn(C, generator=gen) * float(g64[1].abs().max()) / 8).float()
    db0 = (torch.randn(C, generator=gen) * float(g64[2].abs().max()) / 8).float()
    dx, dw, db = lib.ln_bwd(x.cuda(), w.cuda(), b.cuda(), do.cuda(), relu, accumulate, dw0.cuda(), db0.cuda())
    if accumulate:
        dw, db = dw.cpu().double() - dw0.double(), db.cpu().double() - db0.double()
    tag = f'ln C{C} rows{rows} relu{relu} acc{accumulate}'
    check(tag + ' dX', dx, g64[0], g32[0])
    check(tag + ' dw', dw, g64[1], g32[1])
    check(tag + ' db', db, g64[2], g32[2])
    if relu:                                           # an output of exactly 0 blocks the gradient
        tiny = FLOOR * float(g64[2].abs().max())
        assert abs(float(db[3])) <= (tiny if accumulate else 0.0) and abs(float(dw[3])) <= (tiny if accumulate else 0.0)


@pytest.mark.parametrize('Cin,N', [(288, 288), (288, 2)])
def test_power_of_two_scaling_of_dY_commutes_bit_for_bit(lib, Cin, N):
    x, mask, w, dy = conv_case(2, 200, Cin, N, 3, seed=11)
    lx, lw, lb, ldo = ln_case(400, Cin, 1, seed=12)
    outs = []
    for s in (2.0 ** -30, 1.0, 2.0 ** 10):
        got = lib.conv_bwd(x.cuda(), mask.cuda(), w.cuda(), (dy * s).cuda())
        got += lib.ln_bwd(lx.cuda(), lw.cuda(), lb.cuda(), (ldo * s).cuda(), 1)
        outs.append([g.cpu() / s for g in got])
    for a, b_, c in zip(*outs):
        assert torch.equal(a, b_) and torch.equal(b_, c)


def test_ten_repeats_are_bit_identical(lib):
    x, mask, w, dy = conv_case(3, 1100, 288, 288, 3, seed=21)
    lx, lw, lb, ldo = ln_case(3300, 288, 1, seed=22)
    args = [t.cuda() for t in (x, mask, w, dy)]
    largs = [t.cuda() for t in (lx, lw, lb, ldo)]
    first = None
    for _ in range(10):
        got = [g.clone() for g in lib.conv_bwd(*args) + lib.ln_bwd(*largs, 1)]
        if first is None:
            first = got
        else:
            assert all(torch.equal(a, b_) for a, b_ in zip(first, got))


def make_head(pkg, name, params):
    head = pkg.modeling.ConvHead(64, 'cls_head', 1, prior_prob=0.01) if name == 'cls' else pkg.modeling.ConvHead(64, 'reg_head', 2, num_fpn_levels=3)
    head.load_state_dict(params)
    return head.cuda()


@pytest.mark.parametrize('name', ['cls', 'reg'])
def test_conv_head_matches_the_reference_backward(name):
    pkg = load_pkg()
    xs, masks, params, ups, g = fixture_case(name, torch.float32)
    head = make_head(pkg, name, params)
    xs = [x.cuda().requires_grad_(True) for x in xs]
    outs = [pkg.autograd.conv_head(x, m.cuda(), head, level=i) for i, (x, m) in enumerate(zip(xs, masks))]
    sum((o * u.cuda()).sum() for o, u in zip(outs, ups)).backward()
    for i, (o, x) in enumerate(zip(outs, xs)):
        torch.testing.assert_close(o.detach().cpu(), g.t(f'{name}/out32/l{i}'), **E2E_TOL)
        check(f'head {name} l{i} dX', x.grad.transpose(1, 2), g.t(f'{name}/gx64/l{i}'), g.t(f'{name}/gx32/l{i}'))
    seen = 0
    for k, p in head.named_parameters():
        if f'{name}/gp64/{k}' in g:
            check(f'head {name} {k}', p.grad, g.t(f'{name}/gp64/{k}'), g.t(f'{name}/gp32/{k}'))
            seen += 1
        else:
            assert p.grad is None, k
    assert seen >= 7


def test_heads_train_through_the_point_objective():
    pkg = load_pkg()
    B, T, L, E = 2, 64, 3, 64
    gen = torch.Generator().manual_seed(3)
    cls1, cls2 = (make_head(pkg, 'cls', fixture_case('cls', torch.float32)[2]) for _ in range(2))
    reg = make_head(pkg, 'reg', fixture_case('reg', torch.float32)[2])
    xs = [torch.randn(B, T >> l, E, generator=gen).cuda() for l in range(L)]
    masks = [(torch.arange(T >> l)[None] < torch.tensor([T >> l, (T * 3 // 4) >> l])[:, None]).cuda() for l in range(L)]
    A = pkg.autograd
    outputs = (tuple(A.conv_head(x, m, cls1) for x, m in zip(xs, masks)), tuple(A.conv_head(x, m, cls2) for x, m in zip(xs, masks)),
               tuple(A.conv_head(x, m, reg, level=l) for l, (x, m) in enumerate(zip(xs, masks))), tuple(masks))
    obj = pkg.loss.PointObjective(pkg.config.make_opt(n_levels=L, max_seq_len=T))
    total = obj(outputs, torch.tensor([[10.0, 30.5], [3.0, 20.0]]).cuda())['total']
    assert bool(torch.isfinite(total))
    params = [p for h in (cls1, cls2, reg) for k, p in h.named_parameters()]
    grads = torch.autograd.grad(total, params)
    assert len(grads) == len(params) and all(bool(torch.isfinite(gr).all()) for gr in grads)
    assert any(float(gr.abs().max()) > 0 for gr in grads)
