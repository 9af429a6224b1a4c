"""GPU checks of the operator pairs of csrc/enc_grad.hip (depthwise convolution, masked max pooling, GELU, LayerScale residual) and of
the autograd functions over them, up to autograd.transformer_encoder.

The yardstick is the project's gradient rule (tests/test_gpu_conv_grad.py, test_gpu_attn_grad.py), per gradient tensor:

    e_gpu <= max(4 * e_ref, 2^-21 * max |g_64|),   e = max |g - g_64|

with g_64 fp64 autograd on the CPU through the oracle's functions (masked_conv1d with groups = C, masked_max_pool1d, F.gelu,
transformer_encoder; the reference's own fp64 `backward()` for the fixture) and e_ref the error of the same in fp32 (the reference's
fp32 `backward()` for the fixture).  Forward values go by the same rule with y_64 in place of g_64 (tests/forward_parity.py).  Every
check prints an `EGERR` line; the worst per case are in profiles/enc_grad.md.

In the operator cases inputs are N(0, 1), the upstream gradient is 1e-3 N(0, 1) on EVERY row, padded ones included, masks have holes
and outputs are pre-filled with NaN.  The pooling gradient is compared bit for bit: it is a sum of at most two fp32 values.

attn.k_norm.bias and attn.attn.key.bias of the block: a constant added to every key moves all scores of a row alike, so these two
gradients are 0 in exact arithmetic and g_64, g_32 and the GPU's result are three roundings of 0; their floor is taken from
max |g_64| of k_norm.weight / key.weight, the terms that cancel.
"""
import pytest
import torch
import torch.nn.functional as F

from conftest import load_pkg
import enc_grad_ref as R
from test_enc_grad_cpu import ZERO_BY_SYMMETRY, encoder_fixture, oracle_encoder_grads, tie_case

pytestmark = pytest.mark.gpu
FLOOR = 2.0 ** -21
NAN = float('nan')


def check(tag, got, g64, g32, top=None):
    got, g64, g32 = got.detach().cpu().double(), g64.detach().double(), g32.detach().double()
    assert got.shape == g64.shape == g32.shape, (tag, got.shape, g64.shape, g32.shape)
    assert bool(torch.isfinite(got).all()), tag
    e_ref, e_gpu = float((g32 - g64).abs().max()), float((got - g64).abs().max())
    top = float(g64.abs().max()) if top is None else top
    bound = max(4 * e_ref, FLOOR * top)
    print(f'EGERR {tag}: max|g64| {top:.3e} e_ref {e_ref:.3e} e_gpu {e_gpu:.3e} bound {bound:.3e} ratio {e_gpu / bound if bound else 0.0:.3f}')
    assert e_gpu <= bound, (tag, e_gpu, bound)
    return bound


class Lib:
    """the eight exports on device tensors; outputs pre-filled with NaN, None where not wanted"""

    def __init__(self):
        self.pkg = load_pkg()
        self.L, self.l = self.pkg._lib.lib(), self.pkg._lib

    def dw(self, x, mask, w, stride):
        B, T, C = x.shape
        l, n = self.l, w.size(0)
        y = torch.full((n, B, T // stride, C), NAN, device='cuda')
        l.check(self.L.dcf_op_dwconv3(l.ptr(x), l.ptr(mask), l.ptr(w), l.ptr(y), B, T, C, n, stride, l.current_stream()), 'dcf_op_dwconv3')
        return y

    def dw_bwd(self, x, mask, w, dy, stride, want=(True, True), into=None):
        B, T, C = x.shape
        l, n = self.l, w.size(0)
        dx = torch.full_like(x, NAN) if want[0] else None
        dw = (torch.full_like(w, NAN) if into is None else into) if want[1] else None
        l.check(self.L.dcf_op_dwconv3_bwd(l.ptr(x), l.ptr(mask), l.ptr(w), l.ptr(dy), l.ptr(dx), l.ptr(dw), B, T, C, n, stride, int(into is not None),
                                          l.current_stream()), 'dcf_op_dwconv3_bwd')
        return dx, dw

    def pool(self, x, mask):
        B, T, C = x.shape
        l = self.l
        y = torch.full((B, T // 2, C), NAN, device='cuda')
        mo = torch.full((B, T // 2), 7, dtype=torch.uint8, device='cuda')
        l.check(self.L.dcf_op_masked_maxpool(l.ptr(x), l.ptr(mask), l.ptr(y), l.ptr(mo), B, T, C, l.current_stream()), 'dcf_op_masked_maxpool')
        return y, mo

    def pool_bwd(self, x, mask, dy):
        B, T, C = x.shape
        l = self.l
        dx = torch.full_like(x, NAN)
        l.check(self.L.dcf_op_masked_maxpool_bwd(l.ptr(x), l.ptr(mask), l.ptr(dy), l.ptr(dx), B, T, C, l.current_stream()), 'dcf_op_masked_maxpool_bwd')
        return dx

    def gelu(self, x):
        l = self.l
        y = torch.full_like(x, NAN)
        l.check(self.L.dcf_op_gelu(l.ptr(x), l.ptr(y), x.numel(), l.current_stream()), 'dcf_op_gelu')
        return y

    def gelu_bwd(self, x, dy):
        l = self.l
        dx = torch.full_like(x, NAN)
        l.check(self.L.dcf_op_gelu_bwd(l.ptr(x), l.ptr(dy), l.ptr(dx), x.numel(), l.current_stream()), 'dcf_op_gelu_bwd')
        return dx

    def ls(self, r, mr, h, mh, ls):
        l = self.l
        rows, C = r.numel() // r.size(-1), r.size(-1)
        y = torch.full_like(r, NAN)
        l.check(self.L.dcf_op_layerscale_residual(l.ptr(r), l.ptr(mr), l.ptr(h), l.ptr(mh), l.ptr(ls), l.ptr(y), rows, C, l.current_stream()),
                'dcf_op_layerscale_residual')
        return y

    def ls_bwd(self, dy, h, mr, mh, ls, want=(True, True, True), into=None):
        l = self.l
        rows, C = dy.numel() // dy.size(-1), dy.size(-1)
        dr = torch.full_like(dy, NAN) if want[0] else None
        dh = torch.full_like(dy, NAN) if want[1] else None
        dls = (torch.full_like(ls, NAN) if into is None else into) if want[2] else None
        l.check(self.L.dcf_op_layerscale_residual_bwd(l.ptr(dy), l.ptr(h), l.ptr(mr), l.ptr(mh), l.ptr(ls), l.ptr(dr), l.ptr(dh), l.ptr(dls), rows, C,
                                                      int(into is not None), l.current_stream()), 'dcf_op_layerscale_residual_bwd')
        return dr, dh, dls


@pytest.fixture(scope='module')
def lib():
    return Lib()


def cu(*ts):
    return [None if t is None else t.cuda() for t in ts]


# ------------------------------------------------------------------------------------------
# depthwise convolution
# ------------------------------------------------------------------------------------------
def dw_case(B, T, C, n, stride, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, C, generator=gen)
    w = torch.randn(n, C, 3, generator=gen)
    dy = torch.randn(n, B, T // stride, C, generator=gen) * 1e-3
    return x, w, dy, R.holes(B, T, gen)


def dw_refs(x, mask, w, dy, stride):
    """((Y, dX, dW) by fp64 autograd through the oracle's masked_conv1d, the same in fp32)"""
    out = []
    for dt in (torch.float64, torch.float32):
        xr, wr = x.to(dt).requires_grad_(True), w.to(dt).requires_grad_(True)
        y = R.oracle_dwconv3(xr, mask, wr, stride)
        out.append((y.detach(),) + torch.autograd.grad((y * dy.to(dt)).sum(), (xr, wr)))
    return out


# (1, 4098, 64, 3, 2): 2049 output rows, more than one row per wave of the weight gradient's slices (a wave owns ceil(rows / 2048) rows)
DW_CASES = [(2, 72, 32, 3, 1), (2, 72, 32, 3, 2), (1, 1, 64, 3, 1), (1, 2, 256, 1, 2), (3, 8, 256, 3, 2), (4, 63, 288, 3, 1), (2, 200, 1024, 1, 1),
            (3, 1100, 256, 3, 2), (1, 4098, 64, 3, 2)]


@pytest.mark.parametrize('B,T,C,n,stride', DW_CASES)
def test_depthwise_convolution_matches_fp64(lib, B, T, C, n, stride):
    x, w, dy, mask = dw_case(B, T, C, n, stride, seed=T * 3 + C + n + stride)
    (y64, gx64, gw64), (y32, gx32, gw32) = dw_refs(x, mask, w, dy, stride)
    xc, mc, wc, dyc = cu(x, mask, w, dy)
    tag = f'dwconv B{B} T{T} C{C} n{n} s{stride}'
    check(f'{tag} Y', lib.dw(xc, mc, wc, stride), y64, y32)
    dx, dw = lib.dw_bwd(xc, mc, wc, dyc, stride)
    check(f'{tag} dX', dx, gx64, gx32)
    for i in range(n):
        check(f'{tag} dW{i}', dw[i], gw64[i], gw32[i])
    assert bool((dx.cpu()[~mask] == 0).all()), 'dX at a padded row is exactly 0'
    # accumulate: g + g is exact
    _, acc = lib.dw_bwd(xc, mc, wc, dyc, stride, want=(False, True), into=dw.clone())
    assert torch.equal(acc, 2 * dw)
    # a NULL output leaves the other bit-identical
    only_x, none_w = lib.dw_bwd(xc, mc, wc, dyc, stride, want=(True, False))
    none_x, only_w = lib.dw_bwd(xc, mc, wc, dyc, stride, want=(False, True))
    assert none_w is None and none_x is None and torch.equal(only_x, dx) and torch.equal(only_w, dw)
    # NULL mask = every row valid
    (_, gx64, gw64), (_, gx32, gw32) = dw_refs(x, None, w, dy, stride)
    dx, dw = lib.dw_bwd(xc, None, wc, dyc, stride)
    check(f'{tag} dX (NULL mask)', dx, gx64, gx32)
    check(f'{tag} dW (NULL mask)', dw, gw64, gw32)


def seam_inputs(B, T, C, seed):
    """rows next to the sequence seam and one masked row hold values 100 times the rest (positive ones: they win every window)"""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, C, generator=gen)
    mask = torch.ones(B, T, dtype=torch.bool)
    mask[0, 30] = False
    for b, t in ((0, T - 1), (1, 0), (0, 30)):
        x[b, t] = 100 * x[b, t].abs()
    return x, mask, gen


@pytest.mark.parametrize('stride', [1, 2])
def test_depthwise_taps_stop_at_sequence_seams_and_masked_rows(lib, stride):
    B, T, C, n = 2, 64, 64, 3
    x, mask, gen = seam_inputs(B, T, C, seed=5)
    w = torch.randn(n, C, 3, generator=gen)
    dy = torch.randn(n, B, T // stride, C, generator=gen) * 1e-3
    dy[:, 0, -1] *= 100
    dy[:, 1, 0] *= 100
    dy[:, 0, 30 // stride] *= 100
    (_, gx64, gw64), (_, gx32, gw32) = dw_refs(x, mask, w, dy, stride)
    dx, dw = lib.dw_bwd(*cu(x, mask, w, dy), stride)
    bounds = [check(f'seam dwconv s{stride} dX', dx, gx64, gx32), check(f'seam dwconv s{stride} dW', dw, gw64, gw32)]
    xd, dyd, wd = x.double(), dy.double(), w.double()
    wrong_seam = R.dwconv3_grads(xd.reshape(1, B * T, C), mask.reshape(1, B * T), wd, dyd.reshape(n, 1, B * T // stride, C), stride)
    wrong_mask = R.dwconv3_grads(xd, None, wd, dyd, stride)
    for wrong in (wrong_seam, wrong_mask):
        for w_, g_, bound in zip(wrong, (gx64, gw64), bounds):
            assert float((w_.detach().reshape(g_.shape) - g_.detach()).abs().max()) > 100 * bound


# ------------------------------------------------------------------------------------------
# max pooling
# ------------------------------------------------------------------------------------------
def pool_ref32(x, mask, dy):
    """(Y, pooled mask, dX) by fp32 autograd on the CPU through the oracle's masked_max_pool1d"""
    xr = x.clone().requires_grad_(True)
    y, mo = R.oracle_pool(xr, mask)
    return y.detach(), mo, torch.autograd.grad((y * dy).sum(), xr)[0]


def pool_equal(lib, x, mask, dy):
    y32, mo32, gx32 = pool_ref32(x, mask, dy)
    xc, mc, dyc = cu(x, mask, dy)
    y, mo = lib.pool(xc, mc)
    assert torch.equal(mo.cpu().bool(), mo32) and bool((mo <= 1).all())
    assert torch.equal(y.cpu(), y32)
    dx = lib.pool_bwd(xc, mc, dyc).cpu()
    assert torch.equal(dx, gx32)
    return dx


@pytest.mark.parametrize('B,T,C', [(2, 72, 32), (1, 2, 64), (3, 8, 256), (3, 1100, 256)])
def test_pooling_is_bit_identical_to_fp32_autograd(lib, B, T, C):
    gen = torch.Generator().manual_seed(T + C)
    x = torch.randn(B, T, C, generator=gen)
    dy = torch.randn(B, T // 2, C, generator=gen) * 1e-3
    mask = R.holes(B, T, gen)
    dx = pool_equal(lib, x, mask, dy)
    assert bool((dx[~mask] == 0).all())
    pool_equal(lib, x, None, dy)


def test_pooling_tie_rule_and_a_wholly_padded_window(lib):
    """tests/test_enc_grad_cpu.py tie_case: a padded slot in front of the row that holds its channel's minimum inside one window (the
    slot wins, the gradient is lost), equal values inside windows (the lower row wins), a window without a valid row"""
    x, mask = tie_case(torch.float32)
    dy = torch.arange(1, 2 * 6 * 4 + 1, dtype=torch.float32).reshape(2, 6, 4) * 1e-3
    dx = pool_equal(lib, x, mask, dy)
    assert bool((dx[0, 3] == 0).all()) and float(dx[0, 4, 0]) == float(dy[0, 2, 0]) and float(dx[0, 5, 0]) == 0.0
    assert bool((dx[1, 5:8] == 0).all())


def test_pooling_matches_the_reference_backward(lib):
    from conftest import Golden
    g = Golden('enc_grad.npz')
    x, mask, up = R.cm(g.t('pool/x')).contiguous(), g.t('pool/mask'), R.cm(g.t('pool/up')).contiguous()
    xc, mc, upc = cu(x, mask, up)
    y, mo = lib.pool(xc, mc)
    assert torch.equal(R.cm(y.cpu()), g.t('pool/out32')) and torch.equal(mo.cpu().bool(), g.t('pool/mask_out'))
    assert torch.equal(R.cm(lib.pool_bwd(xc, mc, upc).cpu()), g.t('pool/gx32'))


def test_pooling_windows_stop_at_sequence_seams_and_masked_rows(lib):
    B, T, C = 2, 64, 64
    x, mask, gen = seam_inputs(B, T, C, seed=6)
    dy = torch.randn(B, T // 2, C, generator=gen) * 1e-3
    xr = x.double().requires_grad_(True)
    y, _ = R.oracle_pool(xr, mask)
    g64, = torch.autograd.grad((y * dy.double()).sum(), xr)
    _, _, g32 = pool_ref32(x, mask, dy)
    bound = check('seam pool dX', lib.pool_bwd(*cu(x, mask, dy)), g64, g32)
    wrong_seam = R.masked_max_pool_grad(x.double().reshape(1, B * T, C), mask.reshape(1, B * T), dy.double().reshape(1, B * T // 2, C))
    wrong_mask = R.masked_max_pool_grad(x.double(), None, dy.double())
    for wrong in (wrong_seam, wrong_mask):
        assert float((wrong.reshape(B, T, C) - g64).abs().max()) > 100 * bound


# ------------------------------------------------------------------------------------------
# GELU
# ------------------------------------------------------------------------------------------
POINTS = [0.0, 1e-4, -1e-4, 6.0, -6.0, 12.0, -12.0]


@pytest.mark.parametrize('n', [1, 5, 7, 4097, 2 ** 20 + 3])
def test_gelu_matches_fp64(lib, n):
    gen = torch.Generator().manual_seed(n)
    x = 3 * torch.randn(n, generator=gen)
    if n >= len(POINTS):
        x[:len(POINTS)] = torch.tensor(POINTS)             # n = 7: the points alone
    dy = torch.randn(n, generator=gen) * 1e-3
    refs = []
    for dt in (torch.float64, torch.float32):
        xr = x.to(dt).requires_grad_(True)
        y = F.gelu(xr)
        refs.append((y.detach(), torch.autograd.grad((y * dy.to(dt)).sum(), xr)[0]))
    xc, dyc = cu(x, dy)
    check(f'gelu n{n} Y', lib.gelu(xc), refs[0][0], refs[1][0])
    check(f'gelu n{n} dX', lib.gelu_bwd(xc, dyc), refs[0][1], refs[1][1])


# ------------------------------------------------------------------------------------------
# LayerScale residual
# ------------------------------------------------------------------------------------------
def ls_refs(r, h, ls, dy, mr, mh):
    out = []
    for dt in (torch.float64, torch.float32):
        rr, hr, lr = (z.to(dt).requires_grad_(True) for z in (r, h, ls))
        y = R.layerscale_residual(rr, hr, lr, mr, mh)
        out.append((y.detach(),) + torch.autograd.grad((y * dy.to(dt)).sum(), (rr, hr, lr)))
    return out


@pytest.mark.parametrize('C', [32, 256, 288, 1024])
def test_layerscale_residual_matches_fp64(lib, C):
    for rows in (1, 5, 4097):
        gen = torch.Generator().manual_seed(C + rows)
        r, h = torch.randn(1, rows, C, generator=gen), torch.randn(1, rows, C, generator=gen)
        ls = 0.5 + 0.25 * torch.randn(C, generator=gen)
        dy = torch.randn(1, rows, C, generator=gen) * 1e-3
        m = torch.rand(1, rows, generator=gen) > 0.15
        for place, (mr, mh) in (('R', (m, None)), ('H', (None, m)), ('none', (None, None))):
            ref64, ref32 = ls_refs(r, h, ls, dy, mr, mh)
            rc, hc, lc, dyc, mrc, mhc = cu(r, h, ls, dy, mr, mh)
            tag = f'layerscale C{C} rows{rows} mask {place}'
            check(f'{tag} Y', lib.ls(rc, mrc, hc, mhc, lc), ref64[0], ref32[0])
            got = lib.ls_bwd(dyc, hc, mrc, mhc, lc)
            for name, a, b, c in zip(('dR', 'dH', 'dls'), got, ref64[1:], ref32[1:]):
                check(f'{tag} {name}', a, b, c)
            _, _, acc = lib.ls_bwd(dyc, hc, mrc, mhc, lc, want=(False, False, True), into=got[2].clone())
            assert torch.equal(acc, 2 * got[2])
            for skip in range(3):
                part = lib.ls_bwd(dyc, hc, mrc, mhc, lc, want=tuple(i != skip for i in range(3)))
                assert all((part[i] is None) if i == skip else torch.equal(part[i], got[i]) for i in range(3))


# ------------------------------------------------------------------------------------------
# every backward export: bit-identical repeats, power-of-two scaling of the upstream gradient
# ------------------------------------------------------------------------------------------
def backward_runs():
    """name -> (function of the upstream gradient returning the list of gradients, upstream gradient on the device)"""
    B, T, C = 3, 1100, 256
    x, w, dy, mask = dw_case(B, T, C, 3, 2, seed=41)
    xc, mc, wc, dyc = cu(x, mask, w, dy)
    gen = torch.Generator().manual_seed(42)
    dyp = (torch.randn(B, T // 2, C, generator=gen) * 1e-3).cuda()
    xg = (3 * torch.randn(2 ** 20, generator=gen)).clamp_(-8, 8).cuda()     # |x| <= 8: Phi(x) dY 2^-30 stays a normal number
    dyg = (torch.randn(2 ** 20, generator=gen) * 1e-3).cuda()
    h = torch.randn(1, B * T, C, generator=gen).cuda()
    ls = (0.5 + 0.25 * torch.randn(C, generator=gen)).cuda()
    dyl = (torch.randn(1, B * T, C, generator=gen) * 1e-3).cuda()
    ml = mask.reshape(1, B * T).cuda()
    return {
        'dwconv3': (lambda lib, g: list(lib.dw_bwd(xc, mc, wc, g, 2)), dyc),
        'maxpool': (lambda lib, g: [lib.pool_bwd(xc, mc, g)], dyp),
        'gelu': (lambda lib, g: [lib.gelu_bwd(xg, g)], dyg),
        'layerscale': (lambda lib, g: list(lib.ls_bwd(g, h, ml, ml, ls)), dyl),
    }


@pytest.mark.parametrize('name', ['dwconv3', 'maxpool', 'gelu', 'layerscale'])
def test_backward_repeats_and_power_of_two_scaling_are_bit_exact(lib, name):
    run, g = backward_runs()[name]
    first = [z.clone() for z in run(lib, g)]
    assert all(bool(torch.isfinite(z).all()) for z in first)
    for _ in range(9):
        assert all(torch.equal(a, b) for a, b in zip(first, run(lib, g)))
    for s in (2.0 ** -30, 2.0 ** 10):
        assert all(torch.equal(a, b / s) for a, b in zip(first, run(lib, g * s)))


# ------------------------------------------------------------------------------------------
# composition
# ------------------------------------------------------------------------------------------
def make_block(pkg, E, stride, heads, window, sd):
    blk = pkg.modeling.TransformerEncoder(E, stride, heads, window)
    blk.load_state_dict(sd)
    return blk.cuda()


def check_block(tag, blk, x, y, want_y, want_mo, mo, g64, g32):
    """forward rule on the output, equality of the mask, gradient rule on the input gradient and the 27 parameter gradients"""
    (y64, gx64, gp64), (y32, gx32, gp32) = g64, g32
    assert torch.equal(mo.cpu(), want_mo)
    check(f'{tag} out', y, y64, y32)
    check(f'{tag} dX', x.grad, gx64, gx32)
    seen = 0
    for k, p in blk.named_parameters():
        top = float(gp64[ZERO_BY_SYMMETRY[k]].abs().max()) if k in ZERO_BY_SYMMETRY else None
        check(f'{tag} {k}', p.grad, gp64[k].reshape(p.shape), gp32[k].reshape(p.shape), top=top)
        seen += 1
    assert seen == 27


@pytest.mark.parametrize('name', ['s1', 's2'])
def test_transformer_encoder_matches_the_reference_backward(lib, name):
    pkg = lib.pkg
    x, mask, sd, up, stride, heads, window, g = encoder_fixture(name, torch.float32)
    blk = make_block(pkg, x.size(-1), stride, heads, window, sd)
    xc = x.cuda().requires_grad_(True)
    y, mo = pkg.autograd.transformer_encoder(xc, mask.cuda(), blk)
    (y * up.cuda()).sum().backward()
    tm = lambda z: z.transpose(1, 2)
    refs = [(tm(g.t(f'{name}/out{t}')), tm(g.t(f'{name}/gx{t}')), g.sub(f'{name}/gp{t}/')) for t in ('64', '32')]
    check_block(f'encoder {name}', blk, xc, y, None, g.t(f'{name}/mask_out'), mo, *refs)


@pytest.mark.parametrize('stride', [1, 2])
def test_transformer_encoder_matches_the_oracle_at_chain_width(lib, stride):
    """E = 256, 4 heads, window 19 (the widths the chain kernels serve), a hole mask, a non-zero upstream gradient on padded rows"""
    pkg = lib.pkg
    E, heads, window, B, T = 256, 4, 19, 3, 72
    gen = torch.Generator().manual_seed(50 + stride)
    torch.manual_seed(60 + stride)
    blk = pkg.modeling.TransformerEncoder(E, stride, heads, window)
    R.set_block_parameters(blk, gen)
    sd = {k: v.detach().clone() for k, v in blk.state_dict().items()}
    x = torch.randn(B, T, E, generator=gen)
    up = torch.randn(B, T // stride, E, generator=gen)
    mask = R.holes(B, T, gen)
    refs = []
    for dt in (torch.float64, torch.float32):
        y, mo, gx, gp = oracle_encoder_grads(x.to(dt), mask, {k: v.to(dt) for k, v in sd.items()}, up.to(dt), stride, heads, window)
        refs.append((y, gx, gp))
    blk = blk.cuda()
    xc = x.cuda().requires_grad_(True)
    y, got_mo = pkg.autograd.transformer_encoder(xc, mask.cuda(), blk)
    (y * up.cuda()).sum().backward()
    check_block(f'encoder E256 s{stride}', blk, xc, y, None, mo, got_mo, *refs)


def test_needs_input_grad(lib):
    """an input that does not require grad gets None, and the others keep their bits"""
    pkg = lib.pkg
    A = pkg.autograd
    x, mask, sd, up, stride, heads, window, g = encoder_fixture('s2', torch.float32)
    blk = make_block(pkg, x.size(-1), stride, heads, window, sd)
    xc = x.cuda().requires_grad_(True)
    (A.transformer_encoder(xc, mask.cuda(), blk)[0] * up.cuda()).sum().backward()
    full = {k: p.grad.clone() for k, p in blk.named_parameters()}
    frozen = ('attn.k_conv.conv.weight', 'drop_path_ffn.scale', 'ffn.fc.weight', 'ln_attn.weight')
    for k, p in blk.named_parameters():
        p.grad = None
        p.requires_grad_(k not in frozen)
    x2 = x.cuda()
    (A.transformer_encoder(x2, mask.cuda(), blk)[0] * up.cuda()).sum().backward()
    assert x2.grad is None
    for k, p in blk.named_parameters():
        assert (p.grad is None) if k in frozen else torch.equal(p.grad, full[k]), k
    # the operators on their own
    gen = torch.Generator().manual_seed(8)
    z, h = torch.randn(2, 8, 32, generator=gen).cuda(), torch.randn(2, 8, 32, generator=gen).cuda()
    ws = [torch.randn(32, 1, 3, generator=gen).cuda().requires_grad_(True) for _ in range(3)]
    zr = z.clone().requires_grad_(True)
    ys, _ = A.depthwise_conv1d(zr, None, ws, 1)
    sum(y.sum() for y in ys).backward()
    ws2 = [w.detach().clone().requires_grad_(i != 1) for i, w in enumerate(ws)]
    ys, _ = A.depthwise_conv1d(z, None, ws2, 1)
    sum(y.sum() for y in ys).backward()
    assert z.grad is None and ws2[1].grad is None and torch.equal(ws2[0].grad, ws[0].grad) and torch.equal(ws2[2].grad, ws[2].grad)
    ls = torch.randn(1, 32, 1, generator=gen).cuda()
    hr, lr = h.clone().requires_grad_(True), ls.clone().requires_grad_(True)
    A.layer_scale_residual(zr, hr, lr).sum().backward()
    h2 = h.clone().requires_grad_(True)
    A.layer_scale_residual(z, h2, ls).sum().backward()
    assert torch.equal(h2.grad, hr.grad) and lr.grad.shape == ls.shape


def test_blocks_train_through_heads_and_the_point_objective(lib):
    """one stride-1 block, one stride-2 block on its output, the three heads on both levels, the point objective"""
    from test_conv_grad_cpu import fixture_case
    from test_gpu_conv_grad import make_head
    pkg = lib.pkg
    B, T, L, E = 2, 64, 2, 64
    gen = torch.Generator().manual_seed(3)
    torch.manual_seed(4)
    blocks = [pkg.modeling.TransformerEncoder(E, s, 4, 9) for s in (1, 2)]
    for blk in blocks:
        R.set_block_parameters(blk, gen)
        blk.cuda()
    cls1, cls2 = (make_head(pkg, 'cls', fixture_case('cls', torch.float32)[2]) for _ in range(2))
    reg = make_head(pkg, 'reg', fixture_case('reg', torch.float32)[2])
    A = pkg.autograd
    x = torch.randn(B, T, E, generator=gen).cuda()
    mask = (torch.arange(T)[None] < torch.tensor([T, T * 3 // 4])[:, None]).cuda()
    x0, m0 = A.transformer_encoder(x, mask, blocks[0])
    x1, m1 = A.transformer_encoder(x0, m0, blocks[1])
    xs, masks = (x0, x1), (m0, m1)
    outputs = (tuple(A.conv_head(z, m, cls1) for z, m in zip(xs, masks)), tuple(A.conv_head(z, m, cls2) for z, m in zip(xs, masks)),
               tuple(A.conv_head(z, m, reg, level=l) for l, (z, m) in enumerate(zip(xs, masks))), tuple(masks))
    obj = pkg.loss.PointObjective(pkg.config.make_opt(n_levels=L, max_seq_len=T))
    total = obj(outputs, torch.tensor([[10.0, 30.5], [3.0, 20.0]]).cuda())['total']
    assert bool(torch.isfinite(total))
    total.backward()
    for i, blk in enumerate(blocks):
        seen = 0
        for k, p in blk.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, (i, k)
            seen += 1
        assert seen == 27


def test_unsupported_blocks_and_shapes_are_refused(lib):
    pkg = lib.pkg
    A, M = pkg.autograd, pkg.modeling
    z = torch.zeros(1, 8, 32).cuda()
    with pytest.raises(ValueError, match='stride'):
        A.transformer_encoder(z, None, M.TransformerEncoder(32, 0, 4, 0).cuda())
    with pytest.raises(ValueError, match='global attention'):
        A.transformer_encoder(z, None, M.TransformerEncoder(32, 1, 4, 0).cuda())
    with pytest.raises(ValueError, match='multiple of the stride'):
        A.transformer_encoder(torch.zeros(1, 7, 32).cuda(), None, M.TransformerEncoder(32, 2, 4, 9).cuda())
    l, L = lib.l, lib.L
    y = torch.zeros(3, 1, 7, 32).cuda()
    assert L.dcf_op_dwconv3(l.ptr(z), None, l.ptr(y), l.ptr(y), 1, 7, 32, 3, 2, l.current_stream()) != 0
    assert b'multiple of the stride' in L.dcf_last_error()
    assert L.dcf_op_masked_maxpool(l.ptr(z), None, l.ptr(y), None, 1, 7, 32, l.current_stream()) != 0
    assert L.dcf_op_layerscale_residual(l.ptr(z), None, l.ptr(z), None, l.ptr(z), l.ptr(y), 8, 30, l.current_stream()) != 0
    assert b'multiple of 4' in L.dcf_last_error()
