"""CPU checks around the operator pairs of csrc/enc_grad.hip and autograd.transformer_encoder: the closed forms of
tests/enc_grad_ref.py against fp64 autograd through the oracle's functions, the oracle's transformer_encoder under fp64 autograd
against the reference's own module (tests/golden/enc_grad.npz, make_golden_enc_grad.py), and the presence of the exports and of the
autograd functions.  No GPU."""
import ctypes
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import Golden, load_pkg
import enc_grad_ref as R
from test_abi import HEADER

EXPORTS = ('dcf_op_dwconv3', 'dcf_op_dwconv3_bwd', 'dcf_op_masked_maxpool', 'dcf_op_masked_maxpool_bwd', 'dcf_op_gelu', 'dcf_op_gelu_bwd',
           'dcf_op_layerscale_residual', 'dcf_op_layerscale_residual_bwd')
FIXTURE = 'enc_grad.npz'
ZERO_BY_SYMMETRY = {'attn.k_norm.bias': 'attn.k_norm.weight', 'attn.attn.key.bias': 'attn.attn.key.weight'}


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


def mask_of(kind, B, T, gen):
    if kind == 'holes':
        return R.holes(B, T, gen)
    if kind == 'tail':
        m = torch.ones(B, T, dtype=torch.bool)
        m[-1, T - T // 3:] = False
        return m
    return None


@pytest.mark.parametrize('B,T,C,n,stride,kind', [(2, 24, 8, 3, 1, 'holes'), (2, 24, 8, 3, 2, 'holes'), (3, 10, 4, 1, 2, 'tail'), (1, 1, 4, 3, 1, 'none'),
                                                  (1, 2, 8, 1, 2, 'none'), (2, 7, 4, 2, 1, 'holes'), (4, 16, 12, 3, 2, 'holes')])
def test_depthwise_closed_forms_equal_autograd_through_the_oracle(B, T, C, n, stride, kind):
    gen = torch.Generator().manual_seed(T * 7 + C + stride)
    x = torch.randn(B, T, C, dtype=torch.float64, generator=gen)
    w = torch.randn(n, C, 3, dtype=torch.float64, generator=gen)
    dy = torch.randn(n, B, T // stride, C, dtype=torch.float64, generator=gen)
    mask = mask_of(kind, B, T, gen)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = R.oracle_dwconv3(xr, mask, wr, stride)
    assert rel(R.dwconv3(x, mask, w, stride), y) <= 1e-12
    gx, gw = torch.autograd.grad((y * dy).sum(), (xr, wr))
    dx, dw = R.dwconv3_grads(x, mask, w, dy, stride)
    assert rel(dx, gx) <= 1e-12 and rel(dw, gw) <= 1e-12
    if mask is not None:
        assert bool((dx[~mask] == 0).all()) and bool((gx[~mask] == 0).all())


@pytest.mark.parametrize('B,T,C,kind', [(2, 24, 8, 'holes'), (3, 10, 4, 'tail'), (1, 2, 4, 'none'), (4, 16, 12, 'holes'), (2, 72, 16, 'holes')])
def test_pooling_closed_forms_equal_autograd_through_the_oracle(B, T, C, kind):
    gen = torch.Generator().manual_seed(T * 5 + C)
    x = torch.randn(B, T, C, dtype=torch.float64, generator=gen)
    dy = torch.randn(B, T // 2, C, dtype=torch.float64, generator=gen)
    mask = mask_of(kind, B, T, gen)
    xr = x.clone().requires_grad_(True)
    y, mo = R.oracle_pool(xr, mask)
    got, gmo = R.masked_max_pool(x, mask)
    assert torch.equal(got, y.detach()) and torch.equal(gmo, mo)
    gx, = torch.autograd.grad((y * dy).sum(), xr)
    assert torch.equal(R.masked_max_pool_grad(x, mask, dy), gx)


def tie_case(dtype):
    """sequence 0: padded slots 1, 2 in front of row 3, which holds the minimum of every channel -- window 1 (slots 1, 2, 3) is a
    three-way tie that the padded slot 1 wins; rows 4, 5 and 8, 9 hold equal values inside windows 2 and 4 / 5 (the lower row wins);
    sequence 1: window 3 (slots 5, 6, 7) is padded as a whole"""
    x = torch.tensor([[0., 1., 5., -3., 2., 2., 3., 1., 4., 4., -1., 0.], [1., 0., 3., 3., 3., 9., 9., 9., -2., 0., 5., 5.]], dtype=dtype)
    x = torch.stack([x, x.flip(0) * 0.5 - 0.25, x + 1.0, -x.abs()], dim=-1)            # (2, 12, 4)
    x[0, 3] = -10.0
    mask = torch.ones(2, 12, dtype=torch.bool)
    mask[0, [1, 2]] = False
    mask[1, [5, 6, 7]] = False
    return x, mask


def test_pooling_tie_rule_on_a_constructed_tie():
    x, mask = tie_case(torch.float64)
    dy = torch.arange(1, 2 * 6 * 4 + 1, dtype=torch.float64).reshape(2, 6, 4)
    xr = x.clone().requires_grad_(True)
    y, mo = R.oracle_pool(xr, mask)
    gx, = torch.autograd.grad((y * dy).sum(), xr)
    got = R.masked_max_pool_grad(x, mask, dy)
    assert torch.equal(got, gx)
    assert bool((got[0, 3] == 0).all()), 'the padded slot in front of the minimum wins the tie and swallows the gradient'
    assert bool((got[0, 4, 0] == dy[0, 2, 0])) and float(got[0, 5, 0]) == 0.0, 'rows 4, 5 tie in window 2 (slots 3, 4, 5): row 4 wins'
    assert not bool(mo[1, 3]) and bool((got[1, 5:8] == 0).all())
    # what the attached minimum would do instead: the gradient of window 1 reaches row 3
    y2, _ = R.O.masked_max_pool1d(R.cm(xr), mask[:, None], 3, 2)
    gx2, = torch.autograd.grad((R.cm(y2) * dy).sum(), xr)
    assert float(gx2[0, 3].abs().max()) > 0


def test_pooling_restatement_reproduces_the_reference_backward():
    g = Golden(FIXTURE)
    for tag, dt in (('32', torch.float32), ('64', torch.float64)):
        x, mask, up = R.cm(g.t('pool/x')).to(dt), g.t('pool/mask'), R.cm(g.t('pool/up')).to(dt)
        y, mo = R.masked_max_pool(x, mask)
        assert torch.equal(R.cm(y), g.t(f'pool/out{tag}')) and torch.equal(mo, g.t('pool/mask_out'))
        assert torch.equal(R.cm(R.masked_max_pool_grad(x, mask, up)), g.t(f'pool/gx{tag}'))
        xr = x.clone().requires_grad_(True)
        yo, _ = R.oracle_pool(xr, mask)
        assert torch.equal(R.cm(torch.autograd.grad((yo * up).sum(), xr)[0]), g.t(f'pool/gx{tag}'))
    assert float(g.t('pool/gx64')[0, :, 3].abs().max()) == 0.0, 'the fixture holds the swallowed gradient (detached fill, lowest position)'


def test_gelu_and_layerscale_closed_forms_equal_autograd():
    gen = torch.Generator().manual_seed(9)
    x = torch.cat([3 * torch.randn(500, dtype=torch.float64, generator=gen), torch.tensor([0., 1e-4, -1e-4, 6., -6., 12., -12.], dtype=torch.float64)])
    dy = torch.randn(x.shape, dtype=torch.float64, generator=gen)
    xr = x.clone().requires_grad_(True)
    y = F.gelu(xr)
    assert float((R.gelu(x) - y).abs().max()) <= 1e-12 * float(y.abs().max())
    gx, = torch.autograd.grad((y * dy).sum(), xr)
    assert rel(R.gelu_grad(x, dy), gx) <= 1e-12
    B, T, C = 3, 9, 8
    r, h, dyy = (torch.randn(B, T, C, dtype=torch.float64, generator=gen) for _ in range(3))
    ls = torch.randn(C, dtype=torch.float64, generator=gen)
    m = R.holes(B, T, gen)
    for mr, mh in ((m, None), (None, m), (None, None)):
        rr, hr, lr = (z.clone().requires_grad_(True) for z in (r, h, ls))
        one = torch.ones(B, T, 1, dtype=torch.float64)
        y = rr * (one if mr is None else mr[..., None].double()) + lr * (hr * (one if mh is None else mh[..., None].double()))
        assert rel(R.layerscale_residual(r, h, ls, mr, mh), y) <= 1e-12
        want = torch.autograd.grad((y * dyy).sum(), (rr, hr, lr))
        for a, b in zip(R.layerscale_residual_grads(dyy, h, ls, mr, mh), want):
            assert rel(a, b) <= 1e-12


def encoder_fixture(name, dtype):
    """(x token-major, mask, state dict, upstream gradient token-major, stride, heads, window, fixture) of case `name`"""
    g = Golden(FIXTURE)
    meta = g.js('meta')
    tm = lambda z: z.transpose(1, 2).contiguous().to(dtype)
    sd = {k: v.to(dtype) for k, v in g.sub('param/').items()}
    return tm(g.t(f'{name}/x')), g.t(f'{name}/mask'), sd, tm(g.t(f'{name}/up')), meta['cases'][name], meta['heads'], meta['window'], g


def oracle_encoder_grads(x, mask, sd, up, stride, heads, window):
    """(output, mask_out, input gradient, {parameter: gradient}) by autograd through the oracle's transformer_encoder, in the dtype of
    the operands"""
    x = x.detach().clone().requires_grad_(True)
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    y, mo = R.oracle_encoder(sd, x, mask, stride, heads, window)
    (y * up).sum().backward()
    return y.detach(), mo, x.grad, {k: v.grad for k, v in sd.items()}


@pytest.mark.parametrize('name', ['s1', 's2'])
def test_oracle_encoder_reproduces_the_reference_backward_in_fp64(name):
    x, mask, sd, up, stride, heads, window, g = encoder_fixture(name, torch.float64)
    y, mo, gx, gp = oracle_encoder_grads(x, mask, sd, up, stride, heads, window)
    assert torch.equal(mo, g.t(f'{name}/mask_out'))
    assert rel(y.transpose(1, 2), g.t(f'{name}/out64')) <= 1e-9
    assert rel(gx.transpose(1, 2), g.t(f'{name}/gx64')) <= 1e-9
    assert len(gp) == 27
    for k, got in gp.items():
        want = g.t(f'{name}/gp64/{k}')
        if k in ZERO_BY_SYMMETRY:
            # a constant added to every key moves all scores of a row alike: these two gradients are 0 in exact arithmetic and the
            # fixture holds the reference's rounding noise (1e-16), so the error is measured against the terms that cancel (the weight's)
            assert float((got - want).abs().max()) <= 1e-9 * float(g.t(f'{name}/gp64/{ZERO_BY_SYMMETRY[k]}').abs().max()), k
        else:
            assert rel(got, want) <= 1e-9, k


def test_exports_are_declared_built_and_bound():
    pkg = load_pkg()
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    h = ctypes.CDLL(pkg.build.build())
    for name in EXPORTS:
        assert re.search(r'\bint\s+' + name + r'\s*\(', src), f'{name} is not declared in the header'
        assert hasattr(h, name), f'{name} is not exported by the library'
        assert name in pkg._lib.SIGNATURES
    assert h.dcf_abi_version() == 12
    for name in ('depthwise_conv1d', 'masked_max_pool1d', 'gelu', 'layer_scale_residual', 'ffn', 'conv_attn_layer', 'transformer_encoder'):
        assert callable(getattr(pkg.autograd, name)), name


def test_autograd_functions_refuse_the_cpu_and_the_text_encoder_blocks():
    pkg = load_pkg()
    A, M = pkg.autograd, pkg.modeling
    z = torch.zeros(1, 4, 32)
    blk = M.TransformerEncoder(32, 1, 4, 9)
    for call in (lambda: A.depthwise_conv1d(z, None, [blk.attn.q_conv.conv.weight], 1), lambda: A.masked_max_pool1d(z, None), lambda: A.gelu(z),
                 lambda: A.layer_scale_residual(z, z, blk.drop_path_ffn.scale), lambda: A.ffn(z, blk.ffn), lambda: A.transformer_encoder(z, None, blk)):
        with pytest.raises(RuntimeError, match='GPU'):
            call()
    with pytest.raises(ValueError, match='stride'):
        A.transformer_encoder(z, None, M.TransformerEncoder(32, 0, 4, 0))
    with pytest.raises(ValueError, match='global attention'):
        A.transformer_encoder(z, None, M.TransformerEncoder(32, 1, 4, 0))
    with pytest.raises(ValueError, match='multiple of the stride'):
        A.transformer_encoder(torch.zeros(1, 5, 32), None, M.TransformerEncoder(32, 2, 4, 9))
