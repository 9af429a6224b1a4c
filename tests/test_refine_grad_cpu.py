"""CPU checks around csrc/refine_grad.hip and autograd.refine_in / tcn_layer / tcn / fuse_and_predict: the closed forms of
tests/refine_grad_ref.py against fp64 autograd through the oracle's `tcn_refine`, the oracle under fp64 autograd against the reference's
own `fuse_and_predict` (tests/golden/refine_grad*.npz, make_golden_refine_grad.py), the fixture's fp32 gradients against its fp64 ones
by the project's gradient rule, one dropout case, and the presence of the exports and of the autograd functions.  No GPU.

The closed forms meet the oracle in two ways.  A single layer of dilation 1: a one-layer `tcn_refine` whose conv_1x1 and conv_out are
the identity is the layer times the mask.  Every dilation, the in-map and the stacking: the whole TCN chained from the closed forms
(refine_in -> layers of dilation 2^i -> conv_out * mask, and its backward chained in reverse) against autograd through `tcn_refine` on
the stacked input; a wrong gradient of any part shows in that part's parameter gradient.

The gradient rule, per tensor: e <= max(4 e_ref, 2^-21 max |g_64|) (tests/test_dec_grad_cpu.py)."""
import ctypes
import re

import pytest
import torch

from conftest import load_pkg
import refine_grad_ref as R
from test_abi import HEADER

EXPORTS = ('dcf_op_refine_in', 'dcf_op_refine_in_bwd', 'dcf_op_tcn_layer', 'dcf_op_tcn_layer_bwd')
FLOOR = 2.0 ** -21
TOL = 1e-10


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


def random_tcn(L, gen, dtype):
    r = lambda *s: torch.randn(*s, generator=gen)
    sd = {'refine.conv_1x1.weight': r(R.C, L, 1) / L ** 0.5, 'refine.conv_1x1.bias': 0.1 * r(R.C),
          'refine.conv_out.weight': r(R.C, R.C, 1) / 32 ** 0.5, 'refine.conv_out.bias': 0.1 * r(R.C)}
    for i in range(L):
        sd.update({f'refine.layers.{i}.{k}': v for k, v in zip(R.LAYER_PARAMS, R.random_layer(gen))})
    return {k: v.to(dtype) for k, v in sd.items()}


@pytest.mark.parametrize('masked', [True, False])
def test_layer_closed_forms_equal_autograd_through_the_oracle(masked):
    gen = torch.Generator().manual_seed(5 + masked)
    B, T0 = 3, 13
    P = R.random_layer(gen, torch.float64)
    x, dy = (torch.randn(B, T0, R.C, dtype=torch.float64, generator=gen) for _ in range(2))
    mask = R.tail_mask(B, T0, gen) if masked else None
    mf = 1.0 if mask is None else mask[..., None].double()
    xr = x.clone().requires_grad_(True)
    Pr = tuple(t.clone().requires_grad_(True) for t in P)
    y = R.oracle_layer(Pr, xr, mask)                                  # = layer(x) * mask
    assert rel(R.tcn_layer(x, mask, P, 1) * mf, y) <= TOL
    want = torch.autograd.grad((y * dy).sum(), (xr,) + Pr)
    got = R.tcn_layer_grads(x, mask, P, 1, dy * mf)
    for name, a, b in zip(R.GRAD_NAMES, got, want):
        assert rel(a, b) <= TOL, name
    if masked:
        full = R.tcn_layer_grads(x, mask, P, 1, dy)                   # dY at padded rows too
        assert float(full[0][~mask].abs().max()) > 0, 'dX is not zero at padded rows: neighbours read them through the side taps'
        assert torch.allclose(full[6], dy.sum((0, 1))), 'dln_b takes dY at padded rows'
        assert float((full[6] - got[6]).abs().max()) > 0


@pytest.mark.parametrize('B,T0,L,masked', [(3, 40, 3, True), (2, 4, 3, True), (1, 16, 1, False), (2, 32, 5, True)])
def test_tcn_closed_forms_equal_autograd_through_the_oracle(B, T0, L, masked):
    """(2, 4, 3): the last layer's dilation equals T0, only its centre tap lands; (2, 32, 5): dilations up to 16"""
    gen = torch.Generator().manual_seed(T0 + L)
    sd = random_tcn(L, gen, torch.float64)
    S = sum(R.sizes(T0, L))
    lg, dout = torch.randn(B, S, dtype=torch.float64, generator=gen), torch.randn(B, T0, R.C, dtype=torch.float64, generator=gen)
    mask = R.tail_mask(B, T0, gen) if masked else None
    lr = lg.clone().requires_grad_(True)
    sr = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    out = R.oracle_tcn(sr, R.stack(lr, mask, T0, L), mask, L)
    assert rel(R.tcn(lg, mask, sd, T0, L)[0], out) <= TOL
    (out * dout).sum().backward()
    dl, gp = R.tcn_grads(lg, mask, sd, T0, L, dout)
    assert rel(dl, lr.grad) <= TOL
    assert sorted(gp) == sorted(sd)
    for k, v in gp.items():
        assert v.shape == sd[k].shape and rel(v, sr[k].grad) <= TOL, k


def test_dropout_case_follows_the_philox_mask():
    """p = 0.5, b0 = 1: the closed forms with the keep mask of tests/philox_ref.py against fp64 autograd through the same forward; the
    mask is the training forward's (site refine layer 2, element ((b0 + b) * 32 + c) * T0 + t), half of it is dropped, and a dropped
    element passes no gradient to conv_1x1"""
    gen = torch.Generator().manual_seed(9)
    B, T0, dil, layer, drop = 2, 24, 4, 2, (0x1234567890ABCDEF, 0.5, 1)
    P = R.random_layer(gen, torch.float64)
    x, dy = (torch.randn(B, T0, R.C, dtype=torch.float64, generator=gen) for _ in range(2))
    mask = R.tail_mask(B, T0, gen)
    ks = R.keep_scale(drop, layer, B, T0)
    assert ks.shape == (B, T0, R.C) and set(ks.unique().tolist()) == {0.0, 2.0}
    assert 0.4 < float((ks == 0).float().mean()) < 0.6
    e = ((1 + 1) * R.C + 7) * T0 + 5
    assert bool(ks[1, 5, 7] > 0) == bool(R.PH.keep(drop[0], R.PH.site(R.PH.G_REFINE, layer, R.PH.TCN), [e], 0.5)[0])
    xr = x.clone().requires_grad_(True)
    Pr = tuple(t.clone().requires_grad_(True) for t in P)
    y = R.tcn_layer(xr, mask, Pr, dil, ks)
    want = torch.autograd.grad((y * dy).sum(), (xr,) + Pr)
    got = R.tcn_layer_grads(x, mask, P, dil, dy, ks)
    for name, a, b in zip(R.GRAD_NAMES, got, want):
        assert rel(a, b) <= TOL, name
    assert not torch.equal(y.detach(), R.tcn_layer(x, mask, P, dil)), 'the mask changes the forward'
    assert R.keep_scale((drop[0], 0.0, 1), layer, B, T0) is None, 'p = 0 is the identity'


def test_oracle_reproduces_the_reference_backward_in_fp64():
    f = R.Fixture(torch.float64)
    outs, gfpn, gp = f.oracle_grads()
    for k, v in outs.items():
        for l in range(f.L):
            assert rel(v[l], f.out['64'][k][l]) <= 1e-9, (k, l)
    for l in range(f.L):
        assert rel(gfpn[l], f.gfpn['64'][l]) <= 1e-9, l
    assert sorted(gp) == sorted(f.gp['64'])
    for k, got in gp.items():
        assert rel(got, f.gp['64'][k]) <= 1e-9, k


def test_fixture_fp32_gradients_are_what_the_gpu_tests_take_for_e_ref():
    """the reference's fp32 `backward()` is an fp32-class result (within 2^-17 max |g_64| of the fp64 one), and fp32 autograd through the
    oracle, a second fp32 evaluation of the same function, passes the rule against it"""
    f = R.Fixture(torch.float32)
    outs, gfpn, gp = f.oracle_grads()
    tensors = [(f'{k}/l{l}', f.out['32'][k][l], f.out['64'][k][l], outs[k][l]) for k in outs for l in range(f.L)]
    tensors += [(f'gfpn/l{l}', f.gfpn['32'][l], f.gfpn['64'][l], gfpn[l]) for l in range(f.L)]
    tensors += [(k, f.gp['32'][k], f.gp['64'][k], gp[k]) for k in gp]
    for tag, g32, g64, mine in tensors:
        assert g32.dtype == torch.float32 and g64.dtype == torch.float64, tag
        top, e_ref = float(g64.abs().max()), float((g32.double() - g64).abs().max())
        assert e_ref <= 2.0 ** -17 * top, (tag, e_ref, top)
        assert float((mine.double() - g64).abs().max()) <= max(4 * e_ref, FLOOR * top), tag


def test_exports_are_declared_built_and_bound():
    pkg = load_pkg()
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    h = ctypes.CDLL(pkg.build.build())
    for name in EXPORTS:
        assert re.search(r'\bint\s+' + name + r'\s*\(', src), f'{name} is not declared in the header'
        assert hasattr(h, name), f'{name} is not exported by the library'
        assert name in pkg._lib.SIGNATURES
    assert h.dcf_abi_version() == 12
    for name in ('refine_in', 'tcn_layer', 'tcn', 'fuse_and_predict'):
        assert callable(getattr(pkg.autograd, name)), name
    assert 'refinement TCN and the gate' not in pkg.autograd.__doc__


def test_autograd_functions_refuse_the_cpu_and_bad_shapes():
    pkg = load_pkg()
    A, M = pkg.autograd, pkg.modeling
    net = M.TCN(3, 32, 32, 3)
    x, lg, m = torch.zeros(1, 8, 32), torch.zeros(1, 14), torch.ones(1, 8, dtype=torch.bool)
    for call in (lambda: A.refine_in(lg, m, net), lambda: A.tcn_layer(x, m, net.layers[0], 1), lambda: A.tcn(lg, m, net)):
        with pytest.raises(RuntimeError, match='GPU'):
            call()
    f = R.Fixture(torch.float32)
    model = M.PtTransformerEarlyFusionIterative(pkg.config.make_opt(**f.opt_kwargs), second_fusion=False)
    with pytest.raises(RuntimeError, match='GPU'):
        A.fuse_and_predict(f.fpn, f.masks, model)
    with pytest.raises(ValueError, match='levels'):
        A.fuse_and_predict(f.fpn[:2], f.masks[:2], model)
    with pytest.raises(ValueError, match='dropout p'):
        A.tcn_layer(x, m, net.layers[0], 1, dropout=(1, 1.0, 0))
    with pytest.raises(ValueError, match='site_layer'):
        A.tcn_layer(x, m, net.layers[0], 3, dropout=(1, 0.5, 0))
