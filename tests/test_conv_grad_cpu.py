"""CPU checks around the backward of MaskedConv1D / channel LayerNorm (csrc/conv_grad.hip): the fp64 restatement
tests/conv_grad_ref.py against the reference's own heads (tests/golden/head_grad*.npz, make_golden_head_grad.py), against finite
differences, and the presence of the three exports.  No GPU."""
import ctypes
import re

import pytest
import torch

from conftest import Golden, load_pkg
import conv_grad_ref as R
from test_abi import HEADER

EXPORTS = ('dcf_op_conv_bwd_data', 'dcf_op_conv_bwd_weight', 'dcf_op_layernorm_bwd')
FIXTURES = {'cls': 'head_grad.npz', 'reg': 'head_grad_reg.npz'}


def fixture_case(name, dtype):
    """(xs token-major, masks, params, upstream gradients, fixture) of head `name` in `dtype`"""
    g0, g = Golden(FIXTURES['cls']), Golden(FIXTURES[name])
    n = len([k for k in g0.keys() if k.startswith('x/')])
    xs = [g0.t(f'x/l{i}').transpose(1, 2).contiguous().to(dtype) for i in range(n)]
    masks = [g0.t(f'mask/l{i}') for i in range(n)]
    params = {k: v.to(dtype) for k, v in g.sub(f'{name}/param/').items()}
    ups = [g.t(f'{name}/up/l{i}').to(dtype) for i in range(n)]
    return xs, masks, params, ups, g


def rel(a, b):
    return float((a.detach().double() - b.double()).abs().max()) / max(float(b.double().abs().max()), 1e-300)


@pytest.mark.parametrize('name', ['cls', 'reg'])
def test_restatement_reproduces_the_reference_heads_in_fp64(name):
    xs, masks, params, ups, g = fixture_case(name, torch.float64)
    xs = [x.requires_grad_(True) for x in xs]
    params = {k: v.requires_grad_(True) for k, v in params.items()}
    outs = [R.head(x, m, params, level=i) for i, (x, m) in enumerate(zip(xs, masks))]
    sum((o * u).sum() for o, u in zip(outs, ups)).backward()
    for i, (o, x) in enumerate(zip(outs, xs)):
        assert rel(o, g.t(f'{name}/out64/l{i}')) <= 1e-12
        assert rel(x.grad.transpose(1, 2), g.t(f'{name}/gx64/l{i}')) <= 1e-12
    seen = 0
    for k, p in params.items():
        if f'{name}/gp64/{k}' in g:
            assert rel(p.grad, g.t(f'{name}/gp64/{k}')) <= 1e-12, k
            seen += 1
    assert seen >= 7


@pytest.mark.parametrize('k', [1, 3])
def test_restatement_passes_finite_differences(k):
    gen = torch.Generator().manual_seed(k)
    B, T, C, N = 2, 5, 4, 3
    x = torch.randn(B, T, C, dtype=torch.float64, generator=gen, requires_grad=True)
    w = torch.randn(N, C, k, dtype=torch.float64, generator=gen, requires_grad=True)
    b = torch.randn(N, dtype=torch.float64, generator=gen, requires_grad=True)
    mask = torch.tensor([[1, 1, 0, 1, 1], [1, 1, 1, 0, 0]], dtype=torch.bool)
    assert torch.autograd.gradcheck(lambda x_, w_, b_: R.conv(x_, mask, w_, b_), (x, w, b))
    lw = torch.randn(C, dtype=torch.float64, generator=gen, requires_grad=True)
    lb = torch.randn(C, dtype=torch.float64, generator=gen, requires_grad=True)
    assert torch.autograd.gradcheck(lambda x_, w_, b_: R.layer_norm(x_, w_, b_), (x, lw, lb))
    # the closed forms (what the kernels compute) are the autograd gradients of the same expressions
    dy = torch.randn(B, T, N, dtype=torch.float64, generator=gen)
    want = torch.autograd.grad((R.conv(x, mask, w, b) * dy).sum(), (x, w, b))
    for got, ref in zip(R.conv_grads(x.detach(), mask, w.detach(), dy), want):
        assert rel(got, ref) <= 1e-13
    for relu in (False, True):
        do = torch.randn(B, T, C, dtype=torch.float64, generator=gen)
        want = torch.autograd.grad((R.layer_norm(x, lw, lb, relu) * do).sum(), (x, lw, lb))
        for got, ref in zip(R.layer_norm_grads(x.detach(), lw.detach(), lb.detach(), do, relu), want):
            assert rel(got, ref) <= 1e-12


def test_exports_are_declared_built_and_bound():
    pkg = load_pkg()
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    h = ctypes.CDLL(pkg.build.build())
    for name in EXPORTS:
        assert re.search(r'\bint\s+' + name + r'\s*\(', src), f'{name} is not declared in the header'
        assert hasattr(h, name), f'{name} is not exported by the library'
        assert name in pkg._lib.SIGNATURES
    assert h.dcf_abi_version() == 12
    assert callable(pkg.autograd.masked_conv1d) and callable(pkg.autograd.channel_layer_norm) and callable(pkg.autograd.conv_head)


def test_autograd_functions_have_no_cpu_path():
    pkg = load_pkg()
    with pytest.raises(RuntimeError, match='GPU'):
        pkg.autograd.masked_conv1d(torch.zeros(1, 4, 32), None, torch.zeros(32, 32, 3))
    with pytest.raises(RuntimeError, match='GPU'):
        pkg.autograd.channel_layer_norm(torch.zeros(1, 4, 32), torch.ones(32), torch.zeros(32))
