"""CPU checks around the backward of the sliding-window attention core (csrc/attn_grad.hip): the closed forms of
tests/attn_grad_ref.py against fp64 autograd through the oracle's banded attention and against finite differences, the MaskedMHA
restatement against the reference's own module (tests/golden/attn_grad.npz, make_golden_attn_grad.py), and the presence of the
export and of the autograd functions.  No GPU."""
import ctypes
import re
import sys

import pytest
import torch

from conftest import Golden, ROOT, load_pkg
import attn_grad_ref as R
from test_abi import HEADER

sys.path.insert(0, ROOT)
from oracle import decafnet_ref as O  # noqa: E402

EXPORTS = ('dcf_op_local_attn_bwd',)
FIXTURE = 'attn_grad.npz'


def rel(a, b):
    return float((a.detach().double() - b.double()).abs().max()) / max(float(b.double().abs().max()), 1e-300)


def banded(q, k, v, mask, heads, window):
    """the oracle's banded attention on token-major (B, T, C) tensors (how tests/test_gpu_ops.py::test_local_attn_core calls it)"""
    B, T, C = q.shape
    d = C // heads
    s = d ** -0.25

    def split(z):
        return z.reshape(B, T, heads, d).permute(0, 2, 1, 3).reshape(B * heads, T, d)

    mask = torch.ones(B, T, dtype=torch.bool) if mask is None else mask
    out = O.banded_attention(split(q) * s, split(k) * s, split(v), mask, window)
    return out.view(B, heads, T, d).permute(0, 2, 1, 3).reshape(B, T, C)


def banded_grads(q, k, v, mask, dO, heads, window):
    """(dQ, dK, dV) by autograd through the oracle, in the dtype of the operands"""
    q, k, v = (z.detach().clone().requires_grad_(True) for z in (q, k, v))
    return torch.autograd.grad((banded(q, k, v, mask, heads, window) * dO).sum(), (q, k, v))


def holes(B, T, gen):
    """tests/test_gpu_conv_grad.py holes(): single invalid rows inside every sequence, a fully padded tail in the odd sequences"""
    m = torch.rand(B, T, generator=gen) > 0.15
    for b in range(1, B, 2):
        m[b, T - T // 4:] = False
    return m


def mha_fixture(name, dtype):
    """(x token-major, mask, state dict, upstream gradient token-major, heads, window, fixture) of case `name`"""
    g = Golden(FIXTURE)
    meta = g.js('meta')
    tm = lambda z: z.transpose(1, 2).contiguous().to(dtype)
    sd = {k: v.to(dtype) for k, v in g.sub('param/').items()}
    return tm(g.t(f'{name}/x')), g.t(f'{name}/mask'), sd, tm(g.t(f'{name}/up')), meta['heads'], meta['cases'][name]['window'], g


@pytest.mark.parametrize('B,T,C,heads,window,kind', [(2, 24, 16, 2, 5, 'holes'), (2, 40, 32, 4, 9, 'holes'), (3, 50, 16, 2, 19, 'holes'),
                                                      (2, 30, 16, 4, 9, 'tail'), (2, 1, 16, 2, 9, 'none'), (2, 4, 16, 2, 9, 'holes'),
                                                      (1, 11, 8, 1, 19, 'tail'), (2, 3, 8, 2, 5, 'none')])
def test_closed_forms_equal_autograd_through_the_banded_oracle(B, T, C, heads, window, kind):
    gen = torch.Generator().manual_seed(T * 31 + window)
    q, k, v, dO = (torch.randn(B, T, C, dtype=torch.float64, generator=gen) for _ in range(4))
    mask = None
    if kind == 'holes':
        mask = holes(B, T, gen)
    elif kind == 'tail':
        mask = torch.ones(B, T, dtype=torch.bool)
        mask[-1, T - T // 3:] = False
    assert rel(R.window_attention(q, k, v, mask, heads, window), banded(q, k, v, mask, heads, window)) <= 1e-12
    want = banded_grads(q, k, v, mask, dO, heads, window)
    got = R.window_attention_grads(q, k, v, mask, dO, heads, window)
    for name, a, b in zip('QKV', got, want):
        assert rel(a, b) <= 1e-12, name
    if mask is not None:                                   # exact zeros at padded rows, in the closed forms and in autograd alike
        for a, b in zip(got, want):
            assert bool((a[~mask] == 0).all()) and bool((b[~mask] == 0).all())


def test_restatement_passes_finite_differences():
    gen = torch.Generator().manual_seed(6)
    B, T, d, window = 2, 6, 4, 5
    q, k, v = (torch.randn(B, T, d, dtype=torch.float64, generator=gen, requires_grad=True) for _ in range(3))
    mask = torch.ones(B, T, dtype=torch.bool)
    mask[1, 2] = False
    assert torch.autograd.gradcheck(lambda q_, k_, v_: R.window_attention(q_, k_, v_, mask, 1, window), (q, k, v))


@pytest.mark.parametrize('name', ['w9', 'w19'])
def test_restatement_reproduces_the_reference_mha_in_fp64(name):
    x, mask, sd, up, heads, window, g = mha_fixture(name, torch.float64)
    x = x.requires_grad_(True)
    sd = {k: v.requires_grad_(True) for k, v in sd.items()}
    out = R.masked_mha(x, x, x, mask, sd, heads, window)
    (out * up).sum().backward()
    assert rel(out.transpose(1, 2), g.t(f'{name}/out64')) <= 1e-12
    assert rel(x.grad.transpose(1, 2), g.t(f'{name}/gx64')) <= 1e-12
    assert len(sd) == 8
    for k, p in sd.items():
        want = g.t(f'{name}/gp64/{k}')
        if k == 'key.bias':
            # a constant added to every key moves all scores of a row alike: this gradient is 0 in exact arithmetic and the fixture
            # holds the reference's rounding noise (1e-16), so the error is measured against the terms that cancel (key.weight's)
            assert float((p.grad - want).abs().max()) <= 1e-12 * float(g.t(f'{name}/gp64/key.weight').abs().max()), k
        else:
            assert rel(p.grad, want) <= 1e-12, k


def test_exports_are_declared_built_and_bound():
    pkg = load_pkg()
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    h = ctypes.CDLL(pkg.build.build())
    for name in EXPORTS:
        assert re.search(r'\bint\s+' + name + r'\s*\(', src), f'{name} is not declared in the header'
        assert hasattr(h, name), f'{name} is not exported by the library'
        assert name in pkg._lib.SIGNATURES
    assert h.dcf_abi_version() == 12
    assert callable(pkg.autograd.window_attention) and callable(pkg.autograd.masked_mha)


def test_autograd_functions_have_no_cpu_path():
    pkg = load_pkg()
    z = torch.zeros(1, 4, 32)
    with pytest.raises(RuntimeError, match='GPU'):
        pkg.autograd.window_attention(z, z, z, None, 4, 9)
    mha = pkg.modeling.MaskedMHA(32, n_heads=4, window_size=9)
    with pytest.raises(RuntimeError, match='GPU'):
        pkg.autograd.masked_mha(z, z, z, None, mha)
