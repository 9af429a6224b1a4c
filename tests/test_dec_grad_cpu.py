"""CPU checks around csrc/xattn_grad.hip and autograd.transformer_decoder / xattn_fusion: the closed forms of tests/dec_grad_ref.py
against fp64 autograd through the oracle's `_mha_global_qkv` and `transformer_decoder`, the oracle under fp64 autograd against the
reference's own modules (tests/golden/dec_grad*.npz, make_golden_dec_grad.py), the fixture's fp32 gradients against its fp64 ones by
the project's gradient rule, and the presence of the exports and of the autograd functions.  No GPU.

The gradient rule, per tensor: e <= max(4 e_ref, 2^-21 max |g_64|).  The third part pins what the GPU tests take for e_ref: the
reference's fp32 `backward()` must itself be an fp32-class result (within 2^-17 max |g_64| of the fp64 one: 64 roundings of the largest element), and
fp32 autograd through the oracle, a second fp32 evaluation of the same function, must pass the rule against it."""
import ctypes
import re

import pytest
import torch

from conftest import load_pkg
import dec_grad_ref as R
from test_abi import HEADER

EXPORTS = ('dcf_op_xattn_bwd', 'dcf_op_adaln', 'dcf_op_adaln_bwd')
FLOOR = 2.0 ** -21
# a constant added to every key moves all scores of a row alike: the gradient of key.bias is 0 in exact arithmetic and the fixture
# holds rounding noise; its error is measured against the terms that cancel (key.weight's gradient)
ZERO_BY_SYMMETRY = {'xattn.xattn.key.bias': 'xattn.xattn.key.weight'}


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


CORE_CASES = [(2, 7, 5, 16, 4, True), (1, 1, 9, 8, 2, False), (3, 12, 1, 8, 2, False), (2, 9, 33, 32, 4, True), (1, 20, 64, 16, 1, True)]


@pytest.mark.parametrize('B,T,Lk,C,heads,masked', CORE_CASES)
def test_cross_attention_closed_forms_equal_autograd_through_the_oracle(B, T, Lk, C, heads, masked):
    gen = torch.Generator().manual_seed(T * 7 + Lk + C)
    q = torch.randn(B, T, C, dtype=torch.float64, generator=gen)
    k, v = (torch.randn(B, Lk, C, dtype=torch.float64, generator=gen) for _ in range(2))
    do = torch.randn(B, T, C, dtype=torch.float64, generator=gen)
    mask = R.holes(B, Lk, gen) if masked else None
    qr, kr, vr = (z.clone().requires_grad_(True) for z in (q, k, v))
    o = R.oracle_cross_attention(qr, kr, vr, mask, heads)
    assert rel(R.cross_attention(q, k, v, mask, heads), o) <= 1e-12
    want = torch.autograd.grad((o * do).sum(), (qr, kr, vr))
    got = R.cross_attention_grads(q, k, v, mask, do, heads)
    for a, b in zip(got, want):
        assert float((a - b).abs().max()) <= 1e-12 * max(float(b.abs().max()), 1e-3)
    if mask is not None:
        assert bool((got[1][~mask] == 0).all()) and bool((got[2][~mask] == 0).all()), 'dK = dV = 0 exactly at a masked key'
    if Lk == 1:
        assert float(got[0].abs().max()) == 0.0 and float(got[1].abs().max()) == 0.0, 'one key: dS = 0 exactly'


@pytest.mark.parametrize('norm', [True, False])
@pytest.mark.parametrize('masked', [True, False])
def test_adaln_closed_forms_equal_autograd_through_the_oracle(norm, masked):
    gen = torch.Generator().manual_seed(3 + norm)
    B, T, C = 2, 11, 12
    x, dy = (torch.randn(B, T, C, dtype=torch.float64, generator=gen) for _ in range(2))
    h = torch.randn(B, T, 2 * C, dtype=torch.float64, generator=gen)
    mask = (torch.rand(B, T, generator=gen) > 0.3) if masked else None
    xr, hr = x.clone().requires_grad_(True), h.clone().requires_grad_(True)
    y = R.oracle_adaln(xr, mask, hr, norm)
    assert rel(R.adaln(x, mask, h, norm), y) <= 1e-12
    gx, gh = torch.autograd.grad((y * dy).sum(), (xr, hr))
    dx, dh = R.adaln_grads(x, mask, h, dy, norm)
    assert rel(dx, gx) <= 1e-12 and rel(dh, gh) <= 1e-12
    if masked:
        assert bool((dx[~mask] == 0).all()) and bool((gx[~mask] == 0).all())
        assert torch.equal(R.adaln(x, mask, h, norm)[~mask], h[..., C:][~mask]), 'a masked row holds the shift'


@pytest.mark.parametrize('name', ['adaln', 'affine', 'single'])
def test_oracle_decoder_reproduces_the_reference_backward_in_fp64(name):
    f = R.Fixture(name, torch.float64)
    y, gvid, gtext, gp = f.oracle_grads()
    assert rel(y, f.out['64']) <= 1e-9
    assert rel(gvid, f.gvid['64']) <= 1e-9 and rel(gtext, f.gtext['64']) <= 1e-9
    assert len(gp) == len(f.gp['64']) == (22 if f.single else 46)
    for k, got in gp.items():
        want = f.gp['64'][k]
        sym = [w for z, w in ZERO_BY_SYMMETRY.items() if k.endswith(z)]
        if sym:
            ref = f.gp['64'][k[:-len('xattn.xattn.key.bias')] + sym[0]]
            assert float((got - want).abs().max()) <= 1e-9 * float(ref.abs().max()), k
        else:
            assert rel(got, want) <= 1e-9, k


@pytest.mark.parametrize('name', ['adaln', 'affine', 'single'])
def test_fixture_fp32_gradients_are_what_the_gpu_tests_take_for_e_ref(name):
    f = R.Fixture(name, torch.float32)
    y, gvid, gtext, gp = f.oracle_grads()                       # a second fp32 evaluation of the same function
    tensors = [('out', f.out, y), ('gvid', f.gvid, gvid), ('gtext', f.gtext, gtext)] + [(k, {t: f.gp[t][k] for t in ('32', '64')}, gp[k]) for k in gp]
    for tag, fx, mine in tensors:
        g64, g32 = fx['64'].double(), fx['32'].double()
        assert fx['32'].dtype == torch.float32 and fx['64'].dtype == torch.float64, tag
        top, e_ref = float(g64.abs().max()), float((g32 - g64).abs().max())
        if any(tag.endswith(z) for z in ZERO_BY_SYMMETRY):
            top = float(f.gp['64'][tag[:-len('bias')] + 'weight'].abs().max())
        assert e_ref <= 2.0 ** -17 * top, (tag, e_ref, top)               # an fp32-class result (ln_out.bias, a sum of the 2^-10 grid of `up`, is exact)
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
    for name in ('cross_attention', 'adaln_modulate', 'xattn_mha', 'conv_xattn_layer', 'transformer_decoder', 'xattn_fusion'):
        assert callable(getattr(pkg.autograd, name)), name


def test_autograd_functions_refuse_the_cpu():
    pkg = load_pkg()
    A, M = pkg.autograd, pkg.modeling
    z, kv = torch.zeros(1, 4, 64), torch.zeros(1, 3, 96)
    blk = M.TransformerDecoder(64, 96, 4)
    fus = M.XAttNFusion(64, 96, 1, 4)
    for call in (lambda: A.cross_attention(z, z, z, None, 4), lambda: A.adaln_modulate(z, None, torch.zeros(1, 4, 128)),
                 lambda: A.xattn_mha(z, kv, None, blk.xattn.xattn), lambda: A.transformer_decoder(z, None, kv, None, blk),
                 lambda: A.xattn_fusion(z, None, kv, None, fus)):
        with pytest.raises(RuntimeError, match='GPU'):
            call()
    with pytest.raises(ValueError, match='window_size = 0'):
        A.xattn_mha(z, kv, None, M.MaskedMHA(64, n_heads=4, window_size=9))
