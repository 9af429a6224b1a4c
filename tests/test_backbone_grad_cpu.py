"""CPU checks around the k = 5 / stride-2 kernels of csrc/conv_grad.hip and autograd.video_transformer / text_transformer: the closed
forms of tests/backbone_grad_ref.py against fp64 autograd through the oracle's `masked_conv1d(..., stride=2)`, the oracle's
`video_transformer` / `text_transformer` under fp64 autograd against the reference's own modules (tests/golden/backbone_grad_*.npz,
make_golden_backbone_grad.py), the fixtures' fp32 gradients against their fp64 ones by the project's gradient rule, and the presence of
the exports and of the autograd functions.  No GPU.

The gradient rule, per tensor: e <= max(4 e_ref, 2^-21 max |g_64|).  The fourth part pins what the GPU tests take for e_ref: the
reference's fp32 `backward()` must itself be an fp32-class result (within 2^-17 max |g_64| of the fp64 one) and fp32 autograd through the
oracle, a second fp32 evaluation of the same function, must pass the rule against it.  For key.bias of every block (the stride-0 ones
included) and k_norm.bias of the video blocks, whose gradients are zero in exact arithmetic, max |g_64| is that of the same layer's
key.weight / k_norm.weight (ZERO_BY_SYMMETRY of tests/test_enc_grad_cpu.py and tests/test_dec_grad_cpu.py)."""
import ctypes
import inspect
import re

import pytest
import torch

from conftest import load_pkg
import backbone_grad_ref as R
from test_abi import HEADER

EXPORTS = ('dcf_op_conv5s2_split', 'dcf_op_conv5s2_bwd_data', 'dcf_op_conv5s2_bwd_weight')
FLOOR = 2.0 ** -21
N_PARAMS = {'s4': 116, 's2': 116, 'pool': 38, 'text': 39}


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


def op_case(B, T, Cin, N, masked):
    gen = torch.Generator().manual_seed(B * 100 + T + Cin + N)
    x = torch.randn(B, T, Cin, dtype=torch.float64, generator=gen)
    w = torch.randn(N, Cin, 5, dtype=torch.float64, generator=gen)
    dy = torch.randn(B, T // 2, N, dtype=torch.float64, generator=gen)
    mask = R.holes(B, T, [T - (b % 2) * 3 for b in range(B)], gen) if masked else None
    return x, w, dy, mask


@pytest.mark.parametrize('B,T,Cin,N,masked', [(2, 10, 4, 6, True), (1, 2, 3, 3, False), (3, 6, 5, 2, False)])
def test_closed_forms_equal_fp64_autograd_through_the_oracle(B, T, Cin, N, masked):
    x, w, dy, mask = op_case(B, T, Cin, N, masked)
    y, gx, gw = R.conv5s2_autograd(x, mask, w, dy)
    assert rel(R.conv5s2(x, mask, w), y) <= 1e-12
    assert rel(R.conv5s2_bwd_weight(x, mask, dy), gw) <= 1e-12
    dx = R.conv5s2_bwd_data(dy, mask, w)
    assert rel(dx, gx) <= 1e-12
    if mask is not None:
        assert not bool(mask.all())
        assert bool((dx[~mask] == 0).all()) and bool((gx[~mask] == 0).all()), 'dX is exactly 0 at masked rows'
        assert torch.equal(R.oracle_conv5s2(x, mask, w)[1], mask[:, ::2]), 'the mask that goes on is m[b, 2u]'


def test_taps_stay_inside_their_sequence():
    """large values in the second sequence: the first one's output and gradients are those of the first sequence alone"""
    x, w, dy, _ = op_case(2, 8, 4, 3, False)
    x[1] *= 1e6
    dy[1] *= 1e6
    assert torch.equal(R.conv5s2(x, None, w)[0], R.conv5s2(x[:1], None, w)[0])
    assert torch.equal(R.conv5s2_bwd_data(dy, None, w)[0], R.conv5s2_bwd_data(dy[:1], None, w)[0])


@pytest.mark.parametrize('name', R.CASES + ('text',))
def test_oracle_backbones_reproduce_the_reference_backward_in_fp64(name):
    f = R.Fixture(name, torch.float64)
    ys, masks, gx, gp = f.oracle_grads()
    assert len(ys) == f.n_levels == (1 if f.text else 3)
    for y, m, want, wm in zip(ys, masks, f.out['64'], f.mask_out):
        assert rel(y, want) <= 1e-10 and torch.equal(m, wm)
    assert rel(gx, f.gx['64']) <= 1e-10
    assert len(gp) == len(f.gp['64']) == N_PARAMS[name]
    for k, got in gp.items():
        want = f.gp['64'][k]
        assert float((got - want).abs().max()) <= 1e-10 * f.top(want, k), k


@pytest.mark.parametrize('name', R.CASES + ('text',))
def test_fixture_fp32_gradients_are_what_the_gpu_tests_take_for_e_ref(name):
    f = R.Fixture(name, torch.float32)
    ys, _, gx, gp = f.oracle_grads()                             # a second fp32 evaluation of the same function
    tensors = [(f'out{l}', {t: f.out[t][l] for t in ('32', '64')}, ys[l], None) for l in range(f.n_levels)]
    tensors += [('gx', f.gx, gx, None)] + [(k, {t: f.gp[t][k] for t in ('32', '64')}, gp[k], k) for k in gp]
    for tag, fx, mine, k in tensors:
        g64, g32 = fx['64'].double(), fx['32'].double()
        assert fx['32'].dtype == torch.float32 and fx['64'].dtype == torch.float64, tag
        top, e_ref = f.top(g64, k), float((g32 - g64).abs().max())
        assert e_ref <= 2.0 ** -17 * top, (tag, e_ref, top)
        assert float((mine.double() - g64).abs().max()) <= max(4 * e_ref, FLOOR * top), tag


def test_key_bias_gradients_of_the_text_blocks_are_stored_and_are_rounding_noise():
    f = R.Fixture('text', torch.float64)
    keys = [k for k in f.gp['64'] if k.endswith('attn.attn.key.bias')]
    assert len(keys) == 2
    for k in keys:
        assert float(f.gp['64'][k].abs().max()) <= 1e-12 * f.top(None, k)


def test_exports_are_declared_built_and_bound():
    pkg = load_pkg()
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    h = ctypes.CDLL(pkg.build.build())
    for name in EXPORTS:
        assert re.search(r'\bint\s+' + name + r'\s*\(', src), f'{name} is not declared in the header'
        assert hasattr(h, name), f'{name} is not exported by the library'
        assert name in pkg._lib.SIGNATURES
    assert h.dcf_abi_version() == 12
    for name in ('video_transformer', 'text_transformer', 'strided_masked_conv1d'):
        assert callable(getattr(pkg.autograd, name)), name
    sig = inspect.signature(pkg.autograd.masked_conv1d)
    assert list(sig.parameters) == ['x', 'mask', 'weight', 'bias', 'stride'] and sig.parameters['stride'].default == 1


def test_autograd_functions_refuse_the_cpu_and_what_has_no_backward():
    pkg = load_pkg()
    A, M = pkg.autograd, pkg.modeling
    z = torch.zeros(1, 4, 32)
    vn = M.VideoTransformer(32, 32, 4, 4, 3, stride=2, arch=(1, 0, 1))
    tn = M.TextTransformer(32, 32, 2, 8, n_layers=1)
    for call in (lambda: A.masked_conv1d(z, None, torch.zeros(32, 32, 5), None, 2), lambda: A.video_transformer(z, None, vn),
                 lambda: A.text_transformer(z, None, tn), lambda: A.transformer_encoder(z, None, tn.transformer[0])):
        with pytest.raises(RuntimeError, match='GPU'):
            call()
    with pytest.raises(ValueError, match='no bias'):
        A.masked_conv1d(z, None, torch.zeros(32, 32, 5), torch.zeros(32), 2)
    with pytest.raises(ValueError, match='stride = 3'):
        A.masked_conv1d(z, None, torch.zeros(32, 32, 5), None, 3)
    with pytest.raises(ValueError, match='TextIdentity is not differentiable yet'):
        A.text_transformer(z, None, M.TextIdentity(32, 32, 8))
    with pytest.raises(ValueError, match='window_size = 0'):
        A.transformer_encoder(z, None, M.TransformerEncoder(32, 1, 4, 0))
