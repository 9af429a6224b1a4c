"""CPU checks that go with the embedding-stage extension (include/decafnet_hip_embd.h, csrc/embd_chain.h): the fold of vid_net.embd_fc
(and of fusion.ln_out's affine) into the first embedding convolution is exact to fp64 rounding against the composition the reference
writes, on ragged masks and at the first and last valid row of every sequence; the names of ``_lib.EMBD_SIGNATURES`` and the
parameter order of its two operators (its header and table: tests/test_abi_headers.py).  No GPU."""
import ctypes

import pytest
import torch

import abi_headers as H
from conftest import load_pkg
import embd_chain_ref as ER

NAMES = ['dcf_embd_ext_version', 'dcf_op_embd_chain', 'dcf_op_embd_launches']


def random_params(E, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return dict(Wfc=r(E, E) / E ** 0.5, bfc=r(E), g=1 + 0.3 * r(E), b=0.5 * r(E),
                Wc=[r(E, E, 3) / (3 * E) ** 0.5 for _ in range(2)], lw=[1 + 0.3 * r(E) for _ in range(2)], lb=[0.3 * r(E) for _ in range(2)])


def ragged_masks(B, T, seed):
    """valid prefixes of different lengths, holes inside them, one fully masked sequence, one full one"""
    g = torch.Generator().manual_seed(seed)
    mask = torch.zeros(B, T, dtype=torch.bool)
    for b in range(B):
        n = T if b == 0 else (0 if b == 2 else int(torch.randint(1, T + 1, (1,), generator=g)))
        mask[b, :n] = True
        if b % 2 == 1 and n > 4:
            mask[b, torch.randint(1, n - 1, (2,), generator=g)] = False
    return mask


@pytest.mark.parametrize('ln_in', [True, False])
@pytest.mark.parametrize('with_pe', [True, False])
@pytest.mark.parametrize('B,T', [(5, 19), (3, 1), (4, 2)])
def test_the_fold_is_exact_to_fp64_rounding(B, T, with_pe, ln_in):
    E = 32
    p = random_params(E, 11)
    g = torch.Generator().manual_seed(5 + B + T)
    X = torch.randn(B, T, E, generator=g, dtype=torch.float64) * 2 + 0.5
    mask = ragged_masks(B, T, 17)
    pe = torch.randn(T + 3, E, generator=g, dtype=torch.float64) if with_pe else None
    want = ER.stage_unfolded(X, mask, p, ln_in, pe)
    got = ER.stage_folded(X, mask, p, ln_in, pe)
    assert torch.isfinite(want).all()
    # every row, the padded ones included: MaskedConv1D does not mask its output, and the folded form agrees there too
    err, scale = float((got - want).abs().max()), float(want.abs().max())
    assert err <= 1e-12 * scale, (err, scale)
    for b in range(B):                                     # the first and the last valid row of every sequence
        idx = torch.nonzero(mask[b]).flatten()
        if idx.numel():
            for t in (int(idx[0]), int(idx[-1])):
                assert float((got[b, t] - want[b, t]).abs().max()) <= 1e-12 * scale, (b, t)


def test_the_gated_bias_matters_at_sequence_edges_and_holes():
    """dropping the per-tap gate (one bias vector added everywhere, what a folded 1x1 bias would be in an unmasked convolution) is
    wrong exactly where a neighbour is missing: the check above can tell the two apart"""
    E, B, T = 16, 2, 9
    p = random_params(E, 3)
    X = torch.randn(B, T, E, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    mask = torch.ones(B, T, dtype=torch.bool)
    mask[1, 6:] = False
    mask[1, 3] = False
    Wp, c = ER.fold(p, True)
    m = mask.unsqueeze(-1).double()
    xh = ER.ln(X)
    ungated = sum(ER.shifted(m, t) * (ER.shifted(xh, t) @ Wp[t].T) for t in range(3)) + c.sum(0)
    gated = sum(ER.shifted(m, t) * (ER.shifted(xh, t) @ Wp[t].T + c[t]) for t in range(3))
    diff = (ungated - gated).abs().amax(-1) > 1e-9
    full = mask & ER.shifted(m, 0).squeeze(-1).bool() & ER.shifted(m, 2).squeeze(-1).bool()
    assert torch.equal(diff, ~full)


# ---------------------------------------------------------------------------------------------- the ABI
def test_embd_table_names_and_parameter_order():
    table = load_pkg()._lib.EMBD_SIGNATURES
    assert sorted(table) == NAMES
    order = ['model', 'X', 'ldx', 'mask', 'B', 'T', 'ln_in', 'pe', 'Y', 'ldy', 'stream']
    for name in NAMES[1:]:
        assert H.param_names('decafnet_hip_embd.h', name) == order, name
    assert table['dcf_op_embd_chain'] == table['dcf_op_embd_launches']


def test_the_operators_refuse_a_null_model_before_a_launch():
    pkg = load_pkg()
    h = ctypes.CDLL(pkg.build.build())
    a = ctypes.c_void_p(4096)                              # never dereferenced: the calls fail in their argument checks
    for name in NAMES[1:]:
        fn = getattr(h, name)
        fn.restype, fn.argtypes = pkg._lib.EMBD_SIGNATURES[name]
        assert fn(None, a, 256, a, 1, 8, 1, None, a, 256, None) == -1
        h.dcf_last_error.restype = ctypes.c_char_p
        assert b'null argument' in h.dcf_last_error()
