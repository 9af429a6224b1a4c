"""GPU checks of the backward of the global self-attention core (csrc/global_attn_grad.hip: dcf_op_global_attn_bwd,
include/decafnet_hip_attn.h).

The yardstick is the project's gradient rule, per gradient tensor:

    e_gpu <= max(4 * e_ref, 2^-21 * max |g_64|),   e = max |g - g_64|

At the shapes of global_attn_grad_ref.SHAPES that are marked F, g_64 is the reference's own fp64 `backward()` of MaskedMHA(window_size=0)
and e_ref the error of its fp32 `backward()` (tests/golden/global_attn_grad.npz; the operands of the core are exact in fp32 there, the
rows compared are the stored ones, e_ref and max |g_64| those of the whole tensor); at the others g_64 is the fp64 restatement
(global_attn_grad_ref.grads, pinned to the fixture and to finite differences by tests/test_global_attn_grad_cpu.py) and e_ref its fp32
evaluation on the CPU.  Every check prints a `GAERR` line; the table is in profiles/global_attn_grad.md.

The tile is 64 queries / 64 keys: T = 1, 37, 64, 65, 130 (two tiles and a tail), a last tile that is all padding, and a sequence
without a valid key.  q, k, v ~ N(0, 1) and dO ~ N(0, 1) on EVERY row: the mask masks keys only, a padded query row is live."""
import pytest
import torch

from conftest import load_pkg
import global_attn_grad_ref as R

pytestmark = pytest.mark.gpu
NAMES = ('dQ', 'dK', 'dV')


class Lib:
    def __init__(self):
        self.pkg = load_pkg()
        self.L, self.l = self.pkg._lib.lib(), self.pkg._lib

    def raw(self, q, k, v, mask, do, heads, want=(True, True, True)):
        """(return code, (dQ, dK, dV)) of device tensors; outputs pre-filled with NaN, None where not wanted"""
        B, T, C = q.shape
        l = self.l
        outs = [torch.full_like(q, float('nan')) if w else None for w in want]
        rc = self.L.dcf_op_global_attn_bwd(l.ptr(q), l.ptr(k), l.ptr(v), l.ptr(mask), l.ptr(do), l.ptr(outs[0]), l.ptr(outs[1]), l.ptr(outs[2]),
                                           B, T, C, heads, l.current_stream())
        return rc, outs

    def bwd(self, *a, **kw):
        rc, outs = self.raw(*a, **kw)
        self.l.check(rc, 'dcf_op_global_attn_bwd')
        return outs


@pytest.fixture(scope='module')
def lib():
    return Lib()


def cu(*ts):
    return [None if t is None else t.cuda() for t in ts]


@pytest.mark.parametrize('name', [s[0] for s in R.SHAPES if not s[7]])
def test_gradients_match_the_fp64_restatement(lib, name):
    q, k, v, do, mask, heads = R.shape_case(name)
    g64, g32 = R.reference_pair(q, k, v, mask, do, heads)
    got = lib.bwd(*cu(q, k, v, mask, do), heads)
    for n, a, b, c in zip(NAMES, got, g64, g32):
        if float(b.abs().max()) == 0.0:                       # one key: dS = 0 exactly
            assert bool((a == 0).all()), (name, n)
            print(f'GAERR {name} {n}: exactly 0')
        else:
            R.rule(f'{name} {n}', a, b, c)
        if mask is not None and n != 'dQ':
            assert bool((a.cpu()[~mask] == 0).all()), f'{n} at a padded key is exactly 0'


@pytest.mark.parametrize('name', [s[0] for s in R.SHAPES if s[7]])
def test_gradients_match_the_reference_backward(lib, name):
    f = R.OpFixture(name)
    got = lib.bwd(*cu(f.q, f.k, f.v, f.mask, f.do), f.heads)
    for n, a in zip(NAMES, got):
        R.fixture_rule(f'{name} {n} (reference)', f.at_rows(a), f, n.lower())
        if n != 'dQ':
            assert bool((a.cpu()[~f.mask] == 0).all()), f'{n} at a padded key is exactly 0'
    g64, g32 = R.reference_pair(f.q, f.k, f.v, f.mask, f.do, f.heads)      # every row, against the restatement
    for n, a, b, c in zip(NAMES, got, g64, g32):
        R.rule(f'{name} {n} (all rows)', a, b, c)


def test_padded_query_rows_are_live(lib):
    """the mask masks keys only: dQ at a padded row is not zero, and dO at a padded row reaches dK and dV"""
    q, k, v, do, mask, heads = R.shape_case('last_tile_padded')
    dq, dk, dv = lib.bwd(*cu(q, k, v, mask, do), heads)
    assert float(dq.cpu()[~mask].abs().min(dim=-1).values.max()) > 0
    do2 = do.clone()
    do2[~mask] = 0
    dq2, dk2, dv2 = lib.bwd(*cu(q, k, v, mask, do2), heads)
    assert torch.equal(dq2.cpu()[mask], dq.cpu()[mask]) and bool((dq2.cpu()[~mask] == 0).all())
    assert not torch.equal(dk2, dk) and not torch.equal(dv2, dv)


def test_a_sequence_without_a_valid_key(lib):
    """its three gradients are exactly 0 and the other sequence of the batch has the bits it has alone"""
    q, k, v, do, mask, heads = R.shape_case('no_valid_key')
    assert not bool(mask[1].any()) and bool(mask[0].all())
    both = lib.bwd(*cu(q, k, v, mask, do), heads)
    alone = lib.bwd(*cu(q[:1], k[:1], v[:1], mask[:1], do[:1]), heads)
    for n, a, b in zip(NAMES, both, alone):
        assert bool((a[1] == 0).all()), n
        assert torch.equal(a[0], b[0]), n


@pytest.mark.parametrize('name', ['past_tile', 'two_tiles_tail', 'tile'])
def test_bit_for_bit(lib, name):
    q, k, v, do, mask, heads = R.shape_case(name)
    args = cu(q, k, v, mask, do)
    full = lib.bwd(*args, heads)
    again = lib.bwd(*args, heads)
    scaled = lib.bwd(*args[:4], args[4] * 256, heads)
    for n, a, b, c in zip(NAMES, full, again, scaled):
        assert torch.equal(a, b), f'{n}: two runs differ'
        assert torch.equal(c, a * 256), f'{n}: dO * 256 is not 256 times the output'
    for skip in range(3):
        want = tuple(i != skip for i in range(3))
        part = lib.bwd(*args, heads, want=want)
        for i in range(3):
            assert (part[i] is None) if i == skip else torch.equal(part[i], full[i]), (skip, i)
    only_q = lib.bwd(*args, heads, want=(True, False, False))
    assert torch.equal(only_q[0], full[0])
    if mask is None:
        ones = torch.ones(q.shape[:2], dtype=torch.bool).cuda()
        for n, a, b in zip(NAMES, full, lib.bwd(args[0], args[1], args[2], ones, args[4], heads)):
            assert torch.equal(a, b), f'{n}: NULL mask differs from an all-ones mask'


def test_null_mask_equals_an_all_ones_mask_past_a_tile(lib):
    q, k, v, do, _, heads = R.shape_case('past_tile')
    args = cu(q, k, v, None, do)
    ones = torch.ones(q.shape[:2], dtype=torch.bool).cuda()
    for n, a, b in zip(NAMES, lib.bwd(*args, heads), lib.bwd(args[0], args[1], args[2], ones, args[4], heads)):
        assert torch.equal(a, b), n


@pytest.mark.parametrize('C,heads,word', [(64, 4, 'head dimension'), (128, 1, 'head dimension'), (64, 3, 'heads')])
def test_unsupported_shapes_fail_with_a_message_and_launch_nothing(lib, C, heads, word):
    z = torch.zeros(1, 8, C).cuda()
    rc, outs = lib.raw(z, z, z, None, z, heads)
    assert rc != 0
    msg = lib.L.dcf_last_error().decode()
    assert word in msg, msg
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outs), 'an output was written'


def test_the_local_export_still_refuses_window_zero(lib):
    z = torch.zeros(1, 8, 64).cuda()
    l = lib.l
    rc = lib.L.dcf_op_local_attn_bwd(l.ptr(z), l.ptr(z), l.ptr(z), None, l.ptr(z), l.ptr(z), l.ptr(z), l.ptr(z), 1, 8, 64, 2, 0, l.current_stream())
    assert rc != 0 and b'window = 0' in lib.L.dcf_last_error()
    assert lib.L.dcf_attn_ext_version() == 1
