"""GPU checks of the validation-loss operator (dcf_op_loss_table_mean, include/decafnet_hip_fit.h, csrc/fit.hip).

1. The cases of tests/fit_abi_cases.py between poisoned borders through tests/borders.run_case / arena.run_three_ways, with both fills:
   the inputs untouched, nothing outside the operands written, ``per_video`` and ``out2`` equal to the plain run and bit for bit to the
   restatement of tests/eval_loss_ref.py; on the tables without NaN or inf ``out2`` within (N + V) * 2^-52 of numpy's own order.
2. Two calls on one table give the same bits.
3. The refusals: non-zero, the export's name in the message, the outputs as they were."""
import ctypes

import numpy as np
import pytest
import torch

import borders
import eval_loss_ref as R
import fit_abi_cases as C
from borders import ctx  # noqa: F401  (the module-scoped fixture)
from conftest import load_pkg

pytestmark = pytest.mark.gpu
IDS = [c.tag for c in C.CASES]


def test_case_table_covers_the_fit_record():
    table = load_pkg()._lib.FIT[0].table
    assert {c.export for c in C.CASES} | set(C.EXCLUDED) == set(table) and len(set(IDS)) == len(IDS)
    assert not {c.export for c in C.CASES} & set(C.EXCLUDED)


def _after(case, specs, plain, verify):
    verify(plain)


@pytest.mark.parametrize('case', C.CASES, ids=IDS)
def test_poisoned_borders(ctx, case):
    borders.run_case(ctx, case, _after)


def _operands(size, seed, special):
    rows, offsets = R.table(C.SIZES[size], seed, special)
    return torch.from_numpy(rows).cuda(), torch.from_numpy(offsets).cuda(), len(offsets) - 1


@pytest.mark.parametrize('size', ['v3', 'v600'])
def test_two_calls_give_the_same_bits(ctx, size):
    rows, offsets, V = _operands(size, 4, size == 'v3')
    p = C.p
    got = []
    for _ in range(2):
        pv, out = torch.full((V, 2), -7.0, dtype=torch.float64, device='cuda'), torch.full((2,), -7.0, dtype=torch.float64, device='cuda')
        ctx.pkg._lib.check(ctx.lib.dcf_op_loss_table_mean(p(rows), p(offsets), V, p(pv), p(out), ctx.stream()), 'dcf_op_loss_table_mean')
        torch.cuda.synchronize()
        got.append((pv.cpu().numpy(), out.cpu().numpy()))
    assert np.array_equal(R.bits(got[0][0]), R.bits(got[1][0])) and np.array_equal(R.bits(got[0][1]), R.bits(got[1][1]))
    assert not (got[0][0] == -7.0).any() and not (got[0][1] == -7.0).any(), 'every element is written'


def test_refusals_launch_nothing(ctx):
    lib, st, p = ctx.lib, ctx.stream(), C.p
    rows, offsets, V = _operands('v3', 4, False)
    pv, out = torch.full((V, 2), -7.0, dtype=torch.float64, device='cuda'), torch.full((2,), -7.0, dtype=torch.float64, device='cuda')
    a = dict(rows=p(rows), offsets=p(offsets), V=V, pv=p(pv), out=p(out))
    odd = lambda t, by: ctypes.c_void_p(t.data_ptr() + by)
    bad = [dict(rows=None), dict(offsets=None), dict(out=None), dict(V=0), dict(V=-2), dict(rows=odd(rows, 2)), dict(offsets=odd(offsets, 4)),
           dict(pv=odd(pv, 4)), dict(out=odd(out, 4))]
    run = lambda k: lib.dcf_op_loss_table_mean(k['rows'], k['offsets'], k['V'], k['pv'], k['out'], st)
    for change in bad:
        assert run(dict(a, **change)) != 0, change
        msg = lib.dcf_last_error().decode()
        assert 'dcf_op_loss_table_mean' in msg, (change, msg)
    torch.cuda.synchronize()
    assert bool((pv == -7.0).all()) and bool((out == -7.0).all())
    assert run(dict(a, pv=None)) == 0                                           # per_video is optional
    torch.cuda.synchronize()
    want = R.loss_table_mean(rows.cpu().numpy(), offsets.cpu().numpy())[1]
    assert np.array_equal(R.bits(out.cpu().numpy()), R.bits(want)) and bool((pv == -7.0).all())
