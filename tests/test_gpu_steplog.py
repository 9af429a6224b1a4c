"""GPU checks of the training-log operators (dcf_op_steplog_add / dcf_op_steplog_flush, include/decafnet_hip_steplog.h,
csrc/steplog.hip).

1. The cases of tests/steplog_abi_cases.py between poisoned borders through tests/borders.run_case / arena.run_three_ways, with both
   fills: the inputs untouched, nothing outside the operands written, the tables and ``out`` equal to the plain run and bit for bit to
   the restatement of tests/steplog_ref.py.
2. A sequence: 257 adds of K = 3 random fp32 scalars held in three separate allocations (one of them at an odd 4-byte offset inside a
   larger tensor), a flush, 2 adds, a flush.  Both ``out`` buffers bit for bit the restatement's; the second shows the reset; two
   fresh runs give the same bits.
3. The refusals: non-zero, the export's name in the message, ``stats``, ``counts`` and ``out`` as they were."""
import ctypes

import numpy as np
import pytest
import torch

import borders
import steplog_abi_cases as C
import steplog_ref as R
from borders import ctx  # noqa: F401  (the module-scoped fixture)
from conftest import load_pkg

pytestmark = pytest.mark.gpu
IDS = [f'{c.export}-{c.tag}' for c in C.CASES]


def test_case_table_covers_the_steplog_record():
    table = load_pkg()._lib.STEPLOG[0].table
    assert {c.export for c in C.CASES} | set(C.EXCLUDED) == set(table) and len(set(IDS)) == len(IDS)
    assert not {c.export for c in C.CASES} & set(C.EXCLUDED) and set(C.EXCLUDED) == {'dcf_steplog_ext_version'}
    assert all(isinstance(r, str) and r.strip() for r in C.EXCLUDED.values())


def _after(case, specs, plain, verify):
    verify(plain)


@pytest.mark.parametrize('case', C.CASES, ids=IDS)
def test_poisoned_borders(ctx, case):
    borders.run_case(ctx, case, _after)


N_ADDS, K = 257, 3


def _sequence(ctx, vals):
    """the adds and flushes of the docstring on fresh tables -> the two ``out`` buffers and the tables afterwards, as numpy"""
    lib, st, p, check = ctx.lib, ctx.stream(), C.p, ctx.pkg._lib.check
    a, c = torch.zeros(1, device='cuda'), torch.zeros(1, device='cuda')           # three allocations; the middle value lies at an
    big = torch.zeros(64, device='cuda')                                          # odd 4-byte offset inside a larger tensor
    b = big[37:38]
    assert b.data_ptr() % 8 == 4 and len({a.data_ptr(), b.data_ptr(), c.data_ptr()}) == 3
    ptrs = (ctypes.c_void_p * K)(a.data_ptr(), b.data_ptr(), c.data_ptr())
    stats = torch.zeros(K, R.COLS, dtype=torch.float64, device='cuda')
    counts = torch.zeros(K + 1, dtype=torch.int64, device='cuda')
    outs = [torch.full((K + 1, R.COLS), -7.0, dtype=torch.float64, device='cuda') for _ in range(2)]
    dev = torch.from_numpy(vals).cuda()

    def adds(rows):
        for i in rows:
            a.copy_(dev[i, 0:1]), b.copy_(dev[i, 1:2]), c.copy_(dev[i, 2:3])      # stream order: the add reads what this step wrote
            check(lib.dcf_op_steplog_add(ptrs, K, p(stats), p(counts), st), 'dcf_op_steplog_add')

    adds(range(N_ADDS))
    check(lib.dcf_op_steplog_flush(p(stats), p(counts), K, p(outs[0]), st), 'dcf_op_steplog_flush')
    adds(range(N_ADDS, N_ADDS + 2))
    check(lib.dcf_op_steplog_flush(p(stats), p(counts), K, p(outs[1]), st), 'dcf_op_steplog_flush')
    torch.cuda.synchronize()
    assert not big[:37].any() and not big[38:].any()
    return [o.cpu().numpy() for o in outs], stats.cpu().numpy(), counts.cpu().numpy()


def test_a_sequence_of_adds_and_flushes_is_the_restatement(ctx):
    g = np.random.default_rng(12)
    vals = (g.standard_normal((N_ADDS + 2, K)) * np.array([1.0, 1e3, 1e-3])).astype(np.float32)
    vals[100, 0], vals[200, 1] = np.nan, np.inf                                  # one key poisoned, one infinite, one clean
    stats, counts = R.empty(K)
    want = []
    for rows in (range(N_ADDS), range(N_ADDS, N_ADDS + 2)):
        for i in rows:
            R.add(stats, counts, vals[i])
        want.append(R.flush(stats, counts))
    first = _sequence(ctx, vals)
    for got, w, what in zip(first[0], want, ('the first flush', 'the second flush')):
        print(f'STEPLOG {what}: means {got[:K, 0].tolist()} want {w[:K, 0].tolist()} steps {got[K, 0]}')
        assert np.array_equal(R.bits(got), R.bits(w)), f'{what}: {int((R.bits(got) != R.bits(w)).sum())} words differ'
    assert first[0][0][K, 0] == N_ADDS and first[0][1][K, 0] == 2, 'the second flush shows the reset'
    assert first[0][0][:K, 5].tolist() == [N_ADDS - 1, N_ADDS - 1, N_ADDS] and first[0][1][:K, 5].tolist() == [2, 2, 2]
    assert np.isnan(first[0][0][0, 0]) and first[0][0][1, 0] == np.inf and np.isfinite(first[0][1]).all()
    assert not first[1].any() and not first[2].any(), 'a flush leaves the tables empty'
    second = _sequence(ctx, vals)                                                 # two fresh runs: the same bits
    for x, y in zip(first[0], second[0]):
        assert np.array_equal(R.bits(x), R.bits(y))


def test_refusals_launch_nothing(ctx):
    lib, st, p = ctx.lib, ctx.stream(), C.p
    vals = [torch.full((2,), 1.5, device='cuda') for _ in range(K)]
    stats = torch.full((K, R.COLS), -7.0, dtype=torch.float64, device='cuda')
    counts = torch.full((K + 1,), -7, dtype=torch.int64, device='cuda')
    out = torch.full((K + 1, R.COLS), -7.0, dtype=torch.float64, device='cuda')
    odd = lambda t, by: ctypes.c_void_p(t.data_ptr() + by)
    array = lambda ptrs: (ctypes.c_void_p * len(ptrs))(*ptrs)
    good = [v.data_ptr() for v in vals]
    a = dict(vals=array(good), K=K, stats=p(stats), counts=p(counts), out=p(out))
    tables = [dict(K=0), dict(K=-1), dict(K=17), dict(stats=None), dict(counts=None), dict(stats=odd(stats, 4)), dict(counts=odd(counts, 4))]
    bad_add = tables + [dict(vals=None), dict(vals=array([good[0], None, good[2]])), dict(vals=array([good[0], good[1] + 2, good[2]])),
                        dict(vals=array([good[0] + 1, good[1], good[2]]))]
    bad_flush = tables + [dict(out=None), dict(out=odd(out, 4))]
    run_add = lambda k: lib.dcf_op_steplog_add(k['vals'], k['K'], k['stats'], k['counts'], st)
    run_flush = lambda k: lib.dcf_op_steplog_flush(k['stats'], k['counts'], k['K'], k['out'], st)
    for name, run, bad in (('dcf_op_steplog_add', run_add, bad_add), ('dcf_op_steplog_flush', run_flush, bad_flush)):
        for change in bad:
            assert run(dict(a, **change)) != 0, (name, change)
            msg = lib.dcf_last_error().decode()
            assert name in msg, (change, msg)
    torch.cuda.synchronize()
    assert bool((stats == -7.0).all()) and bool((counts == -7).all()) and bool((out == -7.0).all())
    assert bool(torch.stack(vals).eq(1.5).all())
    ok = dict(a, vals=array([good[0], good[1] + 4, good[2]]))                     # 4-byte alignment is all an entry needs
    stats.zero_(), counts.zero_()
    assert run_add(ok) == 0 and run_flush(a) == 0
    torch.cuda.synchronize()
    assert out[:K, 0].tolist() == [1.5] * K and out[K].tolist() == [1.0, 0, 0, 0, 0, 0] and not bool(counts.any())
