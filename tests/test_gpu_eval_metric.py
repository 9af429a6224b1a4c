"""GPU checks of the Recall@k operator (dcf_op_recall_update, include/decafnet_hip_eval.h, csrc/eval_metric.hip).

1. The operator through the C ABI against the restatement of tests/eval_metric_ref.py: ``hits`` and ``n_queries`` as integers, ``best``
   as bits, on a ``best`` pre-filled with a value the operator never writes so that an unwritten element shows: the cases of
   tests/eval_abi_cases.py (NaN / inf beyond ``counts``, counts above M and below 0, three calls into one pre-filled table).
2. The same cases between poisoned borders through tests/borders.run_case / arena.run_three_ways, with both fills: the inputs
   untouched, nothing outside the operands written, the outputs equal to the plain run and to the restatement.
3. The refusals: non-zero, the export's name in the message, the tables as they were; then ``best = NULL`` succeeds.
4. ``evaluator.DeviceRecallCounter`` on top: ``update_device`` twice, the accessors, ``reset()``."""
import ctypes

import numpy as np
import pytest
import torch

import borders
import eval_abi_cases as C
import eval_metric_ref as R
from borders import ctx  # noqa: F401  (the module-scoped fixture)
from conftest import load_pkg

pytestmark = pytest.mark.gpu
IDS = [c.tag for c in C.CASES]
UNWRITTEN = -7.0


def test_case_table_covers_the_staged_record():
    table = load_pkg()._lib.STAGED[0].table
    assert {c.export for c in C.CASES} | set(C.EXCLUDED) == set(table) and len(set(IDS)) == len(IDS)


@pytest.mark.parametrize('case', C.CASES, ids=IDS)
def test_operator_equals_the_restatement(ctx, case):
    specs, call, _, verify = case.make()
    v = {}
    for name, t, role, *_ in specs:
        v[name] = torch.full(t.shape, UNWRITTEN, dtype=t.dtype, device='cuda') if role == 'out' else t.cuda()
    ctx.pkg._lib.check(call(ctx, v), case.export)
    torch.cuda.synchronize()
    verify(v)
    assert not bool((v['best'] == UNWRITTEN).any()), 'best is written for every query'
    for name, t, role, *_ in specs:
        if role == 'in':
            assert torch.equal(v[name].cpu().view(torch.uint8), t.contiguous().view(torch.uint8)), name


def _after(case, specs, plain, verify):
    verify(plain)


@pytest.mark.parametrize('case', C.CASES, ids=IDS)
def test_poisoned_borders(ctx, case):
    borders.run_case(ctx, case, _after)


def test_refusals_launch_nothing(ctx):
    lib, st, p = ctx.lib, ctx.stream(), C.p
    segs, counts, meta = (t.cuda() for t in C.operands(3, 5, 0))
    ranks = torch.tensor([1, 5], dtype=torch.int32, device='cuda')
    threshs = torch.tensor([0.3, 0.5], dtype=torch.float64, device='cuda')
    table = torch.full((5,), 41, dtype=torch.int64, device='cuda')             # hits (2, 2), then n_queries
    best = torch.full((3, 2), UNWRITTEN, device='cuda')
    a = dict(segs=p(segs), counts=p(counts), meta=p(meta), nq=3, M=5, ranks=p(ranks), nr=2, threshs=p(threshs), nt=2, hits=p(table),
             n=p(table[4:]), best=p(best))
    odd = lambda t: ctypes.c_void_p(t.data_ptr() + 4)
    bad = [dict(segs=None), dict(counts=None), dict(meta=None), dict(ranks=None), dict(threshs=None), dict(hits=None), dict(n=None),
           dict(nq=-1), dict(M=0), dict(M=-3), dict(nr=0), dict(nr=9), dict(nt=0), dict(nt=9), dict(hits=odd(table)), dict(n=odd(table))]

    def run(k):
        return lib.dcf_op_recall_update(k['segs'], k['counts'], k['meta'], k['nq'], k['M'], k['ranks'], k['nr'], k['threshs'], k['nt'], k['hits'],
                                        k['n'], k['best'], st)

    for change in bad:
        assert run(dict(a, **change)) != 0, change
        msg = lib.dcf_last_error().decode()
        assert 'dcf_op_recall_update' in msg, (change, msg)
    assert run(dict(a, nq=0)) == 0                                              # nothing to count: success, nothing launched
    torch.cuda.synchronize()
    assert bool((table == 41).all()) and bool((best == UNWRITTEN).all())
    assert run(dict(a, best=None)) == 0                                         # best is optional
    torch.cuda.synchronize()
    want_hits, want_n = torch.full((2, 2), 41, dtype=torch.int64), torch.full((1,), 41, dtype=torch.int64)
    R.recall_update(segs.cpu(), counts.cpu(), meta.cpu(), (1, 5), (0.3, 0.5), want_hits, want_n)
    assert torch.equal(table[:4].cpu().view(2, 2), want_hits) and int(table[4]) == 44 and bool((best == UNWRITTEN).all())


def test_device_counter_accumulates_reads_and_resets():
    E = load_pkg().evaluator
    ranks, threshs = C.TABLES['r5t8']
    dc = E.DeviceRecallCounter(ranks, threshs)
    want_hits, want_n = torch.zeros(len(ranks), len(threshs), dtype=torch.int64), torch.zeros(1, dtype=torch.int64)
    for nq, M in ((65, 5), (3, 7)):
        segs, counts, meta = C.operands(nq, M, 1)
        best = torch.full((nq, len(ranks)), UNWRITTEN, device='cuda')
        dc.update_device(segs.cuda(), counts.cuda(), meta.cuda(), best=best)
        want_best = R.recall_update(segs, counts, meta, ranks, threshs, want_hits, want_n)
        assert torch.equal(R.bits(best.cpu()), R.bits(want_best))
    dc.add_misses(4)
    assert np.array_equal(dc.hits, want_hits.numpy()) and dc.hits.dtype == np.float64 and dc.n_queries == dc.text_cnt == 72
    assert np.array_equal(dc.counts, dc.hits) and np.array_equal(dc.metrics(), want_hits.numpy() / 72)
    host = E.RecallCounter(ranks, threshs)
    host.hits, host.n_queries = want_hits.numpy().astype(np.float64), 72
    assert dc.report() == host.report()
    assert dc.reset() is dc and dc.n_queries == 0 and not dc.hits.any() and np.array_equal(dc.metrics(), np.zeros((5, 8)))
    with pytest.raises(ValueError):
        E.DeviceRecallCounter(tuple(range(1, 10)), (0.5,))
