"""The cases of the evaluation-metric extension (include/decafnet_hip_eval.h, ``_lib.EVAL_TABLE``) for tests/test_gpu_eval_metric.py, in
the format of tests/abi_cases.py: ``Case(export, tag, make, options)`` with ``make()`` -> ``(specs, call, None, verify)``;
``verify(outputs)`` compares ``hits`` and ``n_queries`` as integers and ``best`` as bits with the restatement of
tests/eval_metric_ref.py -- integer sums and single fp32 operations have no tolerance.

``threshs`` is placed as the int64 bits of its float64 values (the arena has no float64 fill); ``hits`` and ``n_queries`` are ``inout``
operands pre-filled with non-zero values, ``best`` is an ``out`` operand.

Shapes: nq in {1, 3, 65, 257} (one lane; a few; across a 64-lane wave; across a 256-thread workgroup into a second one) times M in
{1, 5, 7} times two tables -- ranks (1, 5) with thresholds (0.3, 0.5), and ranks (1, 2, 3, 5, 8) with the eight thresholds 0.1 ... 0.8
(a rank above every M).  Rows beyond ``counts`` hold NaN and inf; from nq = 3 on one count lies above M and one is negative, which the
operator clamps.  Videos alternate between fps 30 and 29.97, vid_stride 1 and 2, and every fourth query block is not converted.  The
``x3`` cases make three consecutive calls into one table."""
import torch

import eval_metric_ref as R
from abi_cases import Case, gen, p

CASES = []
TABLES = {'r2t2': ((1, 5), (0.3, 0.5)), 'r5t8': ((1, 2, 3, 5, 8), tuple(round(0.1 * i, 1) for i in range(1, 9)))}
PREFILL_HITS, PREFILL_N = 1000, 77


def operands(nq, M, seed):
    """nq queries made of blocks of up to 16 with their own video constants"""
    g = gen(83, nq, M, seed)
    segs, counts, meta = [], [], []
    for b, q0 in enumerate(range(0, nq, 16)):
        v = R.random_video(g, min(16, nq - q0), M, vid_stride=1 + b % 2, fps=(30.0, 29.97)[(b // 2) % 2], convert=b % 4 != 3)
        segs.append(v['segs']), counts.append(v['counts']), meta.append(v['meta'])
    segs, counts, meta = torch.cat(segs), torch.cat(counts), torch.cat(meta)
    if nq >= 3:
        counts[1], counts[2] = M + 3, -2          # clamped to M (every row is live: no sentinel there) and to 0
        segs[1] = torch.nan_to_num(segs[1], nan=1.0, posinf=2.0)
    if nq >= 65:
        # an empty prediction against an empty ground truth (0 / 0: NaN, a miss everywhere) and IoU exactly 0.5, both in seconds
        for q, (pred, gt) in ((5, ((3., 3.), (3., 3.))), (6, ((0., 2.), (0., 1.)))):
            segs[q, 0], counts[q] = torch.tensor(pred), 1
            meta[q, :2], meta[q, 7] = torch.tensor(gt), 0.
    return segs, counts, meta


def recall(nq, M, table, times=1):
    def make():
        ranks, threshs = TABLES[table]
        segs, counts, meta = operands(nq, M, times)
        hits0 = torch.full((len(ranks), len(threshs)), PREFILL_HITS, dtype=torch.int64) + torch.arange(len(threshs))[None]
        n0 = torch.full((1,), PREFILL_N, dtype=torch.int64)
        want_hits, want_n = hits0.clone(), n0.clone()
        for _ in range(times):
            want_best = R.recall_update(segs, counts, meta, ranks, threshs, want_hits, want_n)
        specs = [('segs', segs.reshape(nq * M, 2), 'in'), ('counts', counts, 'in'), ('meta', meta, 'in'),
                 ('ranks', torch.tensor(ranks, dtype=torch.int32), 'in'), ('threshs', torch.tensor(threshs, dtype=torch.float64).view(torch.int64), 'in'),
                 ('hits', hits0, 'inout'), ('n_queries', n0, 'inout'), ('best', torch.zeros(nq, len(ranks)), 'out')]

        def call(c, v):
            for _ in range(times):
                rc = c.lib.dcf_op_recall_update(p(v['segs']), p(v['counts']), p(v['meta']), nq, M, p(v['ranks']), len(ranks), p(v['threshs']),
                                                len(threshs), p(v['hits']), p(v['n_queries']), p(v['best']), c.stream())
                if rc != 0:
                    return rc
            return 0

        def verify(got):
            assert torch.equal(got['hits'].cpu(), want_hits), f"hits {got['hits'].cpu().tolist()} want {want_hits.tolist()}"
            assert torch.equal(got['n_queries'].cpu(), want_n)
            assert torch.equal(R.bits(got['best'].cpu()), R.bits(want_best)), 'best differs from the restatement'
            assert int((want_hits - hits0).sum()) > 0 or nq < 65          # the case counts something
        return specs, call, None, verify
    return make


for table in TABLES:
    for nq in (1, 3, 65, 257):
        for M in (1, 5, 7):
            CASES.append(Case('dcf_op_recall_update', f'{table}-nq{nq}-M{M}', recall(nq, M, table), ()))
for table, nq, M in (('r2t2', 3, 5), ('r5t8', 257, 7), ('r5t8', 65, 1)):
    CASES.append(Case('dcf_op_recall_update', f'{table}-nq{nq}-M{M}-x3', recall(nq, M, table, times=3), ()))

EXCLUDED = {'dcf_eval_ext_version': 'no device operand: returns a constant'}
