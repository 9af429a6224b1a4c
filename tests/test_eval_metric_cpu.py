"""CPU checks that go with the evaluation-metric extension (include/decafnet_hip_eval.h, csrc/eval_metric.hip).

1. The declared boundary of the ``_lib.STAGED`` record: the table equals the header (tests/abi_headers.check_table), the built library
   exports the declared symbols and the version is 1, the source is part of the build, no name is shared with a table of
   ``EXTENSIONS`` / ``PENDING``, those two are what they were, and hipcc compiles the source without a warning under the project's flags.
2. The restatement of tests/eval_metric_ref.py against the package's own host arithmetic, which is pinned to the reference:
   ``GroundingEvaluator.finish_proposals`` for the seconds (bits), ``evaluator.iou`` for the best overlap per rank (bits, a NaN as the
   header's quiet NaN) and ``RecallCounter`` for the table (integers).  Scores are strictly decreasing: the operator defines no tie
   order and ``RecallCounter``'s argsort pins none."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import abi_headers as H
import eval_metric_ref as R
from conftest import load_pkg


# ---------------------------------------------------------------------------------------------- 1. the boundary
def test_staged_record_equals_its_header_and_the_library():
    pkg = load_pkg()
    L = pkg._lib
    assert len(L.STAGED) == 1
    ext = L.STAGED[0]
    assert ext == L.Extension('eval', 'decafnet_hip_eval.h', 'dcf_eval_ext_version', 1, 'DCF_EVAL_EXT_VERSION', ('decafnet_hip.h',), L.EVAL_TABLE)
    H.check_table(ext)
    assert sorted(ext.table) == ['dcf_eval_ext_version', 'dcf_op_recall_update']
    assert 'eval_metric.hip' in pkg.build.SOURCES and '-ffp-contract=off' in pkg.build.EXTRA['eval_metric.hip']
    h = ctypes.CDLL(pkg.build.build())
    for s in H.declared_symbols(ext.header):
        assert hasattr(h, s), f'{s} declared in include/{ext.header} but not exported'
    assert h.dcf_eval_ext_version() == 1


def test_source_compiles_without_warnings_under_the_project_flags(tmp_path):
    b = load_pkg().build
    cmd = [b.hipcc()] + b.FLAGS + b.EXTRA['eval_metric.hip'] + ['-c', os.path.join(b.CSRC, 'eval_metric.hip'), '-o', str(tmp_path / 'eval_metric.o')]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0 and 'warning' not in r.stderr and 'warning' not in r.stdout, r.stderr


def test_registry_and_pending_are_unchanged_and_share_no_name():
    L = load_pkg()._lib
    assert [e.key for e in L.EXTENSIONS] == ['base', 'train', 'dist', 'attn', 'front', 'guard', 'clock', 'half', 'front_half', 'embd']
    assert [e.key for e in L.PENDING] == ['batch']
    assert not [n for n in dir(L) if n.endswith('SIGNATURES') and getattr(L, n) is L.EVAL_TABLE]
    taken = {name for e in L.EXTENSIONS + L.PENDING for name in e.table}
    assert not taken & set(L.EVAL_TABLE)
    assert L.STAGED[0].key not in {e.key for e in L.EXTENSIONS + L.PENDING}
    assert L.STAGED[0].header not in {e.header for e in L.EXTENSIONS + L.PENDING}


# ---------------------------------------------------------------------------------------------- 2. the restatement
class _Done:
    def synchronize(self):
        pass


def host_route(pkg, v, ranks, threshs):
    """the parent commit's arithmetic on one video: finish_proposals on a packed host buffer, then RecallCounter -> (results, best, hits, n)"""
    E = pkg.evaluator
    ev = object.__new__(E.GroundingEvaluator)
    ev.vid_stride, ev._pinned = v['vid_stride'], {}
    nq, M = v['segs'].shape[:2]
    counts = v['counts'].clamp(0, M)
    scores = torch.arange(M, 0, -1, dtype=torch.float32)[None].expand(nq, M) / (M + 1)          # strictly decreasing
    packed = torch.cat((v['segs'].reshape(nq, 2 * M), scores, counts[:, None].float()), 1)
    data = dict(clip_stride=v['clip_stride'], clip_size=v['clip_size'], fps=v['fps'], duration=v['duration']) if v['convert'] else None
    results = ev.finish_proposals(('packed', _Done(), packed, nq, M, data))
    counter = E.RecallCounter(ranks, threshs)
    counter.update(results, v['gt'])
    best = torch.zeros(nq, len(ranks))
    for q, res in enumerate(results):
        ov = E.iou(res['segments'], torch.as_tensor(v['gt'][q], dtype=torch.float32)[None])
        for i, k in enumerate(ranks):
            if len(ov[:k]):
                best[q, i] = R.QNAN if bool(torch.isnan(ov[:k]).any()) else ov[:k].max()
    return results, best, counter.hits, counter.n_queries


def compare(pkg, v, ranks, threshs):
    nq, M = v['segs'].shape[:2]
    results, best, hits, n = host_route(pkg, v, ranks, threshs)
    secs = R.to_seconds(v['segs'], v['meta'])
    for q, res in enumerate(results):
        k = len(res['segments'])
        assert k == min(max(int(v['counts'][q]), 0), M)
        assert torch.equal(R.bits(secs[q, :k]), R.bits(res['segments'])), f'seconds of query {q}'
    got_hits, got_n = torch.zeros(len(ranks), len(threshs), dtype=torch.int64), torch.zeros(1, dtype=torch.int64)
    got_best = R.recall_update(v['segs'], v['counts'], v['meta'], ranks, threshs, got_hits, got_n)
    assert torch.equal(R.bits(got_best), R.bits(best)), 'best'
    assert np.array_equal(got_hits.numpy(), hits.astype(np.int64)) and np.array_equal(hits, hits.astype(np.int64)), 'hits'
    assert int(got_n) == n == nq
    return got_best, got_hits


RANKS, THRESHS = (1, 2, 3, 5, 8), tuple(round(0.1 * i, 1) for i in range(1, 9))


@pytest.mark.parametrize('fps', [30.0, 29.97])
@pytest.mark.parametrize('vid_stride', [1, 2])
@pytest.mark.parametrize('convert', [True, False])
def test_restatement_equals_the_host_route(fps, vid_stride, convert):
    pkg = load_pkg()
    g = torch.Generator().manual_seed(int(fps * 100) + 7 * vid_stride + convert)
    for M in (1, 5, 7):                                   # ranks 8 > M always, 5 > M once; counts from 0 to M: count == 0, count < k
        v = R.random_video(g, 40, M, vid_stride=vid_stride, fps=fps, convert=convert, sentinels=False)
        best, hits = compare(pkg, v, RANKS, THRESHS)
        assert int((v['counts'] == 0).sum()) > 0 and bool((best[v['counts'] == 0] == 0).all())
        if convert:                                       # the clamps at 0 and at the duration both bite
            secs = R.to_seconds(v['segs'], v['meta'])
            assert bool((secs == 0).any()) and bool((secs == v['meta'][0, 6]).any())
        assert 0 < int(hits.sum()) < hits.numel() * 40
    assert torch.equal(torch.from_numpy(pkg.evaluator.query_meta(v['gt'], vid_stride, 16, 16, fps, v['duration'], convert)), v['meta'])


def test_reciprocal_multiply_would_differ():
    """the fps cases mean something: at 29.97 a multiply by 1 / fps gives other bits than the division for some row"""
    g = torch.Generator().manual_seed(5)
    v = R.random_video(g, 40, 5, fps=29.97, sentinels=False)
    m = v['meta'][:, None, :]
    x = v['segs'] * m[..., 2:3] * m[..., 3:4] + m[..., 4:5]
    assert not torch.equal(R.bits(x / m[..., 5:6]), R.bits(x * (1.0 / m[..., 5:6])))


def test_exact_half_is_a_hit_and_empty_against_empty_is_a_miss():
    pkg = load_pkg()
    # pred [0, 2] against gt [0, 1]: IoU exactly 0.5, a hit at 0.5; pred [3, 3] against gt [3, 3]: 0 / 0, a miss everywhere
    segs = torch.tensor([[[0., 2.]], [[3., 3.]]])
    v = dict(segs=segs, counts=torch.tensor([1, 1], dtype=torch.int32), gt=np.array([[0., 1.], [3., 3.]]),
             meta=R.meta_rows([[0., 1.], [3., 3.]], 1, 16, 16, 30.0, 10.0, convert=False), vid_stride=1, clip_stride=16, clip_size=16, fps=30.0,
             duration=10.0, convert=False)
    best, hits = compare(pkg, v, (1, 5), (0.3, 0.5, 0.5000001))
    assert float(best[0, 0]) == 0.5 and bool(torch.isnan(best[1]).all())
    assert hits.tolist() == [[1, 1, 0], [1, 1, 0]]
