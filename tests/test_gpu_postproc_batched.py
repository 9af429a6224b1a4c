"""The post-processing kernels (csrc/postproc.hip: k_collect, k_nms, k_softnms, k_voting) in the form production calls them -- several
queries per launch, a counts vector, rows longer than their live part, max_iters set -- and on the branches no other test reaches, each
against the CPU oracles through tests/postproc_ref.py.  Indices, dets and decoded segments are compared EXACTLY; the voting's fp32 sums
go by the project's parity rule against the oracle in fp64.  The reference side never sees anything the GPU returned.  GPU only."""
import ctypes

import pytest
import torch

import forward_parity as FP
import postproc_ref as PR
from conftest import load_pkg

pytestmark = pytest.mark.gpu

THR, SIGMA = 0.3, 0.5
KEEP_SENTINEL, DETS_SENTINEL, COUNT_SENTINEL = -777, -7.0, -5


@pytest.fixture(scope='module')
def L():
    pkg = load_pkg()
    lib = pkg._lib.lib()          # raises if the .so is missing: no silent fallback
    return pkg, lib


_KEEP = []


def P(t):
    """device address; the tensor is kept alive until the kernels that read it have run"""
    _KEEP.append(t)
    if len(_KEEP) > 256:
        torch.cuda.synchronize()
        del _KEEP[:128]
    return ctypes.c_void_p(t.data_ptr())


def st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------ launches
def run_nms(L, segs, scores, counts, n_max, thr):
    """dcf_nms_1d on CPU tensors segs (nq, stride, 2), scores (nq, stride), counts (nq) or None: (keep, keep_counts) back on the CPU,
    pre-filled with sentinels"""
    pkg, lib = L
    nq, stride = scores.shape
    keep = torch.full((nq, stride), KEEP_SENTINEL, dtype=torch.int64).cuda()
    kc = torch.full((nq,), COUNT_SENTINEL, dtype=torch.int32).cuda()
    cp = P(counts.to(torch.int32).cuda()) if counts is not None else None
    pkg._lib.check(lib.dcf_nms_1d(P(segs.cuda()), P(scores.cuda()), cp, nq, n_max, stride, float(thr), P(keep), P(kc), st()), 'dcf_nms_1d')
    return keep.cpu(), kc.cpu()


def run_softnms(L, segs, scores, counts, n_max, thr, sigma, min_score, method, max_iters):
    pkg, lib = L
    nq, stride = scores.shape
    dets = torch.full((nq, stride, 3), DETS_SENTINEL).cuda()
    inds = torch.full((nq, stride), KEEP_SENTINEL, dtype=torch.int64).cuda()
    oc = torch.full((nq,), COUNT_SENTINEL, dtype=torch.int32).cuda()
    cp = P(counts.to(torch.int32).cuda()) if counts is not None else None
    pkg._lib.check(lib.dcf_softnms_1d(P(segs.cuda()), P(scores.cuda()), cp, nq, n_max, stride, float(thr), float(sigma), float(min_score), int(method),
                                      int(max_iters), P(dets), P(inds), P(oc), st()), 'dcf_softnms_1d')
    return dets.cpu(), inds.cpu(), oc.cpu()


def assert_nms(tag, keep, kc, want):
    for q, w in enumerate(want):
        k = len(w)
        assert int(kc[q]) == k, (tag, q, int(kc[q]), k)
        assert torch.equal(keep[q, :k], w), (tag, q, (keep[q, :k] != w).nonzero()[:4].flatten().tolist())
        assert bool((keep[q, k:] == KEEP_SENTINEL).all()), (tag, q, 'written behind keep_counts')


def assert_softnms(tag, dets, inds, oc, want):
    for q, (wd, wi) in enumerate(want):
        k = len(wi)
        assert int(oc[q]) == k, (tag, q, int(oc[q]), k)
        assert torch.equal(inds[q, :k], wi), (tag, q, (inds[q, :k] != wi).nonzero()[:4].flatten().tolist())
        assert torch.equal(dets[q, :k], wd), (tag, q, int((dets[q, :k] != wd).sum()))
        assert bool((inds[q, k:] == KEEP_SENTINEL).all()) and bool((dets[q, k:] == DETS_SENTINEL).all()), (tag, q, 'written behind out_counts')


def check_all(L, tag, segs, scores, counts, n_max, thr, min_scores, max_iters=(0,), methods=(0, 1, 2), hard=True):
    """hard NMS and the soft methods of one batched input against the oracle, query by query"""
    if hard:
        keep, kc = run_nms(L, segs, scores, counts, n_max, thr)
        assert_nms((tag, 'hard'), keep, kc, PR.expect_nms(segs, scores, counts, n_max, thr))
    for method in methods:
        for ms in min_scores:
            full = PR.expect_softnms_full(segs, scores, counts, n_max, thr, SIGMA, ms, method)
            for m in max_iters:
                dets, inds, oc = run_softnms(L, segs, scores, counts, n_max, thr, SIGMA, ms, method, m)
                assert_softnms((tag, 'soft', method, ms, m), dets, inds, oc, [PR.softnms_prefix(d, i, m) for d, i in full])


# ------------------------------------------------------------------------------------------------ 3a: over queries
#        nq  n_max stride counts
ROWS = [(5, 600, 640, [600, 3, 0, 257, 1]),          # 256-thread soft NMS, an empty row and rows of one and three
        (1, 600, 700, [700]),                        # a count above n_max is clamped
        (3, 800, 800, [1, 64, 800]),                 # 512-thread kernel with 1 and 64 live rows
        (3, 3100, 3100, [5, 3100, 769]),             # 1024-thread kernel; four keys per lane in the sort
        (3, 4096, 4096, [4096, 2, 1025]),            # the LDS capacity
        (3, 4100, 4104, [4100, 70, 0])]              # global scratch with q > 0


def batched_input(kind, nq, n_max, stride, counts):
    """rows of `stride`; the live part [0, min(count, n_max)) from the generators, everything else -- rows behind the count and the
    columns n_max .. stride -- NaN segments and +inf scores, which must not matter"""
    g = PR.gen(43, nq, n_max, stride, kind == 'ties')
    segs = torch.full((nq, stride, 2), float('nan'))
    scores = torch.full((nq, stride), float('inf'))
    for q in range(nq):
        n = min(counts[q], n_max)
        if n == 0:
            continue
        if kind == 'ties':
            segs[q, :n], scores[q, :n] = PR.grid_segments(n, g), PR.quantised_scores(n, (16, 4, 64)[q % 3], g)
        else:
            segs[q, :n], scores[q, :n] = PR.continuous_case(n, g)
    return segs, scores


@pytest.mark.parametrize('kind', ['ties', 'continuous'])
@pytest.mark.parametrize('nq,n_max,stride,counts', ROWS, ids=[f'{r[0]}x{r[1]}-ld{r[2]}' for r in ROWS])
def test_nms_over_queries_vs_oracle(L, nq, n_max, stride, counts, kind):
    """dcf_nms_1d / dcf_softnms_1d with nq > 1, a counts vector and stride >= n_max against the C oracle run per query on
    row[:min(count, n_max)]: counts, index prefixes and dets exact, the sentinel intact behind every count.  Would trip on: a wrong
    per-query offset of rows or of the global scratch (`q * scratch_per_q`: the queries' keys would mix -- rows 4100 x 3), a missing
    clamp of counts to n_max (row 2: the NaN / inf columns would be read), a max_iters that is not the pick count (out_counts and the
    sentinel check), the thread-count choice by n_max with a handful of live candidates (rows 3 and 4)."""
    segs, scores = batched_input(kind, nq, n_max, stride, counts)
    check_all(L, (nq, n_max, stride, kind), segs, scores, torch.tensor(counts), n_max, THR, min_scores=(0.2 if kind == 'ties' else 0.05,),
              max_iters=(0, 1, 5, n_max + 7))


# ------------------------------------------------------------------------------------------------ 3b: branches at one query
def one_query(segs, scores):
    return segs[None].contiguous(), scores[None].contiguous()


@pytest.mark.parametrize('thr', [0.0, -0.5])
def test_nonpositive_iou_thresh(L, thr):
    """iou_thresh <= 0: `0 >= thr` holds, so pairs that do not overlap suppress / decay each other too -- the `nonpos_thr` branch of
    k_nms and `all_touch` of k_softnms, which skip the division for disjoint pairs otherwise"""
    for n in (2, 5, 70, 300, 1100):
        g = PR.gen(44, n, int(thr * 10))
        for tag, (segs, scores) in (('ties', (PR.grid_segments(n, g, degenerate=True), PR.quantised_scores(n, 16, g))),
                                    ('continuous', PR.continuous_case(n, g))):
            s, c = one_query(segs, scores)
            check_all(L, ('thr', thr, n, tag), s, c, None, n, thr, min_scores=(-2.0, 0.0, 0.2), max_iters=(0, 3))


@pytest.mark.parametrize('levels', [4, 16, 64])
def test_signed_scores(L, levels):
    """scores of both signs and both zeros: the negative half of the sort keys (fkey, snms_key), -0.0 == +0.0 in every comparison,
    min_score <= 0 in soft NMS (nothing or only negative scores pruned; a negative score decays UPWARDS)"""
    for n in (2, 3, 37, 300, 900, 3100):
        g = PR.gen(45, n, levels)
        s, c = one_query(PR.grid_segments(n, g, degenerate=n == 300), PR.signed_scores(n, levels, g))
        check_all(L, ('signed', levels, n), s, c, None, n, THR, min_scores=(-2.0, 0.0, 0.2), max_iters=(0,) if n > 900 else (0, 4))


def test_degenerate_segments(L):
    """zero-length, reversed, duplicated and nested segments: unions of 1e-6, negative areas, IoU of exactly 1"""
    for n in (9, 64, 65, 500, 1500):
        for levels in (4, 64):
            g = PR.gen(46, n, levels)
            s, c = one_query(PR.grid_segments(n, g, degenerate=True, span=4 + n // 12), PR.quantised_scores(n, levels, g))
            check_all(L, ('degenerate', levels, n), s, c, None, n, THR, min_scores=(0.001, 0.2), max_iters=(0, n + 7))


TIE_SIZES = (1, 2, 63, 64, 65, 128, 129, 768, 769, 1024, 1025, 2048, 2049, 3072, 3073, 4095, 4096, 4097)


@pytest.mark.parametrize('levels', [4, 16, 64])
def test_hard_nms_tie_fuzz(L, levels):
    """a few score levels over up to 4097 candidates: long runs of equal keys through every exchange kind of the register bitonic
    network -- lanes, registers of a lane, LDS between waves -- in its three widths (1 / 2 / 4 keys per lane: n <= 1024 / 2048 / 4096)
    and through the global-memory network (4097).  "Lower index first" among equal scores decides which of two overlapping segments is
    kept, so a single exchange that forgets the index half of the key changes the kept list."""
    for n in TIE_SIZES:
        g = PR.gen(47, n, levels)
        s, c = one_query(PR.grid_segments(n, g), PR.quantised_scores(n, levels, g))
        keep, kc = run_nms(L, s, c, None, n, THR)
        assert_nms(('tie fuzz', levels, n), keep, kc, PR.expect_nms(s, c, None, n, THR))


def test_negative_zero_sorts_with_positive_zero(L):
    """two disjoint segments with scores [-0.0, +0.0]: equal scores, so index order -- [0, 1] -- as the oracle's stable sort
    ("take right only if strictly greater") and at::sort have it.  (fkey mapped -0.0 strictly below +0.0 and k_nms returned [1, 0].)"""
    segs = torch.tensor([[[0.0, 1.0], [10.0, 11.0]]])
    scores = torch.tensor([[-0.0, 0.0]])
    assert bool(torch.signbit(scores[0, 0])) and not bool(torch.signbit(scores[0, 1]))
    (want,) = PR.expect_nms(segs, scores, None, 2, 0.5)
    assert want.tolist() == [0, 1]
    keep, kc = run_nms(L, segs, scores, None, 2, 0.5)
    assert int(kc[0]) == 2 and keep[0].tolist() == [0, 1], (int(kc[0]), keep[0].tolist())
    keep, kc = run_nms(L, segs, -scores, None, 2, 0.5)          # [+0.0, -0.0]: the same order
    assert int(kc[0]) == 2 and keep[0].tolist() == [0, 1]


# ------------------------------------------------------------------------------------------------ 3c: voting
def test_voting_vs_fp64(L):
    """dcf_segment_voting against the oracle's segment_voting in fp64 by the project's rule, e_gpu <= max(4 e_ref, 2^-21 max |y64|) with
    e_ref the fp32 oracle's error, POOLED over all cases: n2 in {1, 63, 64, 65, 777, 2000, 4099} (the 64-lane tail), ld 2 and 3,
    thresholds 0.75 and 0.95, three queries with their own n1_counts / n2_counts in rows longer than the counts (NaN / inf behind
    them).  A survivor nothing votes for is NaN on both sides, elementwise; rows at or behind n1_counts[q] keep the sentinel.
    Would trip on: a tail that drops or repeats candidates of the last partial 64-group (the sums change by whole votes), a wrong
    per-query offset, counts not honoured (NaN in the sums)."""
    pkg, lib = L
    got_all, y64_all, y32_all = [], [], []
    for n2, ld, thr in PR.voting_cases():
        case = PR.voting_case(n2, ld, thr)
        nq, n1, n1s = case['nq'], case['n1'], case['n1_stride']
        out = torch.full((nq, n1s, 2), DETS_SENTINEL).cuda()
        pkg._lib.check(lib.dcf_segment_voting(P(case['nms'].cuda()), ld, P(case['c1'].cuda()), n1, n1s, P(case['all_segs'].cuda()),
                                              P(case['all_scores'].cuda()), P(case['c2'].cuda()), n2, case['n2_stride'], float(thr), nq,
                                              P(out), st()), 'dcf_segment_voting')
        out = out.cpu()
        g_c, y64_c, y32_c = [], [], []
        for q, (y64, y32) in enumerate(PR.voting_expect(case)):
            k = int(case['c1'][q])
            assert bool((out[q, k:] == DETS_SENTINEL).all()), (n2, ld, thr, q, 'written at or behind n1_counts')
            nan = torch.isnan(y64)
            assert torch.equal(torch.isnan(out[q, :k]), nan), (n2, ld, thr, q)
            g_c.append(out[q, :k][~nan]); y64_c.append(y64[~nan]); y32_c.append(y32[~nan])
        g_c, y64_c, y32_c = torch.cat(g_c), torch.cat(y64_c), torch.cat(y32_c)
        top, e_ref, e_gpu, bound, ratio = FP.rule(g_c, y64_c, y32_c)
        print(f'VOTEERR n2 {n2} ld {ld} thr {thr}: n {len(g_c)} max|y64| {top:.3e} e_ref {e_ref:.3e} e_gpu {e_gpu:.3e} own bound {bound:.3e}')
        got_all.append(g_c); y64_all.append(y64_c); y32_all.append(y32_c)
    FP.check('voting, pooled', torch.cat(got_all), torch.cat(y64_all), torch.cat(y32_all))


# ------------------------------------------------------------------------------------------------ 3d: collect
@pytest.mark.parametrize('name', list(PR.COLLECT))
def test_collect_exact_vs_oracle(L, name):
    """dcf_collect_segments on grid logits and offsets against the oracle's collect_segments per query: the count, the ORDER and the
    segments exact (atol 0), the scores at rtol 1e-6.  Every top-k cut runs through a group of equal scores (asserted on the CPU,
    tests/test_postproc_ref_cpu.py), so which candidates are emitted hangs on "lower index first" in the selection and in the sort;
    a wrong per-query offset of the re-read keys (`q * S`) would select query 1's candidates by query 0's scores."""
    pkg, lib = L
    c = PR.collect_case(name)
    nq, topk = c['nq'], c['topk']
    segs = torch.full((nq, topk, 2), DETS_SENTINEL).cuda()
    scores = torch.full((nq, topk), DETS_SENTINEL).cuda()
    counts = torch.full((nq,), COUNT_SENTINEL, dtype=torch.int32).cuda()
    pkg._lib.check(lib.dcf_collect_segments(P(c['logits'].cuda()), P(c['offsets'].cuda()), P(c['masks'].cuda()), nq, c['T0'], c['Lv'],
                                            float(c['pre_nms_thresh']), topk, float(c['seg_len_thresh']), P(segs), P(scores), P(counts), st()),
                   'dcf_collect_segments')
    segs, scores, counts = segs.cpu(), scores.cpu(), counts.cpu()
    for q, (ws, wc) in enumerate(PR.collect_expect(name)):
        n = len(wc)
        assert int(counts[q]) == n, (name, q, int(counts[q]), n)
        torch.testing.assert_close(segs[q, :n], ws, rtol=0, atol=0)
        torch.testing.assert_close(scores[q, :n], wc, rtol=1e-6, atol=0)
        assert bool((segs[q, n:] == DETS_SENTINEL).all()) and bool((scores[q, n:] == DETS_SENTINEL).all()), (name, q, 'written behind counts')
