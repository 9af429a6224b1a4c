"""tests/postproc_ref.py pinned on the CPU: the reference side of the post-processing GPU tests against the reference's own fixtures,
the max_iters prefix rule against a restated loop, and the conditions the GPU tests' inputs rest on."""
import pytest
import torch

import postproc_ref as PR
from conftest import Golden
from postproc_ref import R


def test_vote64_reproduces_the_voted_fixture_configurations():
    """R.batched_nms with vote64 in place of its voting == the reference's voted results (postproc.npz) within 1e-5 (relative)"""
    g = Golden('postproc.npz')
    segs, scores = g.t('segs'), g.t('scores')
    cfgs = g.js('nms_cfgs')
    seen = 0
    for k in ('soft_default', 'hard_vote'):
        cfg = dict(cfgs[k])
        assert cfg['voting_thresh'] > 0
        picks, pick_scores = R.batched_nms(segs.clone(), scores.clone(), **dict(cfg, voting_thresh=0.0))
        voted = PR.vote64(picks, segs, scores, cfg['voting_thresh'])
        assert voted.dtype == torch.float64
        # batched_nms ends with a stable descending argsort of the picks' scores: the identity on picks in pick order
        assert torch.equal(pick_scores.argsort(descending=True, stable=True), torch.arange(len(pick_scores)))
        torch.testing.assert_close(pick_scores, g.t(f'{k}/scores'), rtol=0, atol=1e-6)
        # 1e-5 RELATIVE: the fixture is fp32 and its segments lie near 1000, where one fp32 step is 6e-5
        torch.testing.assert_close(voted, g.t(f'{k}/segs').double(), rtol=1e-5, atol=0)
        torch.testing.assert_close(PR.vote32(picks, segs, scores, cfg['voting_thresh']), g.t(f'{k}/segs'), rtol=1e-5, atol=0)
        seen += 1
    assert seen == 2


def test_expectations_reproduce_the_known_answers_at_one_query():
    g = Golden('nms_kat.npz')
    for i, c in enumerate(g.js('cases')):
        segs, scores = g.t(f'k{i}/segs'), g.t(f'k{i}/scores')
        n = len(scores)
        segs_b, scores_b = segs.reshape(1, n, 2), scores.reshape(1, n)
        for counts in (None, torch.tensor([n], dtype=torch.int32)):
            (keep,) = PR.expect_nms(segs_b, scores_b, counts, n, c['iou_thresh'])
            assert torch.equal(keep, g.t(f'k{i}/nms')), c
            for method in (0, 1, 2):
                ((dets, inds),) = PR.expect_softnms(segs_b, scores_b, counts, n, c['iou_thresh'], c['sigma'], c['min_score'], method)
                assert torch.equal(inds, g.t(f'k{i}/soft{method}/idx')), (c, method)
                assert torch.equal(dets, g.t(f'k{i}/soft{method}/dets')), (c, method)


def test_counts_select_the_live_part():
    """counts above n_max are clamped, counts below cut the row, NaN / inf behind the live part are never read"""
    g = PR.gen(5)
    segs, scores = PR.grid_segments(30, g)[None].clone(), PR.quantised_scores(30, 4, g)[None].clone()
    segs[0, 20:], scores[0, 20:] = float('nan'), float('inf')
    (a,) = PR.expect_nms(segs, scores, torch.tensor([20]), 25, 0.3)
    (b,) = PR.expect_nms(segs[:, :20], scores[:, :20], None, 20, 0.3)
    assert torch.equal(a, b) and len(a) > 0
    (c,) = PR.expect_nms(segs[:, :20], scores[:, :20], torch.tensor([700]), 12, 0.3)
    (d,) = PR.expect_nms(segs[:, :12], scores[:, :12], None, 12, 0.3)
    assert torch.equal(c, d)


@pytest.mark.parametrize('trial', range(20))
def test_max_iters_is_a_prefix_of_the_full_run(trial):
    """expect_softnms's rule for max_iters > 0 (the first min(m, k_full) rows of the full run) against a straight restatement of the
    reference's loop that really stops after m picks: tie-heavy inputs, all three methods, prunings of one and of several segments"""
    g = PR.gen(7, trial)
    n = int(torch.randint(2, 41, (1,), generator=g))
    segs = PR.grid_segments(n, g, degenerate=trial % 4 == 3, span=6)
    scores = PR.quantised_scores(n, (4, 16, 64)[trial % 3], g)
    thr = (0.1, 0.3, 0.5)[trial % 3]
    pruned = 0
    for method in (0, 1, 2):
        for ms in (0.001, 0.2, 0.45):
            ((d_full, i_full),) = PR.expect_softnms(segs[None], scores[None], None, n, thr, 0.5, ms, method)
            pruned += len(i_full) < n
            for m in (0, 1, 2, 5, len(i_full), n + 7):
                ((d, i),) = PR.expect_softnms(segs[None], scores[None], None, n, thr, 0.5, ms, method, max_iters=m)
                d2, i2 = PR.softnms_early_stop(segs, scores, thr, 0.5, ms, method, m)
                assert torch.equal(i, i2), (n, method, ms, m)
                assert torch.equal(d, d2), (n, method, ms, m)
                assert len(i) == (len(i_full) if m <= 0 else min(m, len(i_full)))
    assert pruned > 0


def test_generators_are_on_their_grids():
    g = PR.gen(11)
    s = PR.grid_segments(500, g, degenerate=True)
    assert torch.equal(s * 4, torch.round(s * 4))
    ln = s[:, 1] - s[:, 0]
    assert (ln == 0).any() and (ln < 0).any() and ln.abs().max() < 32
    assert len(torch.unique(s, dim=0)) < len(s)                                   # duplicates
    for levels in (4, 16, 64):
        c = PR.signed_scores(300, levels, g)
        assert torch.equal(c * levels, torch.round(c * levels)) and (c < 0).any() and (c > 0).any() and not torch.isnan(c).any()
        z = (c == 0).nonzero().flatten()
        neg = torch.signbit(c[z])
        assert neg.any() and (~neg).any() and int(z[neg].min()) < int(z[~neg].max())
        assert torch.signbit(c[0]) and c[0] == 0 and not torch.signbit(c[-1]) and c[-1] == 0
    lg = PR.grid_logits((2, 5000), g)
    assert torch.equal(lg * 16, torch.round(lg * 16)) and lg.min() >= -8 and lg.max() <= 4
    of = PR.grid_offsets((2, 5000), g)
    assert torch.equal(of * 8, torch.round(of * 8)) and of.min() >= 0 and of.max() <= 5 and of.shape == (2, 5000, 2)


@pytest.mark.parametrize('n2,ld,thr', PR.voting_cases())
def test_every_voting_input_keeps_its_margin(n2, ld, thr):
    """|iou64 - thr| is exactly 0 or >= 1e-4 for every survivor / candidate pair of every voting input the GPU tests use; survivor 1 of
    every query with more than one survivor gets no vote (a NaN row in the reference)"""
    case = PR.voting_case(n2, ld, thr)
    exp = PR.voting_expect(case)
    for q in range(case['nq']):
        k, m = int(case['c1'][q]), int(case['c2'][q])
        assert 0 <= k <= case['n1'] <= case['n1_stride'] and 1 <= m <= case['n2'] < case['n2_stride']
        live = case['nms'][q, :k, :2]
        assert not torch.isnan(live).any() and not torch.isnan(case['all_segs'][q, :m]).any()
        if k:
            assert PR.voting_margin(live, case['all_segs'][q, :m], thr) >= PR.MARGIN, (q, PR.voting_margin(live, case['all_segs'][q, :m], thr))
        y64, y32 = exp[q]
        assert y64.dtype == torch.float64 and y32.dtype == torch.float32 and y64.shape == (k, 2)
        nan = torch.isnan(y64)
        assert torch.equal(nan, torch.isnan(y32))
        if k:
            assert not nan[0].any()                        # survivor 0 is a candidate: it votes for itself at least
        if k > 1:
            assert nan[1].all() and not nan[2::2].any()    # even rows are candidates too; a moved (odd) one may lose every vote at 0.95


# Recorded when the seeds were fixed (the inputs are seeded), per query: candidates above pre_nms_thresh, cut, size of the group of equal scores
# the cut falls into, members of it the cut leaves out, kept after the length filter.  The test prints the same figures.
#
#   | input              | query | candidates | cut at | tie group at the cut | left out | kept after length filter |
#   |--------------------|-------|------------|--------|----------------------|----------|--------------------------|
#   | reread-q2-bitonic  | 0     | 47 343     | 4000   | 224                  | 172      | 3425                     |
#   | reread-q2-bitonic  | 1     | 48 825     | 4000   | 214                  | 196      | 3405                     |
#   | cached-32768       | 0     | 31 574     | 2000   | 116                  | 2        | 1601                     |
#   | cached-32768       | 1     | 32 552     | 2000   | 109                  | 28       | 1580                     |
#   | reread-32769       | 0     | 31 574     | 2048   | 137                  | 57       | 2047                     |
#   | masked-query       | 0     | 63         | 50     | 1                    | 0        | 50                       |
#   | masked-query       | 1     | 63         | 50     | 2                    | 1        | 50                       |
#   | masked-query       | 2     | 0          | 0      | -                    | -        | 0                        |
#   | thresh-0.3         | 0     | 8 995      | 2000   | 120                  | 104      | 1628                     |
#   | thresh-0.3         | 1     | 9 258      | 2000   | 126                  | 77       | 1608                     |


@pytest.mark.parametrize('name', list(PR.COLLECT))
def test_every_collect_input_has_ties_at_the_cut(name):
    """for at least one query of every collect input the top-k cut runs through a group of equal scores (more than one candidate tied
    at the cut, some taken and some left out): the order inside that group -- lower candidate index first -- decides what is emitted"""
    figs = PR.collect_figures(name)
    print(name, figs)
    assert any(grp > 1 and 0 < left_out < grp for _, _, grp, left_out, _ in figs), figs
    c = PR.collect_case(name)
    if name == 'masked-query':
        assert figs[-1][0] == 0 and figs[0][0] > 0 and not c['masks'][-1].any()
    if name == 'reread-32769':
        assert c['S'] == 32769 and figs[0][1] == 2048
    if name == 'cached-32768':
        assert c['S'] == 32768
    if name == 'reread-q2-bitonic':
        assert c['S'] == 49152 and all(f[1] == 4000 for f in figs)
        # the length filter drops candidates in every 1024-candidate chunk of the decode loop
        assert all(f[4] < 3600 for f in figs)
