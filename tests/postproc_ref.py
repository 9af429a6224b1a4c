"""The reference side and the inputs of the post-processing tests (a helper module, CPU only; shared by tests/test_postproc_ref_cpu.py,
tests/test_gpu_postproc_batched.py and the several-query block of tests/test_gpu_ops.py).

Nothing here touches the GPU or anything the GPU returned.  The expectations are the C oracle (oracle/nms_ref.c through
oracle/nms_oracle.py) query by query, and the torch oracle (oracle/decafnet_ref.py) in fp32 and on fp64 casts.

All inputs sit on GRIDS so that every decision a kernel takes is exact and does not hang on the last bit of an fp32 quotient:

* segments: centres and lengths are multiples of 0.25 (`grid_segments`); lengths stay below 32, where `(r - l) + 1e-6f` still differs
  from `r - l` in fp32, so no union is exactly zero;
* scores: 4 / 16 / 64 levels (`quantised_scores`), with both signs and both zeros in `signed_scores`;
* logits: `round((randn * 2 - 2) * 16) / 16` in [-8, 4] (`grid_logits`): at most 193 distinct scores, so every top-k cut runs through a
  group of equal scores;
* offsets: multiples of 1/8 in [0, 5] (`grid_offsets`): `ctr -+ off * stride` and the length filter are exact in fp32.

The inputs of the GPU tests are built by `voting_case` / `collect_case` from fixed seeds, so that the CPU test can assert the conditions
they rest on (the voting margin, a tie group at every top-k cut) on the very tensors the GPU tests feed.
"""
import functools
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import decafnet_ref as R  # noqa: E402
from oracle import nms_oracle  # noqa: E402

MARGIN = 1e-4          # every survivor / candidate pair of a voting input has |iou64 - thr| == 0 or >= MARGIN


def gen(*seed):
    s = 0
    for v in seed:
        s = (s * 1000003 + int(v)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


# ------------------------------------------------------------------------------------------------ generators
def grid_segments(n, g, degenerate=False, span=None):
    """(n, 2) segments, centres and lengths multiples of 0.25 (lengths 0.25 .. 12).  `degenerate` adds, one in eight each, zero-length
    segments, reversed ones (right < left), exact duplicates of an earlier segment and segments nested inside an earlier one."""
    span = span if span is not None else 8 + n // 6
    c = torch.randint(0, 4 * span + 1, (n,), generator=g).float() / 4
    ln = torch.randint(1, 49, (n,), generator=g).float() / 4
    left, right = c - ln / 2, c + ln / 2                     # multiples of 0.125: still exact
    left, right = torch.round(left * 4) / 4, torch.round(right * 4) / 4
    right = torch.maximum(right, left + 0.25)
    if degenerate and n >= 2:
        kind = torch.randint(0, 8, (n,), generator=g)
        src = (torch.rand(n, generator=g) * torch.arange(n)).long()          # an earlier index (0 for i = 0)
        for i in range(1, n):
            k, j = int(kind[i]), int(src[i])
            if k == 0:
                right[i] = left[i]
            elif k == 1:
                left[i], right[i] = right[i].clone(), left[i].clone()
            elif k == 2:
                left[i], right[i] = left[j], right[j]
            elif k == 3 and right[j] - left[j] >= 0.75:
                left[i], right[i] = left[j] + 0.25, right[j] - 0.25
    return torch.stack((left, right), -1).contiguous()


def quantised_scores(n, levels, g):
    """positive scores on `levels` levels in (0, 1]: heavy ties"""
    return (torch.randint(1, levels + 1, (n,), generator=g).float() / levels).contiguous()


def signed_scores(n, levels, g):
    """scores k / levels, k in [-levels, levels]: both signs, and both zeros -- the zeros alternate -0.0, +0.0, ... in index order (and
    positions 0 and n - 1 are made -0.0 / +0.0 for n >= 2), so that a -0.0 always has a lower index than a +0.0.  No NaN."""
    s = torch.randint(-levels, levels + 1, (n,), generator=g).float() / levels
    if n >= 2:
        s[0], s[n - 1] = 0.0, 0.0
    zeros = (s == 0).nonzero().flatten().tolist()
    for k, i in enumerate(zeros):
        s[i] = -0.0 if k % 2 == 0 else 0.0
    if n >= 2:
        s[n - 1] = 0.0
    assert not torch.isnan(s).any()
    return s.contiguous()


def continuous_case(n, g):
    """the continuous input of the fuzz tests: no ties"""
    c = torch.rand(n, generator=g) * (20 + 3 * n ** 0.5)
    ln = torch.rand(n, generator=g) * 30 + 0.1
    return torch.stack((c - ln / 2, c + ln / 2), -1).contiguous(), torch.rand(n, generator=g).contiguous()


def grid_logits(shape, g):
    return (torch.round((torch.randn(*shape, generator=g) * 2 - 2) * 16) / 16).clamp_(-8, 4)


def grid_offsets(shape, g):
    return torch.randint(0, 41, (*shape, 2), generator=g).float() / 8


# ------------------------------------------------------------------------------------------------ NMS expectations
def _live(row, count, n_max):
    return row[:max(min(int(count), int(n_max)), 0)]


def expect_nms(segs, scores, counts, n_max, thr):
    """hard NMS of every query on its live part row[:min(count, n_max)] (counts None: n_max rows): [int64 index tensor per query]"""
    nq = segs.shape[0]
    out = []
    for q in range(nq):
        c = n_max if counts is None else counts[q]
        out.append(nms_oracle.nms(_live(segs[q], c, n_max).contiguous(), _live(scores[q], c, n_max).contiguous(), thr))
    return out


def expect_softnms(segs, scores, counts, n_max, thr, sigma, min_score, method, max_iters=0):
    """soft NMS of every query on its live part: [(dets (k, 3), inds (k,)) per query].

    max_iters = m > 0 stops after m picks.  The expectation is then the first min(m, k_full) rows of the FULL run's dets and inds
    (k_full: the full run's count).  Why a prefix: the reference's loop (nms_cpu.cpp:115-165) is sequential in the picks.  Pick i
    writes dets[i] and swaps the picked segment into position i; the decay and the swap-with-last pruning behind it only touch
    positions > i.  So rows 0 .. i of dets and inds are final once pick i is made, a run stopped after m picks has made exactly the
    first m picks of the full run, and if the candidates run out first (k_full < m) it IS the full run."""
    full = expect_softnms_full(segs, scores, counts, n_max, thr, sigma, min_score, method)
    return [softnms_prefix(d, i, max_iters) for d, i in full]


def expect_softnms_full(segs, scores, counts, n_max, thr, sigma, min_score, method):
    nq = segs.shape[0]
    out = []
    for q in range(nq):
        c = n_max if counts is None else counts[q]
        s, sc = _live(segs[q], c, n_max).contiguous(), _live(scores[q], c, n_max).contiguous()
        dets = torch.full((len(s), 3), float('nan'))
        inds = nms_oracle.softnms(s, sc, dets, thr, sigma, min_score, method)
        out.append((dets[:len(inds)].clone(), inds))
    return out


def softnms_prefix(dets, inds, max_iters):
    k = len(inds) if max_iters <= 0 else min(int(max_iters), len(inds))
    return dets[:k], inds[:k]


def softnms_early_stop(segs, scores, thr, sigma, min_score, method, max_iters):
    """a straight Python restatement of the reference's loop (nms_cpu.cpp:72-172) in fp32 with an early stop after max_iters picks;
    returns (dets, inds) of the picks made.  Slow: for the small inputs that pin the prefix rule of `expect_softnms`."""
    import numpy as np
    f = np.float32
    n = len(segs)
    x1 = segs[:, 0].numpy().astype(f).copy()
    x2 = segs[:, 1].numpy().astype(f).copy()
    sc = scores.numpy().astype(f).copy()
    ar = ((x2 - x1) + f(1e-6)).astype(f)
    ind = np.arange(n)
    dets = []
    nsegs, i = n, 0
    thr, sigma, min_score = f(thr), f(sigma), f(min_score)
    with np.errstate(all='ignore'):
        while i < nsegs and (max_iters <= 0 or i < max_iters):
            mp = i
            for pos in range(i + 1, nsegs):
                if sc[mp] < sc[pos]:
                    mp = pos
            for a in (x1, x2, sc, ar, ind):
                a[i], a[mp] = a[mp], a[i]
            dets.append((x1[i], x2[i], sc[i]))
            pos = i + 1
            while pos < nsegs:
                inter = max(f(0), f(min(x2[i], x2[pos]) - max(x1[i], x1[pos])))
                ovr = f(inter / f(f(ar[i] + ar[pos]) - inter))
                w = f(1)
                if method == 0:
                    w = f(0) if ovr >= thr else w
                elif method == 1:
                    w = f(f(1) - ovr) if ovr >= thr else w
                else:
                    w = _expf(f(-f(ovr * ovr) / sigma))
                sc[pos] = f(sc[pos] * w)
                if sc[pos] < min_score:
                    for a in (x1, x2, sc, ar, ind):
                        a[pos] = a[nsegs - 1]
                    nsegs -= 1
                    pos -= 1
                pos += 1
            i += 1
    k = min(i, nsegs)
    d = torch.tensor([[float(v) for v in row] for row in dets[:k]], dtype=torch.float32).reshape(-1, 3)
    return d, torch.from_numpy(ind[:k].copy())


def _expf(x):
    """the host C library's expf, the function the C oracle calls"""
    import ctypes
    import ctypes.util
    import numpy as np
    global _LIBM
    if _LIBM is None:
        _LIBM = ctypes.CDLL(ctypes.util.find_library('m') or 'libm.so.6')
        _LIBM.expf.restype = ctypes.c_float
        _LIBM.expf.argtypes = [ctypes.c_float]
    return np.float32(_LIBM.expf(float(x)))


_LIBM = None


# ------------------------------------------------------------------------------------------------ voting
def vote32(nms_segs, all_segs, all_scores, thr):
    """the fp32 oracle itself"""
    return R.segment_voting(nms_segs.float(), all_segs.float(), all_scores.float(), thr)


def vote64(nms_segs, all_segs, all_scores, thr):
    """the oracle's segment_voting on fp64 casts of the same fp32 inputs"""
    out = R.segment_voting(nms_segs.double(), all_segs.double(), all_scores.double(), thr)
    assert out.dtype == torch.float64, out.dtype      # a silent downcast inside the oracle would make the gate fp32 against fp32
    return out


def voting_margin(nms_segs, all_segs, thr):
    """the smallest NON-ZERO |iou64 - thr| over all survivor / candidate pairs (inf if there is none).  A voting input is fit for a
    parity test when this is >= MARGIN: then no fp32 rounding of a quotient can move a candidate across the threshold.  |iou - thr| == 0
    is harmless on the grids of this module: overlap and union are exact in fp32 and in fp64, and the one division rounds the same
    rational to the nearest fp32 / fp64 as the literal `thr` is rounded."""
    a, b = nms_segs.double()[:, None, :2], all_segs.double()[None]
    ov = (torch.minimum(a[..., 1], b[..., 1]) - torch.maximum(a[..., 0], b[..., 0])).clamp(min=0)
    uni = (a[..., 1] - a[..., 0]) + (b[..., 1] - b[..., 0]) - ov
    d = (ov / uni - thr).abs()
    assert not torch.isnan(d).any()
    d = d[d > 0]
    return float(d.min()) if d.numel() else float('inf')


VOTING_N2 = (1, 63, 64, 65, 777, 2000, 4099)
VOTING_LD = (2, 3)
VOTING_THR = (0.75, 0.95)
VOTING_NQ = 3
VOTING_N1 = 9


@functools.lru_cache(maxsize=None)
def voting_case(n2, ld, thr):
    """One launch of dcf_segment_voting: nq = 3, n1_max = 9 survivors per query in rows of n1_stride = 11, n2 candidates in rows of
    n2_stride = n2 + 3; per-query counts below the maxima for q > 0.  Survivors are candidates (moved by one grid step on odd rows, so
    that partial overlaps near the threshold occur); survivor 1 of every query lies far from every candidate: nothing votes for it.
    Dead rows and columns hold NaN segments and +inf scores.  Returns a dict of CPU tensors (to be left unchanged)."""
    g = gen(41, n2, ld, int(thr * 100))
    nq, n1, n1s, n2s = VOTING_NQ, VOTING_N1, VOTING_N1 + 2, n2 + 3
    c1 = torch.tensor([n1, 4, 0], dtype=torch.int32)
    c2 = torch.tensor([n2, max(n2 - 1, 1) if n2 < 70 else n2 - 67, n2], dtype=torch.int32)
    all_segs = torch.full((nq, n2s, 2), float('nan'))
    all_scores = torch.full((nq, n2s), float('inf'))
    nms = torch.full((nq, n1s, ld), float('nan'))
    for q in range(nq):
        m = int(c2[q])
        # a narrow span: many candidates vote for one survivor (long fp32 sums)
        all_segs[q, :m] = grid_segments(m, g, span=6 + min(m, 2000) // 40)
        all_scores[q, :m] = torch.rand(m, generator=g) * 0.98 + 0.01
        k = int(c1[q])
        pick = torch.randint(0, m, (k,), generator=g)
        s = all_segs[q, pick].clone()
        s[1::2, 1] += 0.25
        if k > 1:
            s[1] = torch.tensor([1000.0, 1003.5])
        nms[q, :k, :2] = s
        if ld == 3:
            nms[q, :k, 2] = all_scores[q, pick]
    return dict(nq=nq, n1=n1, n1_stride=n1s, ld=ld, n2=n2, n2_stride=n2s, thr=thr, c1=c1, c2=c2, nms=nms, all_segs=all_segs, all_scores=all_scores)


def voting_cases():
    return [(n2, ld, thr) for n2 in VOTING_N2 for ld in VOTING_LD for thr in VOTING_THR]


def voting_expect(case):
    """per query: (y64, y32) of the live survivors against the live candidates"""
    out = []
    for q in range(case['nq']):
        k, m = int(case['c1'][q]), int(case['c2'][q])
        a, b, s = case['nms'][q, :k, :2], case['all_segs'][q, :m], case['all_scores'][q, :m]
        out.append((vote64(a, b, s, case['thr']), vote32(a, b, s, case['thr'])))
    return out


# ------------------------------------------------------------------------------------------------ collect
# name: (T0, levels, nq, topk, seg_len_thresh, pre_nms_thresh, seed)
COLLECT = {
    'reread-q2-bitonic': (32768, 2, 2, 4000, 3.0, 0.001, 0),     # S = 49152: keys re-read from global memory with q > 0; bitonic sort, ties at the cut
    'cached-32768': (32768, 1, 2, 2000, 3.0, 0.001, 0),          # S = 32768: the last register-cached size
    'reread-32769': (32769, 1, 1, 2048, 0.1, 0.001, 0),          # the first re-read size, K = RS_MAX (radix sort's capacity)
    'masked-query': (64, 1, 3, 50, 0.1, 0.001, 3),               # the last query fully masked next to live ones
    'thresh-0.3': (32768, 1, 2, 2000, 3.0, 0.3, 1),              # pre_nms_thresh = 0.3
}


@functools.lru_cache(maxsize=None)
def collect_case(name):
    T0, Lv, nq, topk, slt, pthr, seed = COLLECT[name]
    g = gen(42, T0, Lv, nq, topk, seed)
    sizes = [T0 >> l for l in range(Lv)]
    S = sum(sizes)
    logits, offsets = grid_logits((nq, S), g), grid_offsets((nq, S), g)
    masks = torch.ones(nq, S, dtype=torch.bool)
    if name == 'masked-query':
        masks[-1] = False
    else:
        masks[0, int(S * 0.97):] = False
    return dict(name=name, T0=T0, Lv=Lv, nq=nq, topk=topk, seg_len_thresh=slt, pre_nms_thresh=pthr, sizes=sizes, S=S, logits=logits,
                offsets=offsets, masks=masks)


@functools.lru_cache(maxsize=None)
def collect_expect(name):
    """[(segs, scores) per query] from the oracle's collect_segments"""
    c = collect_case(name)
    pts = R.generate_points(c['T0'], c['Lv'], 4, 0.5)
    out = []
    for q in range(c['nq']):
        out.append(R.collect_segments(pts, [x[None] for x in c['logits'][q].split(c['sizes'])], [x[None] for x in c['offsets'][q].split(c['sizes'])],
                                      [x[None] for x in c['masks'][q].split(c['sizes'])], pre_nms_thresh=c['pre_nms_thresh'],
                                      pre_nms_topk=c['topk'], seg_len_thresh=c['seg_len_thresh']))
    return out


def collect_figures(name):
    """per query: (candidates above pre_nms_thresh, cut = min(candidates, topk), size of the group of equal scores the cut falls into
    -- 0 if the cut takes every candidate --, candidates of that group left out by the cut, kept after the length filter)"""
    c = collect_case(name)
    figs = []
    for q, (ws, wc) in enumerate(collect_expect(name)):
        s = torch.sigmoid(c['logits'][q]) * c['masks'][q].float()
        s = s[s > c['pre_nms_thresh']].sort(descending=True)[0]
        n, cut = len(s), min(len(s), c['topk'])
        if cut == n or cut == 0:
            figs.append((n, cut, 0, 0, len(wc)))
            continue
        grp = int((s == s[cut - 1]).sum())
        left_out = int((s[cut:] == s[cut - 1]).sum())
        figs.append((n, cut, grp, left_out, len(wc)))
    return figs
