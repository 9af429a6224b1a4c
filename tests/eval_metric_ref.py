"""dcf_op_recall_update (include/decafnet_hip_eval.h) restated in torch on the CPU, one fp32 operation per line: what the operator is
compared with on the GPU (tests/test_gpu_eval_metric.py), and what tests/test_eval_metric_cpu.py compares with the package's own host
arithmetic (``GroundingEvaluator.finish_proposals``, ``evaluator.iou``, ``RecallCounter``).  The random case generator of both lives
here too.

A NaN ``best`` is written as the quiet NaN 0x7fc00000, as the header says, so that ``best`` compares as bits."""
import numpy as np
import torch

QNAN = torch.tensor([0x7fc00000], dtype=torch.int32).view(torch.float32)[0]


def to_seconds(segs, meta):
    """step 1: (nq, M, 2) grid units -> seconds where meta[:, 7] != 0; rows beyond the counts are converted too and mean nothing"""
    m = meta[:, None, :]
    x = segs * m[..., 2:3]
    x = x * m[..., 3:4]
    x = x + m[..., 4:5]
    x = x / m[..., 5:6]
    x = torch.minimum(torch.maximum(x, torch.zeros(())), m[..., 6:7])         # NaN-propagating, like torch.clamp
    return torch.where(m[..., 7:8] != 0, x, segs)


def overlaps(secs, meta):
    """step 2: IoU of every row with its query's ground truth, (nq, M)"""
    p0, p1, g0, g1 = secs[..., 0], secs[..., 1], meta[:, None, 0], meta[:, None, 1]
    lo = torch.maximum(p0, g0)
    hi = torch.minimum(p1, g1)
    d = hi - lo
    inter = torch.maximum(d, torch.zeros(()))
    total = (p1 - p0) + (g1 - g0)
    return inter / (total - inter)


def recall_update(segs, counts, meta, ranks, threshs, hits, n_queries):
    """steps 3 and 4 -> best (nq, n_ranks) fp32; ``hits`` (n_ranks, n_threshs) int64 and ``n_queries`` (1) int64 are added to in place"""
    nq, M = segs.shape[:2]
    v = overlaps(to_seconds(segs, meta), meta)
    best = torch.zeros(nq, len(ranks), dtype=torch.float32)
    for q in range(nq):
        c = min(max(int(counts[q]), 0), M)
        for i, k in enumerate(ranks):
            n = min(max(int(k), 0), c)
            if n:
                row = v[q, :n]
                best[q, i] = QNAN if bool(torch.isnan(row).any()) else row.max()
    hit = best.double()[:, :, None] >= torch.as_tensor(np.asarray(threshs, dtype=np.float64))[None, None]
    hits += hit.sum(0)
    n_queries += nq
    return best


def bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------- cases
def meta_rows(gt, vid_stride, clip_stride, clip_size, fps, duration, convert=True):
    """the operator's record per query from the quantities of a video, each rounded to fp32 once (what evaluator.query_meta returns)"""
    gt = np.asarray(gt, dtype=np.float64).reshape(-1, 2)
    meta = np.empty((len(gt), 8), dtype=np.float32)
    meta[:, :2] = gt
    meta[:, 2:] = np.array([vid_stride, clip_stride, 0.5 * clip_size, fps, duration, 1.0 if convert else 0.0])
    return torch.from_numpy(meta)


def random_video(g, nq, M, vid_stride=1, clip_stride=16, clip_size=16, fps=30.0, n_clips=120, convert=True, sentinels=True):
    """one video's worth of operands: segs (nq, M, 2) in grid units (seconds if not ``convert``) with some rows reaching before 0 and
    past the duration, counts (nq) drawn from [0, M], the ground truth inside the video, and NaN / inf beyond the counts"""
    duration = ((n_clips - 1) * clip_stride + clip_size) / fps
    unit = clip_stride * vid_stride / fps if convert else 1.0
    span = duration / unit if convert else duration
    a = torch.rand(nq, M, generator=g) * span * 1.2 - 0.15 * span
    b = a + torch.rand(nq, M, generator=g) * span * 0.4
    segs = torch.stack((a, b), -1).float()
    counts = torch.randint(0, M + 1, (nq,), generator=g, dtype=torch.int32)
    g0 = torch.rand(nq, generator=g).double() * duration * 0.6
    g1 = g0 + (0.05 + torch.rand(nq, generator=g).double() * 0.35) * duration
    gt = torch.stack((g0, g1.clamp(max=duration)), -1).numpy()
    if sentinels:
        for q in range(nq):
            c = int(counts[q])
            segs[q, c:] = torch.tensor([float('nan'), float('inf')])[(torch.arange(M - c) + q) % 2][:, None]
    return dict(segs=segs, counts=counts, gt=gt, meta=meta_rows(gt, vid_stride, clip_stride, clip_size, fps, duration, convert),
                vid_stride=vid_stride, clip_stride=clip_stride, clip_size=clip_size, fps=fps, duration=duration, convert=convert)
