"""The selected-clip rules restated in torch (include/decafnet_hip_select.h), for tests/test_select_cpu.py and tests/test_gpu_select.py.

    needed[t] = vid_mask[t] and any_q gate[q, t] != 0
    clips     = the needed clips, ascending;  count = len(clips)
    pos[t]    = rank of t among the needed clips, -1 where t is not needed
    rows[i]   = X[:, clips[i]]

and the oracle's gates of an evaluation fixture (oracle/decafnet_ref.py: sidekick_scores, topk_block_gate), with the gap between the
k-th and the (k+1)-th pooled block score that decides how exact a comparison of gates can be."""
import sys

import torch
import torch.nn.functional as F

from conftest import ROOT

if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import decafnet_ref as R  # noqa: E402

# the fixtures of the exact-gate list: the default class with the expert half in use, vid_net.stride = 1, no scat
FIXTURES = ['c1', 'pe', 'nomsf', 'affine']
GAP_MIN = 1e-4                  # far above the 2e-6 the scoring kernels are known to differ by (tests/test_gpu_e2e.py)


def select_clips(gate, vid_mask):
    """gate (nq, T) float, vid_mask (T) bool / bytes -> (clips int32 (count), pos int32 (T), count)"""
    needed = vid_mask.reshape(-1).bool() & (gate != 0).any(0)
    clips = needed.nonzero().reshape(-1).to(torch.int32)
    pos = torch.full((needed.numel(),), -1, dtype=torch.int32)
    pos[clips.long()] = torch.arange(clips.numel(), dtype=torch.int32)
    return clips, pos, int(clips.numel())


def gather_clip_rows(x_cm, clips):
    """x_cm (D, T) -> (n, D): row i = column clips[i]"""
    return x_cm[:, clips.long()].t().contiguous()


def oracle_gates(cfg, shallow_vid, vid_masks, text_cls):
    """the oracle's (nq, T) 0 / 1 gates of one video: model.py:527-541 per query, zero on the padded clips"""
    correl = R.sidekick_scores(shallow_vid, text_cls, cfg['norm'])
    vid_len = int(vid_masks.sum())
    gate = torch.zeros(correl.shape[0], vid_masks.shape[-1])
    for b in range(correl.shape[0]):
        gate[b, :vid_len] = R.topk_block_gate(correl[b], vid_len, cfg['sn'], cfg['sratio'])
    return gate


def gate_gaps(cfg, shallow_vid, vid_masks, text_cls):
    """per query, the distance between the k-th largest and the (k+1)-th largest pooled block score, k = int(sratio n): the margin by
    which the top-k choice is decided (inf where k == 0 or k == n: every block is kept whatever the scores are)"""
    correl = R.sidekick_scores(shallow_vid, text_cls, cfg['norm'])
    vid_len = int(vid_masks.sum())
    gaps = []
    for b in range(correl.shape[0]):
        pooled = F.avg_pool1d(correl[b][None, None, :vid_len], kernel_size=cfg['sn'], stride=cfg['sn'], ceil_mode=True)[0, 0]
        n = pooled.numel()
        k = int(cfg['sratio'] * n)
        if k == 0 or k == n:
            gaps.append(float('inf'))
            continue
        s = pooled.sort(descending=True).values
        gaps.append(float(s[k - 1] - s[k]))
    return gaps
