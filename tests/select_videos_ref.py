"""Selected-clip inference on several videos restated in torch (include/decafnet_hip_select_videos.h), for
tests/test_select_videos_cpu.py and tests/test_gpu_select_videos.py: per video the rules of tests/select_ref.py, then the packing.

    queries of video v     = rows q_first[v] .. q_first[v + 1] - 1 of the flat gate (NQ, T)
    clips[v, :counts[v]]   = select_ref.select_clips(gate of v's queries, vid_masks[v]);  the rest keeps ``fill``
    pos[v]                 = its inverse, video-local
    row_first              = the running sum of counts, from 0
    rows[row_first[v] + i] = X[v][:, clips[v, i]]
"""
import torch

import select_ref as S


def select_clips_videos(gate, vid_masks, nqs, fill=-7):
    """gate (NQ, T) float, vid_masks (nvid, T) bool / bytes, nqs: the videos' query counts
    -> (clips int32 (nvid, T) with ``fill`` beyond each count, pos int32 (nvid, T), counts: list of int, row_first: list of int)"""
    nvid, T = vid_masks.shape
    assert len(nqs) == nvid and sum(nqs) == gate.shape[0] and gate.shape[1] == T
    clips = torch.full((nvid, T), fill, dtype=torch.int32)
    pos = torch.empty(nvid, T, dtype=torch.int32)
    counts, row_first, q = [], [0], 0
    for v in range(nvid):
        c, p, n = S.select_clips(gate[q:q + nqs[v]], vid_masks[v])
        clips[v, :n], pos[v] = c, p
        counts.append(n)
        row_first.append(row_first[-1] + n)
        q += nqs[v]
    return clips, pos, counts, row_first


def gather_clip_rows_videos(xs, clips, counts):
    """xs: the videos' (D, T) matrices -> (sum of counts, D): video after video, row i of video v = column clips[v, i]"""
    return torch.cat([S.gather_clip_rows(x, clips[v, :counts[v]]) for v, x in enumerate(xs)])


def video_gaps(cfg, videos):
    """S.gate_gaps of every video of ``videos`` ((vid, shallow_vid (1, D, T), vid_masks (1, T), text, text_cls, text_masks) on the
    host) as one flat list, video after video"""
    return [gap for a in videos for gap in S.gate_gaps(cfg, a[1], a[2], a[4])]


# ---------------------------------------------------------------------------------------------- the seeded inputs of the GPU tests
# the model and the three videos of test_forward_videos_equals_single_video_forwards (tests/test_gpu_e2e.py): one padded length,
# valid lengths 256 / 200 / 77, 2 / 1 / 3 queries
KW3 = dict(D=64, E=64, TE=32, text_in=32, n_levels=4, win=5, n_heads=4, sn=8, sratio=0.3, msf=True, norm=True, max_seq_len=128,
           text_layers=1, text_max_len=24)
T3, LENS3, WSEED3 = 256, [(256, 2), (200, 1), (77, 3)], 33
SECOND_SEED = 953               # the synthetic video a fixture is paired with: its own T, nine padded clips, two queries


def three_inputs(pkg):
    """synth.make_inputs of the three videos (host tensors)"""
    return [pkg.synth.make_inputs(64, T3, vid_len, nq, 32, 5 + v, 900 + v) for v, (vid_len, nq) in enumerate(LENS3)]


def second_input(pkg, c):
    """the second video beside the fixture case ``c`` (forward_parity.e2e_case)"""
    return pkg.synth.make_inputs(c.kw['D'], c.meta['T'], c.meta['T'] - 9, 2, c.kw['text_in'], 6, SECOND_SEED)


TINY = dict(D=64, E=64, TE=32, text_in=32, n_levels=4, win=5, n_heads=4, sn=8, sratio=0.3, msf=True, norm=True, max_seq_len=128,
            text_layers=1, text_max_len=24, max_vid_len=128)
EVAL_LENS, EVAL_SEED = (100, 128, 90, 300), 16   # padded lengths 128, 128, 128, 320: a group of three and a group of one


def evaluator_samples():
    """the per-video dicts GroundingEvaluator.run takes, on the host"""
    g = torch.Generator().manual_seed(EVAL_SEED)
    samples = []
    for vid_len in EVAL_LENS:
        nq = 1 + vid_len % 3
        samples.append(dict(vid=torch.randn(64, vid_len, generator=g), shallow_vid=torch.randn(64, vid_len, generator=g),
                            text=tuple(torch.randn(32, 6, generator=g) for _ in range(nq)), text_cls=torch.randn(nq, 64, generator=g),
                            segment=torch.rand(nq, 2, generator=g).sort(1).values * vid_len * 16 / 30.0,
                            fps=30.0, clip_stride=16, clip_size=32, duration=vid_len * 16 / 30.0 + 2, clip_id=f'v{vid_len}'))
    return samples


def sample_gaps(cfg, sample):
    """S.gate_gaps of an evaluator sample (the padding does not enter: the gate pools the valid clips only)"""
    n = sample['shallow_vid'].size(-1)
    return S.gate_gaps(cfg, sample['shallow_vid'][None], torch.ones(1, n, dtype=torch.bool), sample['text_cls'])
