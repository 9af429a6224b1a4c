"""Hot-path harness: the parts of the reference ``Evaluator`` that sit on the grounding path
(libs/worker_v2.py:726-1187), on device tensors, for all queries of a video at once.

    padded_length      worker_v2.py:769-781, 969-976
    GroundingEvaluator.predict   _forward (930-1026) + _generate_proposals (1063-1129):
        pad -> encode_text -> model(..., eval=True) -> collect_segments -> batched NMS -> seconds

    iou, RecallCounter  libs/train_utils.py:81-96 and the metric loop of Evaluator.run, worker_v2.py:857-878, 890-901
    load_features       feature-file formats of libs/data/dataset.py:128-135, 398-399 ((T, C) on disk -> (C, T))

    query_meta, DeviceRecallCounter   the same metric accumulated in device memory by dcf_op_recall_update
        (include/decafnet_hip_eval.h): ``run(dataset, counter=DeviceRecallCounter(...))`` enqueues forward, collect_segments,
        batched NMS and the metric per video and reads nothing back before ``metrics()``
"""
from __future__ import annotations

import os
import time
from collections import defaultdict

import numpy as np
import torch
import torch.nn.functional as F

from . import loss as _loss
from . import nms as _nms


def iou(pred_segs, gt_segs):
    """Temporal IoU of (..., 2) [start, end] segments, broadcast over the leading dimensions.  Same value as the reference's
    ``iou`` (libs/train_utils.py:81-96): intersection clamped at 0 over (sum of lengths - intersection), no epsilon, so two
    empty segments give nan there as here."""
    lo = torch.maximum(pred_segs[..., 0], gt_segs[..., 0])
    hi = torch.minimum(pred_segs[..., 1], gt_segs[..., 1])
    inter = (hi - lo).clamp(min=0)
    total = (pred_segs[..., 1] - pred_segs[..., 0]) + (gt_segs[..., 1] - gt_segs[..., 0])
    return inter / (total - inter)


class RecallCounter:
    """Recall@k at temporal-IoU thresholds, the metric ``Evaluator.run`` accumulates (libs/worker_v2.py:857-878) and prints
    (:890-901).  A query is a hit at (k, t) when any of its k best-scored proposals overlaps the ground truth by IoU >= t;
    a query without proposals is a miss everywhere."""

    def __init__(self, ranks=(1, 5), iou_threshs=(0.3, 0.5)):
        self.ranks = tuple(int(k) for k in ranks)
        self.iou_threshs = np.asarray(iou_threshs, dtype=np.float64)
        self.hits = np.zeros((len(self.ranks), len(self.iou_threshs)))
        self.n_queries = 0

    # the reference's attribute names, for code that reads them
    @property
    def counts(self):
        return self.hits

    @property
    def text_cnt(self):
        return self.n_queries

    def update(self, results, targets):
        if len(results) != len(targets):
            raise ValueError(f'{len(results)} results for {len(targets)} ground-truth segments')
        for res, gt in zip(results, targets):
            segs, scores = res['segments'].cpu(), res['scores'].cpu()
            best_first = segs[torch.argsort(scores, descending=True)[:max(self.ranks)]]
            overlaps = iou(best_first, torch.as_tensor(gt, dtype=torch.float32)[None])
            for i, k in enumerate(self.ranks):
                best = float(overlaps[:k].max()) if len(overlaps[:k]) else 0.0
                self.hits[i] += best >= self.iou_threshs
        self.n_queries += len(targets)

    def metrics(self):
        return self.hits / max(self.n_queries, 1)

    def report(self):
        """the reference's table layout (worker_v2.py:890-901)"""
        m = self.metrics() * 100
        lines = ['', 'Final:']
        for i, k in enumerate(self.ranks):
            lines.append('-----')
            lines += [f'Rank@{k}, IoU@{t:.1f}: {m[i, j]:.2f}' for j, t in enumerate(self.iou_threshs)]
        return '\n'.join(lines + ['-----', ''])


META_FIELDS = ('gt_start', 'gt_end', 'vid_stride', 'clip_stride', 'half_clip', 'fps', 'duration', 'convert')


def query_meta(segment, vid_stride, clip_stride, clip_size, fps, duration, convert=True):
    """The per-query record of dcf_op_recall_update, (n, 8) float32 in the order of ``META_FIELDS``: the ground truth rounded to
    fp32 as ``RecallCounter.update`` rounds it, and the scalars of ``finish_proposals`` each rounded to fp32 as torch rounds a
    Python scalar that meets an fp32 tensor (0.5 * clip_size is formed in double first, as there)."""
    seg = np.asarray(segment, dtype=np.float64).reshape(-1, 2)
    meta = np.empty((len(seg), 8), dtype=np.float32)
    meta[:, :2] = seg
    meta[:, 2:] = np.array([vid_stride, clip_stride, 0.5 * clip_size, fps, duration, 1.0 if convert else 0.0], dtype=np.float64)
    return meta


class DeviceRecallCounter:
    """``RecallCounter`` with its table in device memory: ``update_device`` launches dcf_op_recall_update (include/decafnet_hip_eval.h)
    on the current stream for the rows ``nms.batched_nms_queries`` left on the GPU, and nothing is read back until ``hits`` /
    ``n_queries`` / ``metrics()`` / ``report()`` are asked for -- each of those is one 8 * (cells + 1)-byte copy that waits for the
    current stream.  The adds are integer atomics, so lanes on several streams may share one counter; the reader's stream has to be
    behind them (``GroundingEvaluator.run`` sees to it).  ``reset()`` zeroes the table on the stream."""

    MAX = 8                                        # ranks and thresholds of one dcf_op_recall_update call

    def __init__(self, ranks=(1, 5), iou_threshs=(0.3, 0.5), device='cuda'):
        self.ranks = tuple(int(k) for k in ranks)
        self.iou_threshs = np.asarray(iou_threshs, dtype=np.float64)
        if not 1 <= len(self.ranks) <= self.MAX or not 1 <= len(self.iou_threshs) <= self.MAX or min(self.ranks) < 1:
            raise ValueError(f'DeviceRecallCounter: ranks {self.ranks}, iou_threshs {tuple(self.iou_threshs)}: 1 to {self.MAX} of each, ranks >= 1')
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('DeviceRecallCounter counts on the MI355X only: RecallCounter is the host route')
        self._ranks = torch.tensor(self.ranks, dtype=torch.int32, device=self.device)
        self._threshs = torch.from_numpy(self.iou_threshs.copy()).to(self.device)
        self._cells = len(self.ranks) * len(self.iou_threshs)
        self._table = torch.zeros(self._cells + 1, dtype=torch.int64, device=self.device)      # hits, then n_queries

    def reset(self):
        self._table.zero_()
        return self

    def update_device(self, segs, counts, meta, best=None):
        """segs (nq, M, 2) fp32 and counts (nq) int32 as ``batched_nms_queries`` returns them, meta (nq, 8) fp32 (``query_meta``), all on
        the GPU; ``best``: an (nq, n_ranks) fp32 tensor to receive the best IoU per rank, or None.  No host wait."""
        from . import _lib
        nq, M = segs.shape[0], segs.shape[1]
        if segs.dim() != 3 or segs.shape[2] != 2 or counts.shape != (nq,) or meta.shape != (nq, 8):
            raise ValueError(f'update_device: segs {tuple(segs.shape)}, counts {tuple(counts.shape)}, meta {tuple(meta.shape)}')
        if segs.dtype != torch.float32 or meta.dtype != torch.float32 or not (segs.is_cuda and counts.is_cuda and meta.is_cuda):
            raise ValueError('update_device: segs and meta are fp32 tensors on the GPU')
        if best is not None and (best.shape != (nq, len(self.ranks)) or best.dtype != torch.float32 or not best.is_contiguous()):
            raise ValueError(f'update_device: best is a contiguous fp32 tensor of shape ({nq}, {len(self.ranks)})')
        if nq == 0:
            return
        segs, counts, meta = segs.contiguous(), counts.to(torch.int32).contiguous(), meta.contiguous()
        _lib.check(_lib.lib().dcf_op_recall_update(_lib.ptr(segs), _lib.ptr(counts), _lib.ptr(meta), nq, M, _lib.ptr(self._ranks),
                                                   len(self.ranks), _lib.ptr(self._threshs), len(self.iou_threshs), _lib.ptr(self._table),
                                                   _lib.ptr(self._table[self._cells:]), _lib.ptr(best), _lib.current_stream()),
                   'dcf_op_recall_update')

    def add_misses(self, n):
        """n queries without a proposal: misses at every cell (on the stream)"""
        self._table[self._cells:] += int(n)

    def _read(self):
        t = self._table.cpu()                      # the one host read
        return t[:self._cells].numpy().reshape(len(self.ranks), len(self.iou_threshs)).astype(np.float64), int(t[self._cells])

    @property
    def hits(self):
        return self._read()[0]

    @property
    def n_queries(self):
        return self._read()[1]

    counts = hits                                  # the reference's attribute names, as on RecallCounter
    text_cnt = n_queries

    def metrics(self):
        hits, n = self._read()
        return hits / max(n, 1)

    report = RecallCounter.report


LOSS_KEYS = ('cls_loss', 'reg_loss')


class DeviceLossMeter:
    """The validation loss ``Evaluator.run`` logs (worker_v2.py:856, 903-906: ``_calc_loss`` per video, then the mean over the videos)
    without a host read per video.  Holds, on the bank's device, ``rows`` (N_queries, 4) fp32, zeroed -- one row (focal1, focal2, iou,
    n_pos) per query, in the bank's query order --, ``offsets`` (V + 1) int64 from ``bank.queries`` and ``bank.targets``.

    ``update_device(flat, T, data)`` is ONE dcf_point_objective call on what the evaluation forward left on the device, with the
    parameters of ``calc_loss`` (one classification head, alpha 0.5, smoothing 0.2, GIoU, centre sampling from ``opt.train``), whose
    ``rows_out`` is the video's slice of the table.  Videos own disjoint slices: lanes on several streams and several ranks fill one
    table without atomics, and a sum of the ranks' tables adds zeros, which is exact.  ``losses()`` is one launch of
    dcf_op_loss_table_mean (include/decafnet_hip_fit.h) and one 16-byte read.

    ``opt``: the ``config.make_opt`` tree; None: ``GroundingEvaluator.run`` hands over its own at the first pass."""

    def __init__(self, bank, opt=None):
        if bank.device.type != 'cuda':
            raise RuntimeError('DeviceLossMeter computes on the MI355X only: calc_loss per video is the host route')
        self.bank, self.device, self.opt = bank, bank.device, opt
        ends = np.cumsum([0] + [nq for _, nq in (bank.queries[k] for k in bank.index)])
        if [q0 for q0, _ in (bank.queries[k] for k in bank.index)] != ends[:-1].tolist():
            raise ValueError('DeviceLossMeter: bank.queries is not the bank\'s videos back to back')
        self.offsets = torch.from_numpy(ends.astype(np.int64)).to(self.device)
        self.targets = bank.targets
        self.rows = torch.zeros(int(ends[-1]), 4, dtype=torch.float32, device=self.device)
        self._out = torch.empty(2, dtype=torch.float64, device=self.device)

    def use(self, opt):
        """take ``opt`` where the meter was made without one"""
        if self.opt is None:
            self.opt = opt
        return self

    def reset(self):
        self.rows.zero_()
        return self

    def update_device(self, flat, T, data):
        """``flat``: (logits (nq, S), offsets (nq, S, 2), masks (nq, S)) of the video's queries as the evaluation forward leaves them,
        ``T`` the padded input length, ``data`` the video's item of the bank.  No host wait.  Refused before the launch, with the
        video's name: what dcf_point_objective would refuse (``T // vid_stride`` beyond pt_gen's max_seq_len or no pyramid)."""
        from . import _lib
        if self.opt is None:
            raise ValueError('DeviceLossMeter: no opt (DeviceLossMeter(bank, opt), or hand the meter to GroundingEvaluator.run)')
        logits, offsets, masks = flat
        name = data['clip_id']
        q0, nq = self.bank.queries[name]
        mo, tr = self.opt['model'], self.opt['train']
        (rr, sigma, msl), use_offset = _loss.pt_gen_params(self.opt)
        Tp, L = T // int(mo.get('vid_stride', 1)), int(mo['num_fpn_levels'])
        S = sum(Tp >> l for l in range(L))
        if Tp > msl:
            raise ValueError(f'video {name}: T // vid_stride = {Tp} points at level 0, pt_gen.max_seq_len is {msl}: dcf_point_objective '
                             f'refuses the layout')
        if not 1 <= L <= 16 or Tp < 1 or Tp >= 1 << 23 or Tp % (1 << (L - 1)):
            raise ValueError(f'video {name}: T // vid_stride = {Tp} with {L} levels is not a PtGenerator layout')
        if logits.shape != (nq, S) or offsets.shape != (nq, S, 2) or masks.shape != (nq, S):
            raise ValueError(f'video {name}: logits {tuple(logits.shape)}, offsets {tuple(offsets.shape)}, masks {tuple(masks.shape)} for '
                             f'{nq} queries of {S} points')
        if logits.dtype != torch.float32 or offsets.dtype != torch.float32 or masks.dtype != torch.bool or \
                not (logits.is_contiguous() and offsets.is_contiguous() and masks.is_contiguous()) or logits.device != self.rows.device:
            raise ValueError(f'video {name}: the forward\'s outputs are contiguous fp32 / bool tensors on {self.device}')
        if nq == 0:
            return
        _lib.check(_lib.lib().dcf_point_objective(
            None, _lib.ptr(logits), _lib.ptr(offsets), _lib.ptr(masks), _lib.ptr(self.targets[q0:q0 + nq]), nq, Tp, L, rr, sigma,
            int(use_offset), msl, int(tr.get('center_sampling', 'radius') == 'radius'), float(tr['center_sampling_radius']), 0.5, 0.2, 0, 1e-8,
            None, 1.0, 1.0, _lib.ptr(self.rows[q0:q0 + nq]), None, _lib.current_stream()), 'dcf_point_objective')

    def losses(self, per_video=False):
        """-> {'cls_loss', 'reg_loss'} as Python floats: one launch, one 16-byte read that waits for the current stream.
        ``per_video=True``: -> (that, the (V, 2) float64 array of the per-video means), a second read."""
        from . import _lib
        pv = torch.empty(len(self.offsets) - 1, 2, dtype=torch.float64, device=self.device) if per_video else None
        _lib.check(_lib.lib().dcf_op_loss_table_mean(_lib.ptr(self.rows), _lib.ptr(self.offsets), len(self.offsets) - 1, _lib.ptr(pv),
                                                     _lib.ptr(self._out), _lib.current_stream()), 'dcf_op_loss_table_mean')
        out = self._out.cpu()                          # the one host read
        stats = {k: float(out[i]) for i, k in enumerate(LOSS_KEYS)}
        return (stats, pv.cpu().numpy()) if per_video else stats

    @staticmethod
    def line(stats):
        """the loss line of the evaluation report (worker_v2.py:903-906)"""
        return ''.join(f'{k}: {v:.3f}; ' for k, v in stats.items())


def load_features(path_without_ext: str, fmt: str = 'npy', dtype=np.float32):
    """One feature file as the reference stores it ((T, C) on disk: npy / pt / pk0 / pk1 / pk_avg, libs/data/dataset.py:107-135)
    returned channel-major (C, T) like ``_load_vid_feats`` (:398-399).  Multi-source videos: ``data.load_video_features``.
    ``dtype``: np.float32 (default), 'stored' (a float16 file stays float16) or np.float16 (a cast), as in ``data.load_clip_features``."""
    from . import data as _data
    a = np.asarray(_data.load_clip_features(path_without_ext, fmt, dtype))
    if a.dtype != np.float16:
        a = np.asarray(a, dtype=np.float32)
    return torch.from_numpy(np.ascontiguousarray(a.transpose()))


def min_chunk_size(num_fpn_levels: int, mha_win_size: int) -> int:
    """worker_v2.py:769-781"""
    m = 1
    for l in range(num_fpn_levels):
        s = 2 ** l
        if mha_win_size > 0:
            s *= (mha_win_size // 2) * 2
        m = max(m, s)
    return m


def padded_length(vid_len: int, max_vid_len: int, num_fpn_levels: int, mha_win_size: int, vid_stride: int = 1) -> int:
    """worker_v2.py:969-976: short videos pad to max_vid_len, long ones to the next multiple of the chunk size."""
    input_len = max_vid_len * vid_stride
    if vid_len > input_len:
        stride = min_chunk_size(num_fpn_levels, mha_win_size) * vid_stride
        input_len = (vid_len + (stride - 1)) // stride * stride
    return input_len


def calc_loss(outputs, targets, opt, pt_gen=None):
    """Evaluator._calc_loss (worker_v2.py:1029-1061), the validation-time loss: per (video, query) row norm = max(n_pos, 1),
    cls_loss = calc_focal_loss(logits[masks], labels[masks]) / norm with that function's defaults (smoothing 0.2, alpha 0.5),
    reg_loss = calc_iou_loss(..., reg_loss='iou') / norm, which selects the GIoU loss; then the mean over the rows, NaN skipped.
    ``outputs``: (logits, offsets, masks) as per-level tuples of (B', T_l) tensors (what a forward of the single-head form
    returns; of a two-head training forward pass parts 1 - 3), or the reference's (logits_list, offsets_list, points,
    masks_list) with one level tuple of (1, T_l) tensors per query.  ``targets`` (B', 2), already divided by vid_stride.
    One fused pass on the device (loss.PointObjective's kernel, per-row results) and one host read at the end.
    Returns ({'cls_loss', 'reg_loss'}, per-row (B', 2) array)."""
    if len(outputs) == 4:                                                   # the reference's tuple: per query, then per level
        lg, of, _, mk = outputs
        outputs = tuple(tuple(torch.cat([q[l] for q in part], 0) for l in range(len(part[0]))) for part in (lg, of, mk))
    tr = opt['train']
    params, use_offset = _loss.pt_gen_params(opt, pt_gen)
    rows, _ = _loss._objective(outputs, targets, params, use_offset, tr.get('center_sampling', 'radius'), tr['center_sampling_radius'],
                               0.5, 0.2, 'iou', None, 1, 1.0)
    norm = rows[:, 3].clamp(min=1)
    per_row = torch.stack((rows[:, 1] / norm, rows[:, 2] / norm), 1).cpu().numpy()      # the one host read
    stats = {}
    for k, name in enumerate(('cls_loss', 'reg_loss')):
        v = [float(x) for x in per_row[:, k] if not np.isnan(x)]
        stats[name] = float(np.mean(v)) if v else float('nan')
    return stats, per_row


class GroundingEvaluator:
    """``opt`` needs ``opt.model.{max_vid_len, num_fpn_levels, mha_win_size, vid_stride}``, ``opt.eval.{pre_nms_topk,
    pre_nms_thresh, seg_len_thresh}`` and ``opt.nms`` (libs/core/opt.py:174-194)."""

    def __init__(self, opt, model, feature_dtype=None, expert='dense', expert_fn=None, select_videos=False):
        """``expert``: 'dense' (the default: the reference's interface, ``vid`` holds the expert features of every clip) or 'selected':
        per forward window ``model.select_clips`` says which clips the gates need, the expert features of those clips alone are
        obtained -- from ``expert_fn(sample, clips_host)`` -> (count, D) fp32 or float16 rows, clips_host the ascending int64 clip
        indices (all below the video's length), or, with ``expert_fn=None``, by ``model.gather_clip_rows`` from the sample's dense
        ``vid`` -- and ``model.forward_selected`` runs on them (include/decafnet_hip_select.h).  The proposal stage is the same.
        ``select_videos`` (with expert='selected'; default False): ``run(batch_videos=N)`` groups videos of one padded length as the
        dense route does, on the host route and on the device route; per group ``model.select_clips_videos`` (one host read for all
        videos), ``expert_fn`` once per video -- its rows are packed video after video -- or ``model.gather_clip_rows_videos``, and
        ONE ``model.forward_videos_selected`` (include/decafnet_hip_select_videos.h).  A ``scat`` model is accepted with it.  Without
        it ``run(batch_videos > 1)`` is refused.  Not here in either form: the items of a ``data.EvalBank``.
        ``feature_dtype``: None -- ``vid`` / ``shallow_vid`` go to the GPU in the dtype they come in --, or 'float16': ``prepare``
        rounds them to float16 on the host, before padding, and uploads half the bytes; the forward reads them as they are
        (``model.half_features``).  The proposals then are those of features rounded to float16."""
        self.opt, self.model = opt, model
        if feature_dtype is not None and not any(feature_dtype is x or (isinstance(feature_dtype, str) and feature_dtype == x)
                                                 for x in ('float16', 'half', torch.float16, np.float16)):
            raise ValueError(f"feature_dtype {feature_dtype!r}: None (as the features come) or 'float16'")
        self.feature_dtype = None if feature_dtype is None else torch.float16
        if expert not in ('dense', 'selected'):
            raise ValueError(f"expert {expert!r}: 'dense' or 'selected'")
        if expert_fn is not None and expert != 'selected':
            raise ValueError("expert_fn is the source of the selected clips' features: it needs expert='selected'")
        if select_videos and expert != 'selected':
            raise ValueError("select_videos groups the videos of the selected-clip route: it needs expert='selected'")
        self.expert, self.expert_fn, self.select_videos = expert, expert_fn, bool(select_videos)
        mo = opt['model']
        self.max_vid_len = mo['max_vid_len']
        self.vid_stride = mo.get('vid_stride', 1)
        self.num_fpn_levels = mo['num_fpn_levels']
        self.mha_win_size = mo['mha_win_size']
        assert self.max_vid_len % min_chunk_size(self.num_fpn_levels, self.mha_win_size) == 0, \
            'max video length must be a multiple of the chunk size'            # worker_v2.py:778-780
        ev = opt['eval']
        self.pre_nms_topk, self.pre_nms_thresh, self.seg_len_thresh = ev['pre_nms_topk'], ev['pre_nms_thresh'], ev['seg_len_thresh']
        self.nms_cfg = dict(opt['nms'])
        self.time_dict = defaultdict(list)
        self._pinned = {}                              # free pinned host buffers of launch_proposals, by packed shape

    @classmethod
    def from_checkpoint(cls, opt, root=None, ckpt=None, device='cuda', feature_dtype=None):
        """What ``Evaluator.__init__`` + ``load_model`` do for the model (libs/worker_v2.py:747-749, 806-812): build it with
        ``create_model(opt)``, load ``<root>/models/<ckpt>.pth``['model_ema'] (a checkpoint written by the reference's
        ``Trainer``: the state_dict names are the parameter ABI), move it to the GPU, eval mode, no gradients.
        ``root`` / ``ckpt`` default to ``opt['_root']`` / ``opt['_ckpt']`` like the reference (eval.py:29-36)."""
        from . import modeling
        root = root if root is not None else opt['_root']
        ckpt = ckpt if ckpt is not None else opt['_ckpt']
        path = os.path.join(root, 'models', f'{ckpt}.pth')
        state = torch.load(path, map_location='cpu')
        if 'model_ema' not in state:
            raise KeyError(f"{path}: no 'model_ema' entry (keys: {sorted(state)})")
        model = modeling.create_model(opt)
        model.load_state_dict(state['model_ema'])
        model = model.to(device).eval().requires_grad_(False)
        return cls(opt, model, feature_dtype=feature_dtype)

    @staticmethod
    def _to_half(x, what, name):
        """x rounded to float16 on the host; a finite value that leaves the float16 range (|x| > 65504) is an error, not an inf"""
        if x.dtype == torch.float16:
            return x
        h = x.to(torch.float16)
        bad = ~torch.isfinite(h) & torch.isfinite(x)
        if bool(bad.any()):
            raise ValueError(f'video {name}: {int(bad.sum())} finite values of {what} (max |x| = {float(x[bad].abs().max()):.6g}) leave the float16 '
                             f'range (65504): these features cannot be evaluated with feature_dtype=\'float16\'')
        return h

    @torch.no_grad()
    def prepare(self, data, model=None):
        """pad -> encode_text (worker_v2.py:930-996): the argument tuple of ``model.forward`` for one video, its padded length
        and the padded external scores (or None)."""
        model_ = model or self.model
        dev = next(model_.parameters()).device
        t0 = time.perf_counter()
        tokens = data['text'] if isinstance(data['text'], (tuple, list)) else (data['text'],)
        texts, tmasks = [], []
        for tok in tokens:
            tok = tok[None].to(dev, non_blocking=True)
            m = torch.ones(1, 1, tok.size(-1), dtype=torch.bool, device=dev)
            t, m = model_.encode_text(tok, m)
            texts.append(t)
            tmasks.append(m)
        bank = data.get('bank') if isinstance(data, dict) else None
        if bank is not None:
            # an item of data.EvalBank: the features never left the GPU.  The padded windows and the mask are one ragged transpose
            # each (dcf_op_assemble_rows) out of the bank, the tokens and text_cls are views of it; nothing is uploaded
            if bank.vid_stride != self.vid_stride:
                raise ValueError(f'the EvalBank was filled for vid_stride {bank.vid_stride}, the model has {self.vid_stride}')
            if self.feature_dtype is not None and bank.data['vid'].dtype != self.feature_dtype:
                raise ValueError(f"feature_dtype='float16' rounds host features; the EvalBank holds {bank.data['vid'].dtype} as stored")
            T = padded_length(data['vid_len'], self.max_vid_len, self.num_fpn_levels, self.mha_win_size, self.vid_stride)
            window, shallow_window, mask = bank.windows(data['clip_id'], T)
            self.time_dict['prepare'].append(time.perf_counter() - t0)
            return (window, shallow_window, mask, tuple(texts), data['text_cls'], tuple(tmasks)), T, None
        shallow = data['shallow_vid']
        # expert='selected' with an expert_fn: the sample needs no dense expert features, and none are uploaded
        vid = None if self.expert == 'selected' and self.expert_fn is not None else data['vid']
        if self.feature_dtype is not None:
            name = data.get('clip_id', '?') if isinstance(data, dict) else '?'
            vid, shallow = None if vid is None else self._to_half(vid, 'vid', name), self._to_half(shallow, 'shallow_vid', name)
        vid_len = shallow.size(-1)
        T = padded_length(vid_len, self.max_vid_len, self.num_fpn_levels, self.mha_win_size, self.vid_stride)
        window = None if vid is None else F.pad(vid, (0, T - vid_len))[None].to(dev, non_blocking=True)
        shallow_window = F.pad(shallow, (0, T - vid_len))[None].to(dev, non_blocking=True)
        mask = (torch.arange(T, device=dev).view(1, -1) < vid_len)
        text_cls = data['text_cls'].to(dev, non_blocking=True)
        # external per-clip scores (NQ, vid_len), zero-padded like the features (worker_v2.py:964-967,992-994)
        ext = data.get('ext_scores') if isinstance(data, dict) else None
        ext = None if ext is None else F.pad(ext.float(), (0, T - vid_len)).to(dev, non_blocking=True)
        self.time_dict['prepare'].append(time.perf_counter() - t0)
        return (window, shallow_window, mask, tuple(texts), text_cls, tuple(tmasks)), T, ext

    @torch.no_grad()
    def forward(self, data, model=None):
        """data: vid (D,T), shallow_vid (D,T), text: tuple of (C_t, Lq) token tensors, text_cls (NQ,D).
        Returns the flat device outputs (logits (NQ,S), offsets (NQ,S,2), masks (NQ,S)) and T_padded.
        ``model``: a ``self.model.replica()`` when several videos are kept in flight (``run(n_streams > 1)``)."""
        model_ = model or self.model
        args, T, self._window_ext = self.prepare(data, model_)
        t0 = time.perf_counter()
        if self.select_videos:                        # a group of one video: the same route as run(batch_videos=N), scat included
            out = self._forward_group([(data, args, T, self._window_ext)], model_)[0]
        else:
            out = self._forward_selected(data, model_, args) if self.expert == 'selected' else model_(*args, eval=True)
        self.time_dict['forward'].append(time.perf_counter() - t0)
        self.outputs = out
        return model_._last_flat, T

    def _expert_rows(self, data, clips_host, count, half):
        """``expert_fn``'s rows for the ``count`` clips ``clips_host`` of one video, checked and in the type the forward takes (half: the
        shallow features are float16), on whatever device ``expert_fn`` left them"""
        rows = self.expert_fn(data, clips_host)
        if not torch.is_tensor(rows) or rows.dim() != 2 or rows.size(0) != count:
            raise ValueError(f'expert_fn returned {tuple(rows.shape) if torch.is_tensor(rows) else type(rows).__name__} for {count} clips: '
                             f'one row of D features per clip is expected')
        if self.feature_dtype is not None:
            return self._to_half(rows, 'the expert rows', data.get('clip_id', '?') if isinstance(data, dict) else '?')
        return rows if half else rows.float()

    def _forward_selected(self, data, model_, args):
        """the two-call pattern on one forward window: select_clips -> the rows of the selected clips -> forward_selected"""
        if isinstance(data, dict) and data.get('bank') is not None:
            raise NotImplementedError("expert='selected' does not take the items of a data.EvalBank (they hold dense features on the device)")
        window, shallow_window, mask, texts, text_cls, tmasks = args
        sel = model_.select_clips(shallow_window, mask, text_cls)
        if self.expert_fn is None:
            rows = model_.gather_clip_rows(window, sel)
        else:
            rows = self._expert_rows(data, sel.clips_host(), sel.count, shallow_window.dtype == torch.float16)
            rows = rows.to(shallow_window.device, non_blocking=True)
        self.last_selection = sel
        return model_.forward_selected(rows, sel, shallow_window, mask, texts, tmasks)

    def _forward_group(self, pending, model=None):
        """one forward for the videos of ``pending`` ((data, args, T, ext) each, one padded length); the outputs are model._last_flat"""
        videos = [p[1] for p in pending]
        model_ = model or self.model
        if not self.select_videos:
            return model_.forward_videos(videos)
        for data, _, _, _ in pending:
            if isinstance(data, dict) and data.get('bank') is not None:
                raise NotImplementedError("expert='selected' does not take the items of a data.EvalBank (they hold dense features on the device)")
        batch = model_.select_clips_videos(videos)
        if self.expert_fn is None:
            rows = model_.gather_clip_rows_videos([a[0] for a in videos], batch)
        else:
            half = videos[0][1].dtype == torch.float16
            parts = []
            for v, (data, _, _, _) in enumerate(pending):
                parts.append(self._expert_rows(data, batch.clips_host(v), batch.counts[v], half))
            dev = videos[0][1].device
            if any(r.is_cuda for r in parts):
                rows = torch.cat([r.to(dev, non_blocking=True) for r in parts])
            else:
                rows = torch.cat(parts).to(dev, non_blocking=True)           # host rows: packed on the host, ONE upload
        self.last_selection = batch
        return model_.forward_videos_selected(rows, batch, videos)

    @torch.no_grad()
    def launch_proposals(self, flat, T, data=None, window_ext=None):
        """Enqueue _collect_segments + batched_nms for every query of a video and the ONE device -> host copy of the kept rows
        (<= max_num_segs segments + scores + count per query) into pinned memory, without waiting for any of it.  Returns a
        handle for ``finish_proposals``; the caller may launch the next video's forward first, so that the host-side wait and
        the launch latency of the next forward overlap with GPU work (``run`` does)."""
        logits, offsets, masks = flat
        t0 = time.perf_counter()
        # the pyramid (and its points) starts at T / vid_stride (video_net.py:59-74); segments go back to input clips in finish_proposals
        assert window_ext is None or self.vid_stride == 1, 'ext_scores are per input clip: the reference multiplies them at level 0 (worker_v2.py:1150-1156)'
        segs, scores, counts = _nms.collect_segments(logits, offsets, masks, T // self.vid_stride, self.num_fpn_levels, self.pre_nms_thresh,
                                                     self.pre_nms_topk, self.seg_len_thresh, ext_scores=window_ext)
        self.time_dict['post_process'].append(time.perf_counter() - t0)
        cfg = self.nms_cfg
        if cfg.get('max_num_segs', 0) <= 0:             # keeps nothing in the reference either (nms.py:144-146): per query on the host
            return ('eager', segs, scores, counts, data)
        t0 = time.perf_counter()
        # every query of the video in one pass on the device
        s_all, c_all, k_all = _nms.batched_nms_queries(segs, scores, counts, **cfg)
        nq, M = c_all.shape
        packed = torch.cat((s_all.reshape(nq, 2 * M), c_all, k_all[:, None].to(c_all.dtype)), 1)
        # the pinned buffer belongs to the handle until finish_proposals has read it, then goes back to the free list of its
        # shape: two handles never share one, whatever order shapes arrive in (nq differs between videos)
        free = self._pinned.setdefault(tuple(packed.shape), [])
        host = free.pop() if free else torch.empty(packed.shape, dtype=packed.dtype, pin_memory=True)
        host.copy_(packed, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        self.time_dict['nms'].append(time.perf_counter() - t0)
        return ('packed', done, host, nq, M, data)

    def finish_proposals(self, handle):
        """Wait for a video's kept rows and turn them into the reference's result list (worker_v2.py:1120-1124)."""
        if handle[0] == 'eager':
            _, segs, scores, counts, data = handle
            counts_h = counts.cpu()
            results = []
            for q in range(segs.shape[0]):
                n = int(counts_h[q])
                s, c = _nms.batched_nms(segs[q, :n], scores[q, :n], **self.nms_cfg)
                results.append({'segments': s.cpu(), 'scores': c.cpu()})
            return results
        _, done, host, nq, M, data = handle
        done.synchronize()                              # the only wait
        packed = host.clone()
        self._pinned.setdefault(tuple(host.shape), []).append(host)      # back to the free list: a later video may take it now
        s_host = packed[:, :2 * M].reshape(nq, M, 2)
        if data is not None:                            # on the <= max_num_segs kept rows, on the host: the same fp32 operations
            s_host = s_host * self.vid_stride
            s_host = (s_host * data['clip_stride'] + 0.5 * data['clip_size']) / data['fps']        # worker_v2.py:1120-1122
            s_host = torch.clamp(s_host, min=0, max=data['duration'])
        results = []
        for q in range(nq):
            k = int(packed[q, 3 * M])
            results.append({'segments': s_host[q, :k], 'scores': packed[q, 2 * M:3 * M][:k]})
        return results

    def generate_proposals(self, flat, T, data=None, window_ext=None):
        """_collect_segments + batched_nms + seconds for every query; results as in worker_v2.py:1124.
        ``window_ext``: padded external scores (NQ, T) on the device (worker_v2.py:1078-1081) or None."""
        return self.finish_proposals(self.launch_proposals(flat, T, data, window_ext))

    def _own_carry(self, on=True):
        """while predict / run are in charge, the model does not raise for the one-pass LayerNorm guard at its next call: the evaluator
        repeats the affected videos (replicas made meanwhile inherit the setting)"""
        self.model._carry_handled_by_caller = bool(on)

    def predict(self, data):
        self._own_carry()
        try:
            return self._predict(data)
        finally:
            self._own_carry(False)

    def _predict(self, data):
        flat, T = self.forward(data)
        res = self.generate_proposals(flat, T, data, self._window_ext)
        if self._carry_tripped([self.model]):       # the host has just synchronised for the proposals: 4 more bytes
            flat, T = self.forward(data)            # one-pass LayerNorm guard: the model runs two-pass launches now, the video is repeated
            res = self.generate_proposals(flat, T, data, self._window_ext)
            self._check_numerics([self.model])
        return res

    def run(self, dataset, counter: RecallCounter = None, n_streams: int = 1, batch_videos: int = 1, loss_meter=None):
        """Evaluator.run (worker_v2.py:815-910) over an iterable of per-video dicts (keys as in
        libs/data/dataset.py:977-994: vid, shallow_vid, text, text_cls, segment, fps, clip_stride, clip_size, duration).
        ``batch_videos > 1``: consecutive videos of the same padded length (every video up to max_vid_len is one) share a
        forward (``model.forward_videos``); same proposals, fewer and larger kernel launches.
        ``counter``: a ``DeviceRecallCounter`` takes the device route (``_run_on_device``): forward, collect_segments, batched NMS and
        dcf_op_recall_update are enqueued per video, in each of the three modes, and nothing is waited for before the counter is read;
        ``dataset`` may then be a ``data.EvalBank``, whose videos never leave the GPU.
        ``loss_meter``: a ``DeviceLossMeter`` of the bank the videos come from; on the device route, in each of the three modes, every
        video's forward is followed by ``loss_meter.update_device`` beside the counting.  The host route refuses it (ValueError:
        ``calc_loss`` per video is the host's validation loss)."""
        if self.expert == 'selected' and batch_videos > 1 and not self.select_videos:
            raise NotImplementedError("expert='selected' runs one video per forward: run(batch_videos=1), or make the evaluator with "
                                      "select_videos=True")
        if loss_meter is not None and not isinstance(counter, DeviceRecallCounter):
            raise ValueError('run(loss_meter=...): the meter fills its table on the device route, run(counter=DeviceRecallCounter(...)); '
                             'calc_loss per video is the host route')
        self._own_carry()
        try:
            return self._run(dataset, counter, n_streams, batch_videos, loss_meter)
        finally:
            self._own_carry(False)

    # ---- the device route: nothing is waited for per video ---------------------------------------------------------------------
    def _count_on_device(self, flat, T, data, window_ext, counter, loss_meter=None):
        """collect_segments + batched NMS + dcf_op_recall_update for every query of a video, enqueued on the current stream: no
        pinned copy, no event, no result list; with a ``loss_meter`` the video's rows of the validation loss first"""
        logits, offsets, masks = flat
        if loss_meter is not None:
            loss_meter.update_device(flat, T, data)
        assert window_ext is None or self.vid_stride == 1, 'ext_scores are per input clip: the reference multiplies them at level 0 (worker_v2.py:1150-1156)'
        segs, scores, counts = _nms.collect_segments(logits, offsets, masks, T // self.vid_stride, self.num_fpn_levels, self.pre_nms_thresh,
                                                     self.pre_nms_topk, self.seg_len_thresh, ext_scores=window_ext)
        nq = segs.shape[0]
        if self.nms_cfg.get('max_num_segs', 0) <= 0:    # keeps nothing (nms.py:144-146): every query is a miss
            counter.add_misses(nq)
            return
        s_all, _, k_all = _nms.batched_nms_queries(segs, scores, counts, **self.nms_cfg)
        meta = data.get('meta')
        if meta is None:                                # a host sample: its 32 bytes per query are the one upload
            meta = torch.from_numpy(query_meta(data['segment'], self.vid_stride, data['clip_stride'], data['clip_size'], data['fps'],
                                               data['duration'])).to(s_all.device, non_blocking=True)
        if meta.shape[0] != nq:
            raise ValueError(f'{nq} queries for {meta.shape[0]} ground-truth segments')
        counter.update_device(s_all, k_all, meta)

    def _pass_on_device(self, dataset, counter, n_streams, batch_videos, loss_meter=None):
        """one pass over the dataset in the mode ``run`` was asked for -> the models that ran"""
        if batch_videos > 1:
            pending = []                              # (data, args, T, ext)

            def flush():
                if not pending:
                    return
                T = pending[0][2]
                self._forward_group(pending)
                logits, offsets, masks = self.model._last_flat
                q = 0
                for data, args, _, ext in pending:
                    n = len(args[3])
                    self._count_on_device((logits[q:q + n], offsets[q:q + n], masks[q:q + n]), T, data, ext, counter, loss_meter)
                    q += n
                pending.clear()

            for data in dataset:
                args, T, ext = self.prepare(data)
                if pending and (pending[0][2] != T or len(pending) == batch_videos):
                    flush()
                pending.append((data, args, T, ext))
            flush()
            return [self.model]
        if n_streams <= 1:
            for data in dataset:
                flat, T = self.forward(data)
                self._count_on_device(flat, T, data, self._window_ext, counter, loss_meter)
            return [self.model]
        # one model replica and one HIP stream per lane; the lanes share the counter (integer atomics), and the caller's stream waits
        # for every lane at the end -- on the device, not on the host
        lanes = [(self.model if i == 0 else self.model.replica(), torch.cuda.Stream()) for i in range(n_streams)]
        main = torch.cuda.current_stream()
        for _, stream in lanes:
            stream.wait_stream(main)                  # behind the counter's reset and whatever made the weights
        for i, data in enumerate(dataset):
            mdl, stream = lanes[i % n_streams]
            with torch.cuda.stream(stream):
                flat, T = self.forward(data, mdl)
                self._count_on_device(flat, T, data, self._window_ext, counter, loss_meter)
        for _, stream in lanes:
            main.wait_stream(stream)
        return [m for m, _ in lanes]

    def _run_on_device(self, dataset, counter, n_streams, batch_videos, loss_meter=None):
        """``run`` with a ``DeviceRecallCounter``.  The one-pass LayerNorm guard cannot be polled per video without a wait: it is
        checked once after the last video, and if it tripped the models run two-pass launches from then on, the counter (and the loss
        meter) is reset and the whole pass is repeated once."""
        if iter(dataset) is dataset:
            raise TypeError('run(counter=DeviceRecallCounter): the dataset is an iterator; the pass may have to be repeated, hand over an iterable')
        if loss_meter is not None:
            loss_meter.use(self.opt)
        models = self._pass_on_device(dataset, counter, n_streams, batch_videos, loss_meter)
        if self._carry_tripped(models):
            counter.reset()
            if loss_meter is not None:
                loss_meter.reset()
            models = self._pass_on_device(dataset, counter, n_streams, batch_videos, loss_meter)
        self._check_numerics(models)
        return counter

    def _run(self, dataset, counter, n_streams, batch_videos, loss_meter=None):
        if isinstance(counter, DeviceRecallCounter):
            return self._run_on_device(dataset, counter, n_streams, batch_videos, loss_meter)
        counter = counter or RecallCounter(self.opt['eval'].get('ranks', (1, 5)), self.opt['eval'].get('iou_threshs', (0.3, 0.5)))
        if batch_videos > 1:
            pending = []                              # (data, args, T, ext)

            def flush():
                if not pending:
                    return
                T = pending[0][2]
                t0 = time.perf_counter()

                def compute():
                    self._forward_group(pending)
                    logits, offsets, masks = self.model._last_flat
                    q, out = 0, []
                    for data, args, _, ext in pending:
                        n = len(args[3])
                        out.append(self.generate_proposals((logits[q:q + n], offsets[q:q + n], masks[q:q + n]), T, data, ext))
                        q += n
                    return out

                results = compute()
                if self._carry_tripped([self.model]):          # (the host has synchronised for the proposals) repeat the group
                    results = compute()
                self.time_dict['forward'].append(time.perf_counter() - t0)
                for res, (data, _, _, _) in zip(results, pending):
                    counter.update(res, data['segment'])
                pending.clear()

            for data in dataset:
                args, T, ext = self.prepare(data)
                if pending and (pending[0][2] != T or len(pending) == batch_videos):
                    flush()
                pending.append((data, args, T, ext))
            flush()
            self._check_numerics([self.model])
            return counter
        if n_streams <= 1:
            # one video per forward like the reference, software-pipelined by one video: the proposals of video i are waited for
            # after the forward of video i + 1 has been launched (same stream: its kernels run after video i's decode / NMS)
            def launch(data):
                flat, T = self.forward(data)
                return self.launch_proposals(flat, T, data, self._window_ext)

            prev = None
            for data in dataset:
                handle = launch(data)
                if prev is not None:
                    res = self.finish_proposals(prev[0])
                    # the one-pass LayerNorm guard, without a wait: the probe of prev's forward has landed (its proposals have); if it
                    # -- or the forward in flight behind it -- tripped, the model switches to two-pass launches and both are repeated
                    if self.model.ln_carry_flag_nowait():
                        torch.cuda.synchronize()
                        self.finish_proposals(handle)          # (gives its pinned buffer back)
                        self._carry_tripped([self.model])
                        res = self.finish_proposals(launch(prev[1]))
                        handle = launch(data)
                    counter.update(res, prev[1]['segment'])
                prev = (handle, data)
            if prev is not None:
                res = self.finish_proposals(prev[0])
                if self._carry_tripped([self.model]):
                    res = self.finish_proposals(launch(prev[1]))
                counter.update(res, prev[1]['segment'])
            self._check_numerics([self.model])
            return counter
        # throughput mode: n_streams videos in flight, one model replica (shared parameters, own workspace) and one HIP
        # stream each; the decode / NMS of a video (host syncs on its own stream only) overlaps the forwards of the others
        lanes = [(self.model if i == 0 else self.model.replica(), torch.cuda.Stream()) for i in range(n_streams)]
        group = []

        def finish():
            results = []
            for stream, mdl, flat, T, data, ext in group:
                with torch.cuda.stream(stream):
                    results.append(self.generate_proposals(flat, T, data, ext))
            if self._carry_tripped([m for m, _ in lanes]):     # (every lane's host wait is behind us) repeat the group, two-pass LayerNorms
                results = []
                for stream, mdl, _, _, data, _ in group:
                    with torch.cuda.stream(stream):
                        flat, T = self.forward(data, mdl)
                        results.append(self.generate_proposals(flat, T, data, self._window_ext))
            for res, entry in zip(results, group):
                counter.update(res, entry[4]['segment'])
            group.clear()

        for data in dataset:
            mdl, stream = lanes[len(group)]
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                flat, T = self.forward(data, mdl)
            group.append((stream, mdl, flat, T, data, self._window_ext))
            if len(group) == n_streams:
                finish()
        finish()
        torch.cuda.synchronize()
        self._check_numerics([m for m, _ in lanes])
        return counter

    @staticmethod
    def _carry_tripped(models):
        """The one-pass LayerNorm guard (dcf_numerics_status & 16: a carried LayerNorm met a row whose mean dwarfs its spread; that forward's
        logits were set to NaN) checked where the host has synchronised anyway.  True: EVERY model now runs the two-pass LayerNorm launches
        (set_ln_carry(False)), the flags are reset, and the caller repeats the forwards since the last check -- the run goes on instead of
        aborting.  The fp16-range bit still raises (nothing to fall back to but another gemm_mode)."""
        tripped = False
        for m in models:
            st = m.numerics_status(reset=False) if hasattr(m, 'numerics_status') else 0
            if st & 1:
                m.numerics_status(reset=True)
                raise RuntimeError("an activation left the fp16 operand range of the f16x3 GEMM mode: results are not valid; "
                                   "set opt.model.gemm_mode = 'bf16x6'")
            tripped = tripped or bool(st & 16)
        if tripped:
            for m in models:
                m.acknowledge_ln_carry()
        return tripped

    @staticmethod
    def _check_numerics(models):
        """the f16x3 GEMM mode flags operands beyond the fp16 range (|a| >= 4094) instead of passing inf / NaN on"""
        for m in models:
            st = m.numerics_status(reset=True) if hasattr(m, 'numerics_status') else 0
            if st & 1:
                raise RuntimeError("an activation left the fp16 operand range of the f16x3 GEMM mode: results are not valid; "
                                   "set opt.model.gemm_mode = 'bf16x6'")
            if st & 16:
                for mm in models:
                    mm.set_ln_carry(False)
                raise RuntimeError("a LayerNorm carried between kernels as one-pass row statistics met a row whose mean dwarfs its spread: "
                                   "results are not valid; the model now runs two-pass LayerNorm launches (set_ln_carry(False)) -- run again")
