"""Real-data side of the evaluation harness: the feature-file formats, the text-CLS table, the
annotation file and the per-video dict of the reference's video-centric dataset, as far as ``Evaluator.run`` consumes them
(libs/data/dataset.py).  Pure host code (numpy / torch CPU tensors): the tensors it yields are what
``GroundingEvaluator.predict`` / ``run`` take.

    clip features      VID_LOAD_FUNC, dataset.py:107-135: '<id>.npy' (T, C), '<id>.pt' (T, C) tensor, '<id>.pk' = pickled
                       sequence of (T, C) arrays ('pk0' / 'pk1' pick an entry, 'pk_avg' averages the first two)
    video features     _load_vid_feats, dataset.py:362-408: several feature sources of one video aligned (the shorter ones
                       padded by repeating their last clip, lengths may differ by <= 10), concatenated along channels,
                       temporally down-sampled, returned channel-major (C, T), optionally L2-normalised per clip
    text features      _load_text_feats, dataset.py:460-484: '<text_id>.npy' (L, C) -> (C, L)
    text-CLS table     dataset.py:556-560, 671-678: np.save'd dict sentence -> (1, D) array, one file per split
    annotations        _parse_annotations, dataset.py:287-353: {split: {video: {fps, num_frames, [duration], annotations:
                       [{segment, sentence, [sentence_id]}]}}}; segments clipped to [0, duration], empty ones dropped
    per-video dict     __getitem__, dataset.py:977-994 (eval: every query of a video in one sample, :599-603)

The training side, further down: ``VideoCentricTrainData`` (what the reference's training dataset decides: groups, windows, targets;
host code), ``collate_host`` (the Trainer's collate on CPU tensors), ``FeatureBank`` (the features of a training set in device memory,
filled once) and ``TrainLoader`` (batches for ``train.TrainStep.step``, assembled on the GPU by dcf_op_assemble_rows,
include/decafnet_hip_batch.h, or on the host route); and ``EvalBank``, the validation set in device memory for the evaluations of a
training run (``train.fit``), whose items ``GroundingEvaluator.prepare`` takes in place of host samples.
"""
from __future__ import annotations

import json
import os
import pickle
import random
from collections import OrderedDict
from typing import Dict, Iterator, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

FEATURE_FORMATS = ('npy', 'pt', 'pk0', 'pk1', 'pk_avg')


def feature_dtype(dtype):
    """The ``dtype`` argument of the feature loaders as one of np.float32, np.float16 or 'stored'; anything else is refused."""
    if isinstance(dtype, str) and dtype == 'stored':
        return 'stored'
    for want, names in ((np.float32, (np.float32, 'float32', torch.float32)), (np.float16, (np.float16, 'float16', 'half', torch.float16))):
        if any(dtype is n or (isinstance(dtype, str) and dtype == n) for n in names) or (isinstance(dtype, np.dtype) and dtype == want):
            return want
    raise ValueError(f"feature dtype {dtype!r}: np.float32 (default), np.float16 or 'stored'")


def _cast_features(a, dtype, always_f32):
    """np.float32: float16 arrays -- and, with ``always_f32`` (the npy format), every array -- become float32, others stay as stored;
    'stored': float16 arrays stay float16, the rest as under np.float32; np.float16: a cast of everything."""
    a = np.asarray(a)
    if dtype is np.float16:
        return a.astype(np.float16)
    if a.dtype == np.float16:
        return a if dtype == 'stored' else a.astype(np.float32)
    return a.astype(np.float32) if always_f32 else a


def load_clip_features(path_without_ext: str, fmt: str = 'npy', dtype=np.float32) -> np.ndarray:
    """One feature source of one video as stored on disk: (T, C).  ``dtype``: np.float32 (default) hands float16 files on as
    float32; 'stored' keeps them float16 -- half the bytes from here to the GPU, ``forward(..., eval=True)`` reads them as they
    are --; np.float16 casts whatever is stored."""
    dtype = feature_dtype(dtype)
    if fmt == 'npy':
        return _cast_features(np.load(path_without_ext + '.npy'), dtype, True)
    if fmt == 'pt':
        return _cast_features(torch.load(path_without_ext + '.pt').numpy(), dtype, False)
    if fmt in ('pk0', 'pk1', 'pk_avg'):
        with open(path_without_ext + '.pk', 'rb') as fh:
            entries = pickle.load(fh)
        if fmt == 'pk_avg':
            return _cast_features((entries[0] + entries[1]) / 2, dtype, False)
        return _cast_features(entries[int(fmt[2])], dtype, False)
    raise NotImplementedError(f'feature format {fmt!r}: one of {FEATURE_FORMATS}')


def load_video_features(feat_dirs: Sequence[str], vid_id: str, fmt: str = 'npy', downsample_rate: int = 1,
                        normalize: bool = False, dtype=np.float32) -> torch.Tensor:
    """All feature sources of a video -> (C_total, T) float tensor, the reference's in-memory layout.  ``dtype`` as in
    ``load_clip_features``; float16 features are normalised in fp32 and rounded once."""
    srcs = [load_clip_features(os.path.join(d, vid_id), fmt, dtype) for d in feat_dirs]
    if len(srcs) > 1:
        longest = max(len(a) for a in srcs)
        if longest - min(len(a) for a in srcs) > 10:
            raise ValueError(f'misaligned features ([max] {longest}, [min] {min(len(a) for a in srcs)}) for video {vid_id}')
        srcs = [a if len(a) == longest else np.concatenate((a, np.tile(a[-1], (longest - len(a), 1)))) for a in srcs]
        feats = np.concatenate(srcs, axis=-1)
    else:
        feats = srcs[0]
    if downsample_rate > 1:
        feats = feats[::downsample_rate]
    out = torch.from_numpy(np.ascontiguousarray(feats.transpose()))
    if normalize and out.dtype == torch.float16:
        return F.normalize(out.float(), dim=0).half()
    return F.normalize(out, dim=0) if normalize else out


def load_text_features(text_feat_dir: str, text_id, normalize: bool = False) -> torch.Tensor:
    """Token features of one sentence: (C, L)."""
    a = np.load(os.path.join(text_feat_dir, str(text_id) + '.npy')).astype(np.float32)
    out = torch.from_numpy(np.ascontiguousarray(a.transpose()))
    return F.normalize(out, dim=0) if normalize else out


class TextClsTable:
    """sentence -> sentence-level (CLS) feature, merged over the files of all splits."""

    def __init__(self, fnames: Sequence[str]):
        self.table: Dict[str, np.ndarray] = {}
        for f in fnames:
            self.table.update(np.load(f, allow_pickle=True).item())

    def lookup(self, sentences: Sequence[str]) -> torch.Tensor:
        """(n, D): the rows of the sentences, concatenated like dataset.py:675-677"""
        return torch.from_numpy(np.concatenate([self.table[s] for s in sentences], axis=0))


def parse_annotations(anno_file: str, splits: Sequence[str], downsample_rate: int = 1):
    """-> OrderedDict video -> {fps, num_frames, num_clips, duration, text_ids, segments (n, 2), annotations}."""
    with open(anno_file) as fh:
        anno = json.load(fh)
    merged = {}
    for s in splits:
        if s not in anno:
            raise KeyError(f'split [{s}] does not exist')
        merged.update(anno[s])
    videos = OrderedDict()
    for key, value in merged.items():
        if 'annotations' not in value:
            continue
        fps, num_frames = float(value['fps']), int(value['num_frames'])
        duration = float(value['duration']) if 'duration' in value else num_frames / fps
        num_clips = (value['num_clips'] + downsample_rate - 1) // downsample_rate if 'num_clips' in value else None
        text_ids, segments = [], []
        for i, pair in enumerate(value['annotations']):
            start, end = max(float(pair['segment'][0]), 0), min(float(pair['segment'][1]), duration)
            if end - start <= 0:
                continue
            text_ids.append(pair.get('sentence_id', key + '_{:04d}'.format(i)))
            segments.append((start, end))
        if not text_ids:
            continue
        videos[key] = dict(fps=fps, num_frames=num_frames, num_clips=num_clips, duration=duration, text_ids=tuple(text_ids),
                           segments=np.array(segments), annotations=value['annotations'])
    return videos


class VideoCentricEvalData:
    """Iterable over the evaluation samples of the reference's ``VideoCentricTwoFeatDataset`` (one sample = one video with
    all of its queries), yielding the dict ``Evaluator.simple_predict`` / ``GroundingEvaluator.predict`` consume.

    ``cfg`` carries the ``opt.data`` keys the reference reads: anno_file, eval_split (or split), vid_feat_dir,
    shallow_vid_feat_dir, text_feat_dir, text_cls_fname (with ``{split}``), vid_load, shallow_vid_load, downsample_rate,
    clip_size, clip_stride, normalize_vid, normalize_text, ext_score_dir / normalize_scores / temperature (optional).  Extension key
    ``feature_dtype`` (np.float32, np.float16 or 'stored', see ``load_clip_features``): the dtype ``vid`` / ``shallow_vid`` come in."""

    def __init__(self, cfg):
        g = cfg.get
        splits = g('eval_split', g('split', ('val',)))
        self.splits = (splits,) if isinstance(splits, str) else tuple(splits)
        self.ds = int(g('downsample_rate', 1))
        self.videos = parse_annotations(cfg['anno_file'], self.splits, self.ds)
        self.vid_dirs, self.shallow_dirs = list(cfg['vid_feat_dir']), list(cfg['shallow_vid_feat_dir'])
        self.vid_fmt, self.shallow_fmt = g('vid_load', 'npy'), g('shallow_vid_load', 'npy')
        self.text_dir = cfg['text_feat_dir']
        self.clip_size = g('clip_size', 16)
        self.clip_stride = g('clip_stride', 16) * self.ds                     # dataset.py:240
        self.normalize_vid, self.normalize_text = bool(g('normalize_vid', False)), bool(g('normalize_text', False))
        self.feature_dtype = feature_dtype(g('feature_dtype', np.float32))
        self.ext_score_dir = g('ext_score_dir')
        self.normalize_scores, self.temperature = bool(g('normalize_scores', False)), float(g('temperature', 1.0))
        self.cls = TextClsTable([cfg['text_cls_fname'].format(split=s) for s in self.splits])

    def __len__(self):
        return len(self.videos)

    def sample(self, vid_id: str):
        v = self.videos[vid_id]
        n = len(v['segments'])
        vid = load_video_features(self.vid_dirs, vid_id, self.vid_fmt, self.ds, self.normalize_vid, self.feature_dtype)
        # the sidekick features are stored at the down-sampled rate already (dataset.py:1033,1066-1068)
        shallow = load_video_features(self.shallow_dirs, vid_id, self.shallow_fmt, 1, self.normalize_vid, self.feature_dtype)
        text = tuple(load_text_features(self.text_dir, t, self.normalize_text) for t in v['text_ids'])
        # the reference indexes the raw annotation list with the index of the kept segment (dataset.py:672-674)
        text_cls = self.cls.lookup([v['annotations'][i]['sentence'] for i in range(n)])
        ext: Optional[torch.Tensor] = None
        if self.ext_score_dir is not None:                                   # _load_ext_scores, dataset.py:486-505
            rows = []
            for t in v['text_ids']:
                sc = np.load(os.path.join(self.ext_score_dir, str(t) + '.npy')).astype(np.float32)[::self.ds]
                sc = torch.from_numpy(np.ascontiguousarray(sc))[None]
                rows.append(torch.sigmoid(sc / self.temperature) if self.normalize_scores else sc)
            ext = torch.cat(rows)
        return dict(fps=v['fps'], num_frames=v['num_frames'], duration=v['duration'], segment=v['segments'],
                    clip_size=self.clip_size, clip_stride=self.clip_stride, clip_id=vid_id, text_id=tuple(range(n)),
                    vid=vid, shallow_vid=shallow, text=text, text_cls=text_cls, ext_scores=ext)

    def targets(self, vid_id: str, vid_stride: int = 1):
        """The ground truth of the video's queries on the feature grid, as ``Evaluator._calc_loss`` sees it: (n, 2) float32.
        clip(seg * fps, 0, num_frames) / clip_stride - 0.5 * clip_size / clip_stride in float64, stored as float32
        (dataset.py:706-712), then divided by ``vid_stride`` in float32 (worker_v2.py:1037).  ``sample`` does not carry it."""
        v = self.videos[vid_id]
        seg = np.asarray(v['segments'], dtype=np.float64).reshape(-1, 2)
        seg = np.clip(seg * v['fps'], a_min=0, a_max=v['num_frames']) / self.clip_stride - 0.5 * self.clip_size / self.clip_stride
        return torch.from_numpy(np.ascontiguousarray(seg.astype(np.float32))) / vid_stride

    def __iter__(self) -> Iterator[dict]:
        for vid_id in self.videos:
            yield self.sample(vid_id)


# =====================================================================================================================================
# The training side: the reference's decisions on the host, a feature bank on the GPU, batches assembled by one HIP operator
# =====================================================================================================================================
SHALLOW_WINDOWS = ('same', 'reference')


class VideoCentricTrainData:
    """What the reference's training dataset DECIDES (``VideoCentricTwoFeatDataset`` with ``is_training=True``, libs/data/dataset.py):
    which queries of which video make a sample, which window of the video the sample sees, and where its targets lie on the feature
    grid.  ``decide`` makes no tensors; ``sample`` loads the host tensors of one decision (the host route, ``collate_host``).

    ``cfg`` carries the ``opt.data`` keys of ``VideoCentricEvalData`` (``split`` names the training splits; every video needs
    ``num_clips`` in the annotation file, as in the reference) and the training keys max_vid_len, max_text_len, crop_ratio ((lo, hi) or
    None), trunc_thresh, max_num_text, group_method (accepted; without effect on this path, as in the reference), to_fixed_len and
    tokenizer.  ``to_fixed_len=True`` (interpolated features) and a tokenizer (GloVe) are refused with NotImplementedError before
    anything is read.

    Grouping (_build_train_samples / _group_with_max_len, dataset.py:589-597, 624-666), for all ``num_epochs`` at construction and
    with the tail cut: the worst-case window in seconds from num_clips, crop_ratio[0], clip_stride * downsample_rate, clip_size and
    fps; the first available segment probes a window; ``choice(idx, max_num_text, replace=False)`` where a window holds more queries.
    Targets (dataset.py:1109-1126): clip(seg * fps, 0, num_frames) / clip_stride - 0.5 * clip_size / clip_stride in float64, stored
    as float32.  Video length: min(len(vid), len(shallow)) (:1103-1106).  Window (_truncate_vid_feats, :409-458): the crop_ratio draw
    where the video fits max_vid_len, no window where the draw equals the video, s0 / s1, the threshold 0.2 for an over-long segment,
    up to ``num_trials`` draws of a start with the overlap test, the clamp of the targets into the window, and
    ValueError('no valid truncation found') after the trials.

    The RNG contract.  The object owns ``random.Random(seed)`` and ``np.random.RandomState(seed)`` and calls them where, and in the
    order in which, the reference calls the ``random`` and ``np.random`` modules: ``choice`` while grouping, ``randint`` per
    ``decide`` (one for the crop length, one per trial).  A reference run under ``random.seed(seed); np.random.seed(seed)`` that asks
    for its samples in the same order therefore makes the same decisions bit for bit.  ``decide`` advances the stream: calling it
    twice for one sample gives two draws, as two ``__getitem__`` calls do.

    Shuffling is this project's own (the reference's order depends on DataLoader internals and worker seeds): ``order(epoch, rank,
    world_size)`` is ``torch.randperm(len, generator=Generator().manual_seed(seed + epoch))``, of which rank r of w takes
    ``perm[r::w]`` cut to the common length ``len // w``; ``TrainLoader`` makes batches of ``batch_size`` of it and drops the tail.

    ``shallow_window``.  The reference crops ``vid`` to the window and leaves ``shallow_vid`` uncropped (dataset.py:1132-1134,
    1177-1178): under crop_ratio the streams are ``ws`` clips apart, and the shallow stream of a video longer than max_vid_len does
    not fit the batch buffer.  'same' (default): both streams get the window.  'reference': the shallow stream is the first
    ``vid_len`` clips, and ValueError where the reference's ``copy_`` into the batch buffer would fail."""

    def __init__(self, cfg, num_epochs=1, seed=0, shallow_window='same'):
        g = cfg.get
        if g('to_fixed_len', False):
            raise NotImplementedError('VideoCentricTrainData: to_fixed_len=True (features interpolated to a fixed length) is not implemented')
        if g('tokenizer') is not None:
            raise NotImplementedError('VideoCentricTrainData: a tokenizer (GloVe) is not implemented: pass pre-computed token features')
        if shallow_window not in SHALLOW_WINDOWS:
            raise ValueError(f'shallow_window = {shallow_window!r} (one of {SHALLOW_WINDOWS})')
        if int(num_epochs) < 1:
            raise ValueError(f'num_epochs = {num_epochs!r}')
        splits = g('split', ('train',))
        if isinstance(splits, str):
            splits = splits.split(',') if ',' in splits else (splits,)
        self.splits = tuple(splits)
        self.ds = int(g('downsample_rate', 1))
        self.vid_dirs, self.shallow_dirs = list(cfg['vid_feat_dir']), list(cfg['shallow_vid_feat_dir'])
        self.vid_fmt, self.shallow_fmt = g('vid_load', 'npy'), g('shallow_vid_load', 'npy')
        self.text_dir = cfg['text_feat_dir']
        self.clip_size = g('clip_size', 16)
        self.clip_stride = g('clip_stride', 16) * self.ds                     # dataset.py:240
        self.normalize_vid, self.normalize_text = bool(g('normalize_vid', False)), bool(g('normalize_text', False))
        self.feature_dtype = feature_dtype(g('feature_dtype', np.float32))
        self.max_vid_len, self.max_text_len = int(cfg['max_vid_len']), int(cfg['max_text_len'])
        crop = g('crop_ratio', (0.9, 1.0))
        if crop is not None and not (isinstance(crop, (list, tuple)) and len(crop) == 2):
            raise ValueError(f'crop_ratio = {crop!r}: (lo, hi) or None')
        self.crop_ratio = None if crop is None else tuple(crop)
        self.trunc_thresh = g('trunc_thresh', 0.5)
        self.max_num_text = g('max_num_text')
        self.group_method = g('group_method', 'greedy')
        self.shallow_window = shallow_window
        self.num_epochs, self.seed = int(num_epochs), int(seed)
        self.videos = parse_annotations(cfg['anno_file'], self.splits, self.ds)
        self.cls = TextClsTable([cfg['text_cls_fname'].format(split=s) for s in self.splits])
        self.rng, self.np_rng = random.Random(self.seed), np.random.RandomState(self.seed)
        samples = []
        for _ in range(self.num_epochs):                                      # all epochs up front, unshuffled (dataset.py:589-597)
            for vid_id in self.videos:
                samples.extend(self._group(vid_id))
        self.samples = tuple(samples[:len(samples) // self.num_epochs * self.num_epochs])
        self._feats, self._lengths = {}, {}                                   # the reference's vid_feat_dict / shallow_vid_feat_dict

    def __len__(self):
        return len(self.samples) // self.num_epochs

    # ---- grouping ------------------------------------------------------------------------------------------------------------
    def _group(self, vid_id):
        v = self.videos[vid_id]
        if v['num_clips'] is None:
            raise ValueError(f'video {vid_id}: the annotation has no num_clips, which the grouping reads (dataset.py:628)')
        if v['num_clips'] <= self.max_vid_len:
            win_len = v['num_clips']
            if self.crop_ratio is not None:
                win_len = max(np.ceil(self.crop_ratio[0] * win_len), 1)
        else:
            win_len = self.max_vid_len
        win_len = (self.clip_stride * (win_len - 1) + self.clip_size) / v['fps']          # seconds
        sort_idx = np.argsort(v['segments'][:, 0])
        segments = v['segments'][sort_idx]
        mask = np.ones(len(segments), dtype=bool)
        samples = []
        while mask.sum() > 0:
            ptr = np.nonzero(mask)[0].min()                                   # the first available segment probes
            ws, we = segments[ptr, 0], segments[ptr, 0] + win_len
            if segments[ptr, 1] - segments[ptr, 0] > win_len:
                idx = np.array([ptr])                                         # a segment longer than the window, alone
            else:
                idx = np.nonzero((segments[:, 0] >= ws) & (segments[:, 1] <= we) & mask)[0]
                if self.max_num_text is not None and len(idx) > self.max_num_text:
                    idx = self.np_rng.choice(idx, self.max_num_text, replace=False)
            samples.append((vid_id, tuple(int(i) for i in sort_idx[idx])))
            mask[idx] = 0
        return samples

    # ---- one sample ------------------------------------------------------------------------------------------------------------
    def video_streams(self, vid_id):
        """-> (vid (C, T_v), shallow (C_s, T_s)) as the loaders give them, uncropped; cached on the host as the reference caches them"""
        if vid_id not in self._feats:
            vid = load_video_features(self.vid_dirs, vid_id, self.vid_fmt, self.ds, self.normalize_vid, self.feature_dtype)
            # the sidekick features are stored at the down-sampled rate already (dataset.py:1033, 1066-1068)
            shallow = load_video_features(self.shallow_dirs, vid_id, self.shallow_fmt, 1, self.normalize_vid, self.feature_dtype)
            self._feats[vid_id] = (vid, shallow)
            self._lengths[vid_id] = min(vid.size(1), shallow.size(1))
        return self._feats[vid_id]

    def video_length(self, vid_id):
        """min(len(vid), len(shallow)) (dataset.py:1103-1106); ``FeatureBank`` records it while it fills"""
        if vid_id not in self._lengths:
            self.video_streams(vid_id)
        return self._lengths[vid_id]

    def token_features(self, text_id):
        """(C_t, L) cut to max_text_len (dataset.py:477-478; the cut commutes with the per-token normalisation)"""
        return load_text_features(self.text_dir, text_id, self.normalize_text)[:, :self.max_text_len]

    def sentences(self, vid_id, seg_idx):
        """the reference indexes the RAW annotation list with the index of the kept segment (dataset.py:672-675)"""
        return [self.videos[vid_id]['annotations'][i]['sentence'] for i in seg_idx]

    def _truncate(self, vid_len, segments, offset, num_trials):
        """_truncate_vid_feats on the length alone -> (segments, [ws, we] or None); torch's float32 arithmetic as the reference runs it"""
        max_vid_len = self.max_vid_len
        if vid_len <= max_vid_len:
            if self.crop_ratio is None:
                return segments, None
            max_vid_len = self.rng.randint(int(max(np.ceil(self.crop_ratio[0] * vid_len), 1)),
                                           int(min(np.ceil(self.crop_ratio[1] * vid_len), vid_len)))
            if max_vid_len == vid_len:
                return segments, None
        s0 = int(max(0, np.floor(float(segments[:, 0].max() - max_vid_len))))
        s1 = int(min(vid_len - max_vid_len, np.ceil(float(segments[:, 1].min()))))
        if s0 > s1:
            raise ValueError(f'no valid truncation found: the range of window starts [{s0}, {s1}] is empty')
        seg_lens = torch.clamp(segments[:, 1] - segments[:, 0], min=1e-5)
        trunc_thresh = 0.2 if seg_lens.max() > (self.max_vid_len / self.trunc_thresh) else self.trunc_thresh
        for _ in range(num_trials):
            ws = self.rng.randint(s0, s1)
            we = ws + max_vid_len
            start = torch.clamp(segments[:, 0], min=ws - offset)
            end = torch.clamp(segments[:, 1], max=we + offset)
            overlap = torch.clamp(end - start, min=0)
            if torch.all(overlap / seg_lens > trunc_thresh):
                return torch.clamp(segments - ws, min=-offset, max=we - ws + offset), [ws, we]
        raise ValueError('no valid truncation found')

    def decide(self, epoch, idx, num_trials=5000):
        """-> (vid_id, seg_idx, [ws, we] or None, targets (n, 2) float32 in grid units of the window).  The video's length is
        taken from the features the first time a video is met (``FeatureBank`` has met them all) and remembered."""
        if not (0 <= epoch < self.num_epochs and 0 <= idx < len(self)):
            raise IndexError(f'sample {idx} of epoch {epoch}: {len(self)} samples, {self.num_epochs} epochs')
        vid_id, seg_idx = self.samples[epoch * len(self) + idx]
        v = self.videos[vid_id]
        vid_len = self.video_length(vid_id)
        offset = 0.5 * self.clip_size / self.clip_stride
        seg = np.clip(v['segments'][np.array(seg_idx)] * v['fps'], a_min=0, a_max=v['num_frames']) / self.clip_stride - offset
        seg = torch.from_numpy(np.ascontiguousarray(seg.astype(np.float32)))
        seg, window = self._truncate(vid_len, seg, offset, num_trials)
        return vid_id, seg_idx, window, seg.numpy()

    def stream_windows(self, vid_len, window):
        """-> ((v0, v1), (s0, s1)): the clips of ``vid`` and of ``shallow_vid`` a sample holds"""
        vw = (0, vid_len) if window is None else (int(window[0]), int(window[1]))
        return vw, (vw if self.shallow_window == 'same' else (0, vid_len))

    def sample(self, epoch, idx, num_trials=5000):
        """the host tensors of one decision, with the reference's keys: vid (C, n), shallow_vid, text (tuple of (C_t, L)), text_cls
        (n, D), target (n, 2), and window"""
        vid_id, seg_idx, window, target = self.decide(epoch, idx, num_trials)
        vid, shallow = self.video_streams(vid_id)
        (v0, v1), (s0, s1) = self.stream_windows(self.video_length(vid_id), window)
        v = self.videos[vid_id]
        return dict(clip_id=vid_id, text_id=seg_idx, window=window, target=torch.from_numpy(target),
                    vid=vid[:, v0:v1], shallow_vid=shallow[:, s0:s1],
                    text=tuple(self.token_features(v['text_ids'][i]) for i in seg_idx),
                    text_cls=self.cls.lookup(self.sentences(vid_id, seg_idx)))

    # ---- the random streams ----------------------------------------------------------------------------------------------------
    def rng_state(self):
        """the state of both generators of the RNG contract, as plain picklable Python / numpy objects"""
        return {'random': self.rng.getstate(), 'numpy': self.np_rng.get_state()}

    def set_rng_state(self, state):
        """put back what ``rng_state`` returned: the next ``decide`` draws what it would have drawn then"""
        if not isinstance(state, dict) or set(state) != {'random', 'numpy'}:
            raise ValueError("set_rng_state: a dict with the keys 'random' and 'numpy', as rng_state() returns it")
        r = state['random']
        self.rng.setstate((r[0], tuple(r[1]), r[2]))                          # a list after a round trip through some formats
        self.np_rng.set_state(state['numpy'])
        return self

    # ---- order -----------------------------------------------------------------------------------------------------------------
    def order(self, epoch, rank=0, world_size=1):
        """this project's shuffling rule (class docstring) -> the sample indices of ``rank`` in ``epoch``, a list of ints"""
        if not 0 <= rank < world_size:
            raise ValueError(f'rank {rank} of {world_size}')
        perm = torch.randperm(len(self), generator=torch.Generator().manual_seed(self.seed + int(epoch)))
        return perm[rank::world_size][:len(self) // world_size].tolist()


def _pad_rows(rows, width, what):
    """[(C, n_i)] -> ((len, C, width) zero-padded in the rows' dtype, (len, width) bool): _batchify_videos / _batchify_text"""
    lens = [r.size(-1) for r in rows]
    if max(lens) > width:
        raise ValueError(f'{what}: {max(lens)} positions do not fit the batch buffer of {width} '
                         f'(where the reference\'s copy_ fails; shallow_window=\'same\' crops both streams)')
    out = rows[0].new_full((len(rows), rows[0].size(0), width), 0.)
    for i, r in enumerate(rows):
        out[i, :, :lens[i]].copy_(r)
    return out, torch.arange(width)[None] < torch.as_tensor(lens)[:, None]


def collate_host(samples, input_vid_len, max_text_len, vid_stride=1):
    """The host route: ``Trainer._batchify_videos`` / ``_batchify_text`` / ``_batchify`` and worker_v2.py:402-418 on CPU tensors.
    ``samples``: dicts of ``VideoCentricTrainData.sample``.  -> the dict ``TrainStep.step`` takes -- vid / shallow (bs, D, T) in the
    features' dtype, vid_masks (bs, T), tokens (B', C_t, Lmax) flattened over ``text_size`` rather than padded to the largest query
    count, text_cls (B', D), token_masks (B', 1, Lmax), text_size (bs,) int64 (it stays on the host: the step reads it there) --
    plus 'targets' = target / vid_stride (B', 2)."""
    vid, vid_masks = _pad_rows([s['vid'] for s in samples], input_vid_len, 'vid')
    shallow, _ = _pad_rows([s['shallow_vid'] for s in samples], input_vid_len, 'shallow_vid')
    tokens, token_masks = _pad_rows([t[:, :max_text_len] for s in samples for t in s['text']], max_text_len, 'text')
    return dict(vid=vid, shallow=shallow, vid_masks=vid_masks, tokens=tokens, text_cls=torch.cat([s['text_cls'] for s in samples]),
                token_masks=token_masks[:, None], text_size=torch.as_tensor([len(s['text']) for s in samples]),
                targets=torch.cat([s['target'] / vid_stride for s in samples]))


_TORCH_OF = {np.dtype(np.float16): torch.float16, np.dtype(np.float32): torch.float32}


class FeatureBank:
    """Every feature a training run reads, in device memory, filled once: the streams ``vid``, ``shallow`` and ``text`` of
    ``train_data``'s videos and sentences, loaded with the loaders' own rules (several sources aligned and concatenated,
    ``downsample_rate`` for ``vid`` only, ``normalize_*``, ``feature_dtype``; token features cut to max_text_len).  A stream is ONE
    device buffer of rows stored as the files store them, row-major (T_v, C), back to back; ``rows[stream]`` maps a video id (a
    text id) to (first row, number of rows) and ``row_offsets[stream]`` is the int64 table of first rows on the host.  The text-CLS
    table is one (N, D) device tensor, ``cls_row`` maps a sentence to its row.

    One dtype per stream; a float16 / fp32 pair of ``vid`` and ``shallow`` is refused as ``modeling._check_feature_dtypes`` refuses
    it.  ``max_bytes``: ValueError with the size the bank would need where that is more; nothing is uploaded then.  ``nbytes``: what
    the bank holds.  Sizing: T_v * C * element size per stream and video -- 2 h of 1024-channel float16 features at 1.875 clips / s
    are 27 MB; a whole training set of pre-computed features is a few GB of an MI355X's 288."""

    STREAMS = ('vid', 'shallow', 'text')

    def __init__(self, train_data, device='cuda', max_bytes=None):
        td = self.train_data = train_data
        host = {s: [] for s in self.STREAMS}
        self.rows = {s: {} for s in self.STREAMS}
        n = dict.fromkeys(self.STREAMS, 0)

        def add(stream, key, cm):                                  # cm: (C, T) as the loaders return it -> rows (T, C)
            a = cm.t().contiguous()
            if host[stream] and (a.dtype != host[stream][0].dtype or a.size(1) != host[stream][0].size(1)):
                raise ValueError(f'{stream} features of {key}: {a.dtype} x {a.size(1)} channels in a stream of {host[stream][0].dtype} x '
                                 f'{host[stream][0].size(1)} (one dtype and one width per stream)')
            host[stream].append(a)
            self.rows[stream][key] = (n[stream], a.size(0))
            n[stream] += a.size(0)

        sentences = []
        for vid_id, v in td.videos.items():
            vid, shallow = td.video_streams(vid_id)
            add('vid', vid_id, vid)
            add('shallow', vid_id, shallow)
            for t in v['text_ids']:
                if t not in self.rows['text']:
                    add('text', t, td.token_features(t))
            sentences += [a['sentence'] for a in v['annotations']]
        td._feats.clear()                                                     # the bank holds them now; the lengths stay
        if (host['vid'][0].dtype == torch.float16) != (host['shallow'][0].dtype == torch.float16):
            raise ValueError(f"vid is {host['vid'][0].dtype} and shallow_vid is {host['shallow'][0].dtype}: float16 clip features come as a pair")
        self.cls_row = {}
        for s in sentences:
            if s in td.cls.table:
                self.cls_row.setdefault(s, len(self.cls_row))
        cls = torch.from_numpy(np.concatenate([td.cls.table[s] for s in self.cls_row], axis=0))
        need = sum(a.numel() * a.element_size() for s in self.STREAMS for a in host[s]) + cls.numel() * cls.element_size()
        if max_bytes is not None and need > max_bytes:
            raise ValueError(f'FeatureBank: the features need {need} bytes, max_bytes is {max_bytes} '
                             f'(TrainLoader(bank=None) takes the host route)')
        self.device = torch.device(device)
        self.data = {s: torch.cat(host[s]).to(self.device) for s in self.STREAMS}
        self.cls = cls.to(self.device)
        self.width = {s: self.data[s].size(1) for s in self.STREAMS}
        self.row_offsets = {s: np.array([r0 for r0, _ in self.rows[s].values()], dtype=np.int64) for s in self.STREAMS}
        self.nbytes = need

    def assemble(self, stream, desc, T_out, want_mask=True):
        """dcf_op_assemble_rows on one stream: ``desc`` (B, 2) int64 on the device, (element offset, rows) per window ->
        (out (B, C, T_out) in the stream's dtype, mask (B, T_out) bool or None).  The caller has validated the windows."""
        from . import _lib
        bank = self.data[stream]
        if not bank.is_cuda:
            raise RuntimeError('FeatureBank.assemble runs on the MI355X only: the bank is on the host (collate_host is the host route)')
        B, C = desc.size(0), self.width[stream]
        out = torch.empty(B, C, T_out, dtype=bank.dtype, device=bank.device)
        mask = torch.empty(B, T_out, dtype=torch.bool, device=bank.device) if want_mask else None
        _lib.check(_lib.lib().dcf_op_assemble_rows(_lib.ptr(bank), bank.element_size(), _lib.ptr(desc), B, C, T_out, _lib.ptr(out),
                                                   _lib.ptr(mask), _lib.current_stream()), 'dcf_op_assemble_rows')
        return out, mask

    def window(self, stream, key, r0, r1, T_out):
        """-> (element offset, rows) of rows [r0, r1) of ``key``, validated against the video and the batch buffer"""
        first, rows = self.rows[stream][key]
        if not 0 <= r0 <= r1 <= rows:
            raise ValueError(f'{stream} window [{r0}, {r1}) of {key}: the bank holds {rows} rows')
        if r1 - r0 > T_out:
            raise ValueError(f'{stream} of {key}: {r1 - r0} positions do not fit the batch buffer of {T_out} '
                             f'(where the reference\'s copy_ fails; shallow_window=\'same\' crops both streams)')
        return (first + r0) * self.width[stream], r1 - r0


class EvalBank:
    """The validation set in device memory, filled once from a ``VideoCentricEvalData``: the sibling of ``FeatureBank`` for the
    evaluation a training run does between epochs.  The streams ``vid``, ``shallow`` and ``text`` are one device buffer each, rows as
    the files store them (a float16 file stays float16 under ``feature_dtype='stored'``), with the loaders' own rules (sources aligned
    and concatenated, ``downsample_rate`` for ``vid`` only, ``normalize_*``; token features uncut, as ``sample`` hands them on).
    ``cls`` is the (N_queries, D) table of text-CLS rows in query order and ``meta`` the (N_queries, 8) fp32 table of
    ``evaluator.query_meta`` -- ground truth, strides, fps, duration -- that dcf_op_recall_update reads; ``vid_stride`` is the
    model's (``opt.model.vid_stride``), which the evaluator checks.

    Iterating yields one dict per video, in the order of ``eval_data.videos``, that ``GroundingEvaluator.prepare`` / ``run`` take in
    place of a host sample: the host scalars of ``VideoCentricEvalData.sample`` (fps, duration, segment, clip_size, clip_stride,
    clip_id, ...), ``text`` as (C_t, L) views of the bank, ``text_cls`` and ``meta`` as slices of the tables, ``vid_len`` and
    ``bank``.  ``prepare`` asks ``windows(clip_id, T)`` for the padded (1, D, T) windows and the mask: two launches of
    dcf_op_assemble_rows on descriptors that were uploaded with the bank, so a video costs no upload at all.

    Refused: ``ext_score_dir`` (NotImplementedError: external scores stay on the host route), a video whose ``vid`` and ``shallow``
    streams differ in length (the host route pads them apart), a float16 / fp32 pair.  ``max_bytes`` / ``nbytes`` as ``FeatureBank``."""

    STREAMS = FeatureBank.STREAMS

    def __init__(self, eval_data, vid_stride=1, device='cuda', max_bytes=None):
        from .evaluator import query_meta
        ed = self.eval_data = eval_data
        if ed.ext_score_dir is not None:
            raise NotImplementedError(f'EvalBank: ext_score_dir = {ed.ext_score_dir!r} is not implemented: external scores are read '
                                      f'per video on the host route (GroundingEvaluator.run on the VideoCentricEvalData itself)')
        self.vid_stride = int(vid_stride)
        host = {s: [] for s in self.STREAMS}
        self.rows = {s: {} for s in self.STREAMS}
        n = dict.fromkeys(self.STREAMS, 0)

        def add(stream, key, cm):                                  # cm: (C, T) as the loaders return it -> rows (T, C)
            a = cm.t().contiguous()
            if host[stream] and (a.dtype != host[stream][0].dtype or a.size(1) != host[stream][0].size(1)):
                raise ValueError(f'{stream} features of {key}: {a.dtype} x {a.size(1)} channels in a stream of {host[stream][0].dtype} x '
                                 f'{host[stream][0].size(1)} (one dtype and one width per stream)')
            host[stream].append(a)
            self.rows[stream][key] = (n[stream], a.size(0))
            n[stream] += a.size(0)

        cls, meta, self.queries, q0 = [], [], {}, 0
        for vid_id, v in ed.videos.items():
            vid = load_video_features(ed.vid_dirs, vid_id, ed.vid_fmt, ed.ds, ed.normalize_vid, ed.feature_dtype)
            shallow = load_video_features(ed.shallow_dirs, vid_id, ed.shallow_fmt, 1, ed.normalize_vid, ed.feature_dtype)
            if vid.size(1) != shallow.size(1):
                raise ValueError(f'video {vid_id}: vid has {vid.size(1)} clips and shallow_vid {shallow.size(1)}; the bank pads both to one length')
            add('vid', vid_id, vid)
            add('shallow', vid_id, shallow)
            for t in v['text_ids']:
                if t not in self.rows['text']:
                    add('text', t, load_text_features(ed.text_dir, t, ed.normalize_text))
            nq = len(v['segments'])
            cls.append(ed.cls.lookup([v['annotations'][i]['sentence'] for i in range(nq)]))       # as ``sample`` indexes them
            meta.append(query_meta(v['segments'], self.vid_stride, ed.clip_stride, ed.clip_size, v['fps'], v['duration']))
            self.queries[vid_id] = (q0, nq)
            q0 += nq
        if not host['vid']:
            raise ValueError('EvalBank: the evaluation split holds no video')
        if (host['vid'][0].dtype == torch.float16) != (host['shallow'][0].dtype == torch.float16):
            raise ValueError(f"vid is {host['vid'][0].dtype} and shallow_vid is {host['shallow'][0].dtype}: float16 clip features come as a pair")
        cls, meta = torch.cat(cls), torch.from_numpy(np.concatenate(meta))
        desc = {s: torch.tensor([[r0 * host[s][0].size(1), rows] for r0, rows in (self.rows[s][k] for k in ed.videos)], dtype=torch.int64)
                for s in ('vid', 'shallow')}
        tables = [cls, meta, desc['vid'], desc['shallow']]
        need = sum(a.numel() * a.element_size() for s in self.STREAMS for a in host[s]) + sum(t.numel() * t.element_size() for t in tables)
        if max_bytes is not None and need > max_bytes:
            raise ValueError(f'EvalBank: the features need {need} bytes, max_bytes is {max_bytes} '
                             f'(GroundingEvaluator.run on the VideoCentricEvalData takes the host route)')
        self.device = torch.device(device)
        self.data = {s: torch.cat(host[s]).to(self.device) for s in self.STREAMS}
        self.cls, self.meta = cls.to(self.device), meta.to(self.device)
        self.desc = {s: d.to(self.device) for s, d in desc.items()}
        self.width = {s: self.data[s].size(1) for s in self.STREAMS}
        self.index = {k: i for i, k in enumerate(ed.videos)}
        self.nbytes = need

    assemble = FeatureBank.assemble

    def __len__(self):
        return len(self.index)

    def windows(self, vid_id, T):
        """-> (vid (1, D, T), shallow (1, D, T), mask (1, T) bool): the video padded with zeros to T columns, the bits of
        ``F.pad`` on the host sample"""
        i, rows = self.index[vid_id], self.rows['vid'][vid_id][1]
        if rows > T:
            raise ValueError(f'video {vid_id}: {rows} clips do not fit a window of {T}')
        vid, mask = self.assemble('vid', self.desc['vid'][i:i + 1], T)
        shallow, _ = self.assemble('shallow', self.desc['shallow'][i:i + 1], T, want_mask=False)
        return vid, shallow, mask

    def item(self, vid_id):
        ed, v = self.eval_data, self.eval_data.videos[vid_id]
        q0, nq = self.queries[vid_id]
        text = tuple(self.data['text'][r0:r0 + rows].t() for r0, rows in (self.rows['text'][t] for t in v['text_ids']))
        return dict(fps=v['fps'], num_frames=v['num_frames'], duration=v['duration'], segment=v['segments'], clip_size=ed.clip_size,
                    clip_stride=ed.clip_stride, clip_id=vid_id, text_id=tuple(range(nq)), vid_len=self.rows['vid'][vid_id][1], bank=self,
                    text=text, text_cls=self.cls[q0:q0 + nq], meta=self.meta[q0:q0 + nq], ext_scores=None)

    def __iter__(self):
        for vid_id in self.index:
            yield self.item(vid_id)

    @property
    def targets(self):
        """(N_queries, 2) fp32 on the device, in query order: ``eval_data.targets(vid_id, vid_stride)`` of every video, what the
        validation loss is computed against (``evaluator.DeviceLossMeter``).  Made at the first use and kept; 8 bytes per query that
        ``nbytes`` does not count."""
        if getattr(self, '_targets', None) is None:
            rows = [self.eval_data.targets(vid_id, self.vid_stride) for vid_id in self.index]
            self._targets = torch.cat(rows).to(self.device)
        return self._targets

    def subset(self, indices):
        """An iterable view of the videos at ``indices`` (positions in the bank's order, each at most once), in the order given: the
        same item dicts, nothing copied.  What a rank evaluates of a sharded validation set (``train.fit_parallel``)."""
        return EvalBankSubset(self, indices)


class EvalBankSubset:
    """``EvalBank.subset``: iterating yields ``bank.item`` of the chosen videos, with the keys ``EvalBank`` yields and no other."""

    def __init__(self, bank, indices):
        ids = list(bank.index)
        idx = [int(i) for i in indices]
        if any(i != j for i, j in zip(idx, indices)) or any(not 0 <= i < len(ids) for i in idx) or len(set(idx)) != len(idx):
            raise ValueError(f'EvalBank.subset: indices {list(indices)} must be distinct integers in [0, {len(ids)})')
        self.bank, self.indices, self._ids = bank, tuple(idx), [ids[i] for i in idx]

    def __len__(self):
        return len(self._ids)

    def __iter__(self):
        for vid_id in self._ids:
            yield self.bank.item(vid_id)


class TrainLoader:
    """Batches for ``TrainStep.step``.  ``epoch(e)`` yields ``(batch, targets)`` -- with ``microbatch_size``, ``(list of batches, list
    of targets)``, sliced as ``forward_backward`` slices them (worker_v2.py:368-372) -- in the order of ``train_data.order(e, rank,
    world_size)``, ``batch_size`` samples each, the tail dropped.  ``len(loader)`` is the ``itrs_per_epoch`` of ``TrainStep``.

    With a ``FeatureBank`` a batch costs the decisions of ``train_data.decide`` on the host, ONE int64 table uploaded (the window
    descriptors of the three streams, the CLS rows, the float32 targets two to a word) and three launches of dcf_op_assemble_rows
    (``vid`` and ``shallow`` into ``input_vid_len`` columns, the token features into ``max_text_len``) plus an index_select on the
    CLS table: no feature byte crosses the host.  ``bank=None``: ``collate_host`` and ``.cuda()``, the same bits.  ``text_size``
    stays on the host either way, where the step reads it.  ``input_vid_len``: the batch's columns, the Trainer's model max_vid_len *
    vid_stride (worker_v2.py:286; default: the data's max_vid_len); ``vid_stride`` divides the targets (worker_v2.py:417).

    ``state()`` / ``load_state()``: the random streams of ``train_data`` for a checkpoint.  While the generator of ``epoch(e)`` has
    not finished, the state is the snapshot taken when it started -- a checkpoint inside an epoch restarts that epoch
    (``train.fit``), so the restarted epoch draws what the interrupted one drew -- and afterwards it is the live state.  The order of
    the samples needs no state: it is a function of the seed and the epoch."""

    def __init__(self, train_data, bank, batch_size, microbatch_size=None, rank=0, world_size=1, input_vid_len=None, vid_stride=1,
                 device='cuda', num_trials=5000):
        if bank is not None and bank.train_data is not train_data:
            raise ValueError('TrainLoader: the bank was filled from another VideoCentricTrainData')
        mb = batch_size if microbatch_size is None else int(microbatch_size)
        if batch_size < 1 or mb < 1:
            raise ValueError(f'batch_size {batch_size}, microbatch_size {microbatch_size}')
        if not 0 <= rank < world_size:
            raise ValueError(f'rank {rank} of {world_size}')
        self.td, self.bank, self.batch_size, self.microbatch_size, self._mb = train_data, bank, int(batch_size), microbatch_size, mb
        self.input_vid_len = train_data.max_vid_len if input_vid_len is None else int(input_vid_len)   # worker_v2.py:286
        self.vid_stride = vid_stride
        self.rank, self.world_size, self.num_trials = rank, world_size, num_trials
        self.device = torch.device(device) if bank is None else bank.device
        self._epoch_start = None                                              # the streams at the start of an unfinished epoch

    def __len__(self):
        return len(self.td) // self.world_size // self.batch_size

    def state(self):
        """-> {'rng': ``train_data.rng_state()``}: as it was at the start of the epoch that is under way, else as it is now"""
        return {'rng': self.td.rng_state() if self._epoch_start is None else self._epoch_start}

    def load_state(self, state):
        if not isinstance(state, dict) or 'rng' not in state:
            raise ValueError("TrainLoader.load_state: a dict with the key 'rng', as state() returns it")
        self.td.set_rng_state(state['rng'])
        self._epoch_start = None
        return self

    def _host(self, e, ids):
        samples = [self.td.sample(e, i, self.num_trials) for i in ids]
        b = collate_host(samples, self.input_vid_len, self.td.max_text_len, self.vid_stride)
        b = {k: (v if k == 'text_size' else v.to(self.device)) for k, v in b.items()}
        return b, b.pop('targets')

    def _banked(self, e, ids):
        td, bank = self.td, self.bank
        vid, shallow, text, cls, targets, sizes = [], [], [], [], [], []
        for i in ids:
            vid_id, seg_idx, window, target = td.decide(e, i, self.num_trials)
            vw, sw = td.stream_windows(td.video_length(vid_id), window)      # the length was recorded when the bank was filled
            vid.append(bank.window('vid', vid_id, *vw, self.input_vid_len))
            shallow.append(bank.window('shallow', vid_id, *sw, self.input_vid_len))
            for j in seg_idx:
                t = td.videos[vid_id]['text_ids'][j]
                text.append(bank.window('text', t, 0, bank.rows['text'][t][1], td.max_text_len))
            cls += [bank.cls_row[s] for s in td.sentences(vid_id, seg_idx)]
            targets.append(torch.from_numpy(target) / self.vid_stride)
            sizes.append(len(seg_idx))
        bs, nq = len(ids), len(cls)
        tg = torch.cat(targets).contiguous().numpy().view(np.int64).reshape(-1)          # (B', 2) float32 = B' words
        table = np.concatenate([np.asarray(vid, dtype=np.int64).reshape(-1), np.asarray(shallow, dtype=np.int64).reshape(-1),
                                np.asarray(text, dtype=np.int64).reshape(-1), np.asarray(cls, dtype=np.int64), tg])
        dev = torch.from_numpy(table).to(bank.device, non_blocking=True)                  # the step's one upload
        cut = np.cumsum([0, 2 * bs, 2 * bs, 2 * nq, nq, nq])
        part = [dev[cut[k]:cut[k + 1]] for k in range(5)]
        v, vid_masks = bank.assemble('vid', part[0].view(bs, 2), self.input_vid_len)
        s, _ = bank.assemble('shallow', part[1].view(bs, 2), self.input_vid_len, want_mask=False)
        tokens, token_masks = bank.assemble('text', part[2].view(nq, 2), td.max_text_len)
        batch = dict(vid=v, shallow=s, vid_masks=vid_masks, tokens=tokens, text_cls=bank.cls.index_select(0, part[3]),
                     token_masks=token_masks[:, None], text_size=torch.as_tensor(sizes))
        return batch, part[4].view(torch.float32).view(nq, 2)

    def epoch(self, e):
        make = self._host if self.bank is None else self._banked
        order = self.td.order(e, self.rank, self.world_size)
        self._epoch_start = self.td.rng_state()
        for k in range(len(self)):
            ids = order[k * self.batch_size:(k + 1) * self.batch_size]
            if self.microbatch_size is None:
                yield make(e, ids)
            else:
                parts = [make(e, ids[i:i + self._mb]) for i in range(0, self.batch_size, self._mb)]
                yield [p[0] for p in parts], [p[1] for p in parts]
        self._epoch_start = None
