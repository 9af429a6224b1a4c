"""Generate tests/golden/train_data.npz: a synthetic training tree pushed through the reference's OWN training dataset and collate
(``VideoCentricTwoFeatDataset`` with ``is_training=True``, libs/data/dataset.py; ``Trainer._batchify`` / ``_batchify_videos``,
libs/worker_v2.py), with the inert import stubs of make_golden.py.

Run where the reference is importable (not on the GPU machine):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_train_data.py

The dataset is the real class, constructed on the tree (its constructor reads nothing but the annotation file and the text-CLS
table); the Trainer, whose constructor builds a model, lends its three collate methods unbound to a bare namespace.

Two configurations over one tree (tests/train_data_tree.py writes it): 'crop' (crop_ratio (0.5, 1.0)) and 'nocrop' (crop_ratio
None, features normalised).  Recorded per configuration, under ``random.seed(SEED); np.random.seed(SEED)`` set before construction:
the dataset's ``data_list`` (_build_train_samples, all epochs), and the ``__getitem__`` results in the recorded index order ``visits``
(epoch, idx) -- window or None, target, vid, shallow_vid, text, text_cls --, then ``Trainer._batchify`` / ``_batchify_videos`` of the
items listed in ``batch/items``.  The tree drives every branch of the reference's decisions, asserted below: a video that fits
max_vid_len with the crop drawn shorter, one where the draw equals the video, a video longer than max_vid_len, crop_ratio None, a
segment longer than max_vid_len / trunc_thresh, a window with more than max_num_text queries, downsample_rate 2.
"""
import os
import random
import sys
import tempfile
from types import SimpleNamespace as NS

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402
import train_data_tree as TT  # noqa: E402

SEED = 11
EPOCHS = 2
FPS, CLIP_SIZE, CLIP_STRIDE, DS = 30.0, 16, 8, 2
UNIT = CLIP_STRIDE * DS / FPS                     # seconds per down-sampled clip
DATA = dict(downsample_rate=DS, clip_size=CLIP_SIZE, clip_stride=CLIP_STRIDE, max_vid_len=32, max_text_len=6, trunc_thresh=0.5,
            max_num_text=2, group_method='greedy')
CONFIGS = {'crop': dict(DATA, crop_ratio=(0.5, 1.0), normalize_vid=False, normalize_text=False),
           'nocrop': dict(DATA, crop_ratio=None, normalize_vid=True, normalize_text=True)}
VID_STRIDE = 2                                    # the Trainer's divisor of the targets in the recorded batch
# video -> (raw clips of featA, raw clips of featB, clips of shallow, segments in down-sampled clips)
VIDEOS = {
    'fit_many': (48, 47, 24, [(8.0, 10.5), (9.0, 12.0), (10.0, 11.5), (11.0, 14.0), (12.5, 15.0)]),
    'fit_short': (20, 20, 9, [(2.0, 5.0), (4.5, 7.5)]),
    'fit_three': (6, 6, 3, [(0.5, 2.0)]),
    'one_clip': (2, 2, 1, [(0.1, 0.8)]),
    'long': (160, 160, 80, [(30.0, 36.0), (33.0, 41.0), (60.0, 66.5), (5.0, 9.0)]),
    'long_seg': (200, 199, 100, [(4.0, 75.0), (80.0, 86.0)]),
}


def make_tree():
    g = np.random.default_rng(SEED)
    arrays, anno, sentences = {}, {}, []
    for vid, (la, lb, ls, segs) in VIDEOS.items():
        arrays[f'tree/{vid}/featA'] = g.standard_normal((la, 6)).astype(np.float32)
        arrays[f'tree/{vid}/featB'] = g.standard_normal((lb, 4)).astype(np.float32)
        arrays[f'tree/{vid}/shallow'] = g.standard_normal((ls, 10)).astype(np.float32)
        qs = []
        for k, (a, b) in enumerate(segs):
            tid = f'{vid}_{k}'
            sentences.append(f'sentence {k} of {vid} ' if k == 0 else f'sentence {k} of {vid}')
            qs.append({'segment': [a * UNIT, b * UNIT], 'sentence': sentences[-1], 'sentence_id': tid})
            arrays[f'tree/text/{tid}'] = g.standard_normal((3 + (len(sentences) * 5) % 7, 8)).astype(np.float32)
        anno[vid] = {'fps': FPS, 'num_frames': (la - 1) * CLIP_STRIDE + CLIP_SIZE, 'num_clips': la, 'annotations': qs}
    arrays['tree/anno_json'] = TT.blob({'train': anno})
    arrays['tree/sentences'] = TT.blob(sentences)
    arrays['tree/cls_rows'] = g.standard_normal((len(sentences), 10)).astype(np.float32)
    return arrays


def main():
    MG.install_stubs()
    from libs.data import dataset as D
    from libs.worker_v2 import Trainer
    out = make_tree()
    meta = dict(seed=SEED, epochs=EPOCHS, vid_stride=VID_STRIDE, configs=CONFIGS, input_vid_len=DATA['max_vid_len'])
    seen = set()
    with tempfile.TemporaryDirectory() as root:
        TT.write_tree(root, out)
        for name, data in CONFIGS.items():
            cfg = TT.cfg_of(root, data)
            random.seed(SEED)
            np.random.seed(SEED)
            opt = NS(data=NS(downsample_rate=DS, text_cls_fname=cfg['text_cls_fname'], vid_load='npy', shallow_vid_load='npy',
                             shallow_vid_feat_dir=cfg['shallow_vid_feat_dir']))
            ds = D.VideoCentricTwoFeatDataset(
                split=cfg['split'], is_training=True, anno_file=cfg['anno_file'], vid_feat_dir=cfg['vid_feat_dir'],
                text_feat_dir=cfg['text_feat_dir'], ext_score_dir=None, tokenizer=None, clip_size=CLIP_SIZE, clip_stride=CLIP_STRIDE,
                downsample_rate=DS, to_fixed_len=False, normalize_vid=data['normalize_vid'], normalize_text=data['normalize_text'],
                max_vid_len=data['max_vid_len'], max_text_len=data['max_text_len'], crop_ratio=data['crop_ratio'],
                trunc_thresh=data['trunc_thresh'], max_num_text=data['max_num_text'], group_method=data['group_method'],
                num_epochs=EPOCHS, opt=opt)
            assert ds.downsample_rate == 2
            seen.add('ds2')
            out[f'{name}/data_list'] = TT.blob([[v, [int(i) for i in idx]] for v, idx in ds.data_list])
            if any(len(idx) == data['max_num_text'] and len(ds.vid_dict[v]['segments']) > data['max_num_text'] for v, idx in ds.data_list):
                seen.add('choice')
            order = np.random.default_rng(SEED + len(name))
            visits, items = [], []
            for e in range(EPOCHS):
                ds.set_epoch(e)
                for idx in order.permutation(len(ds)).tolist():
                    vid_id, seg_idx = ds.data_list[e * len(ds) + idx]
                    item = ds[idx]
                    k = len(visits)
                    visits.append([e, idx])
                    items.append(item)
                    full = min(ds._load_vid_feats(vid_id).size(1), ds._load_shallow_vid_feats(vid_id).size(1))
                    # what the reference did with the shallow stream: the first vid_len clips, whatever the window
                    assert item['shallow_vid'].size(1) == full
                    window = None if item['vid'].size(1) == full else [int(w) for w in _window_of(ds, vid_id, item)]
                    out[f'{name}/item{k}/window'] = np.array(window if window is not None else [-1, -1], dtype=np.int64)
                    out[f'{name}/item{k}/target'] = item['target'].numpy()
                    out[f'{name}/item{k}/vid'] = item['vid'].numpy()
                    out[f'{name}/item{k}/shallow_vid'] = item['shallow_vid'].numpy()
                    out[f'{name}/item{k}/text_cls'] = item['text_cls'].numpy()
                    for j, t in enumerate(item['text']):
                        out[f'{name}/item{k}/text{j}'] = t.numpy()
                    assert item['clip_id'] == vid_id and tuple(item['text_id']) == tuple(seg_idx)
                    if data['crop_ratio'] is None and full <= data['max_vid_len']:
                        seen.add('crop_none')
                    elif full <= data['max_vid_len']:
                        seen.add('draw_equal' if window is None else 'draw_shorter')
                    else:
                        assert window is not None
                        seen.add('window_search')
                        segs = ds.vid_dict[vid_id]['segments'][list(seg_idx)]
                        if float((segs[:, 1] - segs[:, 0]).max()) / UNIT > data['max_vid_len'] / data['trunc_thresh']:
                            seen.add('thresh_0.2')
            out[f'{name}/visits'] = np.array(visits, dtype=np.int64)
            if name == 'crop':                                      # one batch through the Trainer's collate: items that fit the buffer
                T = DATA['max_vid_len']
                pick = [k for k, it in enumerate(items) if it['shallow_vid'].size(1) <= T]
                first = sorted(pick, key=lambda k: (-len(items[k]['text']), items[k]['vid'].size(1) == items[k]['shallow_vid'].size(1)))[:2]
                pick = list(dict.fromkeys(first + [k for k in pick if len(items[k]['text']) == 1][:2]))
                tr = NS(input_vid_len=T, max_text_len=DATA['max_text_len'])
                tr._batchify_videos = lambda vid_list: Trainer._batchify_videos(tr, vid_list)
                tr._batchify_text = lambda text_list: Trainer._batchify_text(tr, text_list)
                chosen = [items[k] for k in pick]
                vid, vid_masks, text, text_masks, text_size = Trainer._batchify(tr, [d['vid'] for d in chosen], [d['text'] for d in chosen])
                shallow, _ = Trainer._batchify_videos(tr, [d['shallow_vid'] for d in chosen])
                assert len(set(text_size.tolist())) > 1, 'the batch should pad the query dimension'
                out['batch/items'] = np.array(pick, dtype=np.int64)
                out['batch/vid'], out['batch/vid_masks'], out['batch/shallow'] = vid.numpy(), vid_masks.numpy(), shallow.numpy()
                out['batch/text'], out['batch/text_masks'], out['batch/text_size'] = text.numpy(), text_masks.numpy(), text_size.numpy()
                out['batch/text_cls'] = torch.concat([d['text_cls'] for d in chosen]).numpy()           # worker_v2.py:407-408
                out['batch/targets'] = torch.cat([d['target'] / VID_STRIDE for d in chosen]).numpy()    # worker_v2.py:417
    want = {'ds2', 'choice', 'crop_none', 'draw_equal', 'draw_shorter', 'window_search', 'thresh_0.2'}
    assert seen == want, f'branches not driven: {sorted(want - seen)}'
    out['meta'] = TT.blob(meta)
    path = os.path.join(HERE, 'train_data.npz')
    np.savez_compressed(path, **out)
    print(f'train_data.npz: {os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays, branches {sorted(seen)}')


def _window_of(ds, vid_id, item):
    """[ws, we] of a cropped item: the reference returns ``se`` from _truncate_vid_feats and drops it, so it is found again as the
    place of the item's clips in the video (the features are random: the place is unique)"""
    full = ds._load_vid_feats(vid_id)
    n = item['vid'].size(1)
    hits = [s for s in range(full.size(1) - n + 1) if torch.equal(full[:, s:s + n], item['vid'])]
    assert len(hits) == 1, hits
    return hits[0], hits[0] + n


if __name__ == '__main__':
    main()
