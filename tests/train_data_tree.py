"""The synthetic training tree of tests/golden/train_data.npz on disk, for tests/golden/make_golden_train_data.py (which runs the
reference on it), tests/test_train_data.py and tests/test_gpu_batch_assemble.py; and a generated tree at a model's widths for the
end-to-end step of the latter.

A tree: featA/<vid>.npy and featB/<vid>.npy (two sources of the ``vid`` stream at the raw clip rate, featB may be a clip shorter),
shallow/<vid>.npy (at the down-sampled rate), text/<text_id>.npy (L, C_t), anno.json ({'train': {...}} with num_clips) and
cls_train.npy (the pickled sentence -> (1, D) table)."""
import json
import os

import numpy as np


def js(z, key):
    return json.loads(bytes(z[key]).decode())


def blob(obj):
    return np.frombuffer(json.dumps(obj).encode(), dtype=np.uint8)


def write_tree(root, arrays, half=False):
    """materialise the ``tree/`` arrays under ``root``; ``half``: the clip features of all three directories as float16 files"""
    anno = js(arrays, 'tree/anno_json')
    for d in ('featA', 'featB', 'shallow', 'text'):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    for vid in anno['train']:
        for d in ('featA', 'featB', 'shallow'):
            a = np.array(arrays[f'tree/{vid}/{d}'])
            np.save(os.path.join(root, d, vid + '.npy'), a.astype(np.float16) if half else a)
    cls = {}
    for i, sent in enumerate(js(arrays, 'tree/sentences')):
        cls[sent] = np.array(arrays['tree/cls_rows'][i:i + 1])
    for v in anno['train'].values():
        for q in v['annotations']:
            np.save(os.path.join(root, 'text', q['sentence_id'] + '.npy'), np.array(arrays[f"tree/text/{q['sentence_id']}"]))
    with open(os.path.join(root, 'anno.json'), 'w') as fh:
        json.dump(anno, fh)
    np.save(os.path.join(root, 'cls_train.npy'), cls, allow_pickle=True)


def cfg_of(root, data):
    """the ``opt.data`` dict of a tree under ``root``; ``data``: the keys that do not name a path"""
    cfg = dict(data, anno_file=os.path.join(root, 'anno.json'), split=('train',),
               vid_feat_dir=[os.path.join(root, 'featA'), os.path.join(root, 'featB')], shallow_vid_feat_dir=[os.path.join(root, 'shallow')],
               text_feat_dir=os.path.join(root, 'text'), text_cls_fname=os.path.join(root, 'cls_{split}.npy'), vid_load='npy',
               shallow_vid_load='npy')
    if cfg.get('crop_ratio') is not None:
        cfg['crop_ratio'] = tuple(cfg['crop_ratio'])
    return cfg


def random_tree(seed, n_videos, D, C_t, max_vid_len, max_text_len, fps=30.0, clip_size=16, clip_stride=16):
    """-> (arrays, data): a generated tree at the widths of a model -- every video fits ``max_vid_len`` (lengths from a third of it
    up, one of them odd), one to three queries each with segments inside the video, featA / featB of D / 2 channels each,
    downsample_rate 1 -- and the ``data`` keys of ``cfg_of``.  This project's own data: the reference has no part in it."""
    g = np.random.default_rng(seed)
    arrays, anno, sentences = {}, {}, []
    for k in range(n_videos):
        vid = f'g{k}'
        T = int(g.integers(max(max_vid_len // 3, 2), max_vid_len + 1)) | (k == 0)
        T = min(T, max_vid_len)
        arrays[f'tree/{vid}/featA'] = g.standard_normal((T, D // 2)).astype(np.float32)
        arrays[f'tree/{vid}/featB'] = g.standard_normal((T, D - D // 2)).astype(np.float32)
        arrays[f'tree/{vid}/shallow'] = g.standard_normal((T, D)).astype(np.float32)
        dur = ((T - 1) * clip_stride + clip_size) / fps
        qs = []
        for q in range(1 + k % 3):
            a = float(g.uniform(0.1, 0.5) * dur)
            b = float(min(a + g.uniform(0.15, 0.4) * dur, dur))
            tid = f'{vid}_q{q}'
            sentences.append(f'query {q} of {vid}')
            qs.append({'segment': [a, b], 'sentence': sentences[-1], 'sentence_id': tid})
            arrays[f'tree/text/{tid}'] = g.standard_normal((int(g.integers(2, max_text_len + 3)), C_t)).astype(np.float32)
        anno[vid] = {'fps': fps, 'num_frames': int((T - 1) * clip_stride + clip_size), 'num_clips': T, 'annotations': qs}
    arrays['tree/anno_json'] = blob({'train': anno})
    arrays['tree/sentences'] = blob(sentences)
    arrays['tree/cls_rows'] = g.standard_normal((len(sentences), D)).astype(np.float32)
    data = dict(downsample_rate=1, clip_size=clip_size, clip_stride=clip_stride, max_vid_len=max_vid_len, max_text_len=max_text_len,
                crop_ratio=(0.7, 1.0), trunc_thresh=0.5, max_num_text=2, normalize_vid=False, normalize_text=False)
    return arrays, data
