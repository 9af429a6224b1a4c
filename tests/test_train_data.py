"""CPU checks of the training data path (cvpr2025-decafnet_amd/data.py: VideoCentricTrainData, collate_host, FeatureBank, TrainLoader)
against tests/golden/train_data.npz, which tests/golden/make_golden_train_data.py recorded from the reference's own
``VideoCentricTwoFeatDataset`` and ``Trainer._batchify``: the groups of all epochs, and in the recorded visit order every window, every
target (compared as bits) and every per-sample tensor, exactly; the collated batch; the ``shallow_window`` departure; the refusals; the
shuffling rule; and the declared boundary of the batch-assembly extension (the ``_lib.PENDING`` record against its header, the source
in the build, the exports of the built library).  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import abi_headers as H
import train_data_tree as TT
from conftest import GOLDEN, load_pkg

Z = np.load(f'{GOLDEN}/train_data.npz')
META = TT.js(Z, 'meta')
CONFIGS = sorted(META['configs'])


@pytest.fixture(scope='module')
def data():
    return load_pkg().data


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('train_tree'))
    TT.write_tree(root, Z)
    return root


def make(data, tree, name, shallow_window, **over):
    return data.VideoCentricTrainData(TT.cfg_of(tree, dict(META['configs'][name], **over)), num_epochs=META['epochs'], seed=META['seed'],
                                      shallow_window=shallow_window)


_replays = {}


def replay(data, tree, name, shallow_window):
    """the samples of the recorded visits, in their order (the order is the RNG contract), made once"""
    key = (name, shallow_window)
    if key not in _replays:
        td = make(data, tree, name, shallow_window)
        _replays[key] = (td, [td.sample(e, i) for e, i in Z[f'{name}/visits'].tolist()])
    return _replays[key]


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize('name', CONFIGS)
def test_groups_of_all_epochs(data, tree, name):
    td = make(data, tree, name, 'reference')
    want = TT.js(Z, f'{name}/data_list')
    assert [[v, list(i)] for v, i in td.samples] == want
    assert len(td) == len(want) // META['epochs'] and len(td.samples) == len(td) * META['epochs']


@pytest.mark.parametrize('name', CONFIGS)
def test_windows_targets_and_tensors_in_the_recorded_order(data, tree, name):
    td, samples = replay(data, tree, name, 'reference')
    windows = 0
    for k, s in enumerate(samples):
        p = f'{name}/item{k}/'
        assert (s['window'] if s['window'] is not None else [-1, -1]) == Z[p + 'window'].tolist(), k
        got = s['target'].numpy()
        assert got.dtype == np.float32 and got.shape == Z[p + 'target'].shape and np.array_equal(bits(got), bits(Z[p + 'target'])), k
        for key in ('vid', 'shallow_vid', 'text_cls'):
            assert s[key].numpy().dtype == Z[p + key].dtype and np.array_equal(s[key].numpy(), Z[p + key]), (k, key)
        assert len(s['text']) == len(s['text_id']) == sum(f.startswith(p + 'text') and f != p + 'text_cls' for f in Z.files)
        for j, t in enumerate(s['text']):
            assert np.array_equal(t.numpy(), Z[p + f'text{j}']), (k, j)
            assert t.size(1) <= td.max_text_len
        windows += s['window'] is not None
    assert 0 < windows < len(samples)


def test_decide_makes_the_decisions_of_sample(data, tree):
    td = make(data, tree, 'crop', 'same')
    _, samples = replay(data, tree, 'crop', 'same')
    for (e, i), s in zip(Z['crop/visits'].tolist(), samples):
        vid_id, seg_idx, window, target = td.decide(e, i)
        assert (vid_id, seg_idx, window) == (s['clip_id'], s['text_id'], s['window'])
        assert isinstance(target, np.ndarray) and np.array_equal(bits(target), bits(s['target'].numpy()))


def test_collate_host_is_the_trainers_batch(data, tree):
    _, samples = replay(data, tree, 'crop', 'reference')
    chosen = [samples[k] for k in Z['batch/items'].tolist()]
    b = data.collate_host(chosen, META['input_vid_len'], META['configs']['crop']['max_text_len'], vid_stride=META['vid_stride'])
    eq = lambda key, want: b[key].dtype == want.dtype and torch.equal(b[key], want)
    t = lambda key: torch.from_numpy(np.array(Z[key]))
    assert eq('vid', t('batch/vid')) and eq('vid_masks', t('batch/vid_masks')) and eq('shallow', t('batch/shallow'))
    sizes = Z['batch/text_size'].tolist()
    assert b['text_size'].tolist() == sizes and b['text_size'].dtype == torch.int64
    flat = torch.cat([t('batch/text')[i, :n] for i, n in enumerate(sizes)])               # (bs, n_max, C, L) flattened by text_size
    flat_masks = torch.cat([t('batch/text_masks')[i, :n] for i, n in enumerate(sizes)])
    assert eq('tokens', flat) and eq('token_masks', flat_masks[:, None])
    assert eq('text_cls', t('batch/text_cls'))
    assert np.array_equal(bits(b['targets'].numpy()), bits(Z['batch/targets']))
    assert set(b) == {'vid', 'shallow', 'vid_masks', 'tokens', 'text_cls', 'token_masks', 'text_size', 'targets'}


@pytest.mark.parametrize('name', CONFIGS)
def test_same_differs_in_the_shallow_stream_alone(data, tree, name):
    td, ref = replay(data, tree, name, 'reference')
    _, same = replay(data, tree, name, 'same')
    cropped = 0
    for r, s in zip(ref, same):
        assert r['window'] == s['window'] and r['clip_id'] == s['clip_id']
        for key in ('vid', 'target', 'text_cls'):
            assert torch.equal(r[key], s[key])
        assert all(torch.equal(a, b) for a, b in zip(r['text'], s['text']))
        if s['window'] is None:
            assert torch.equal(r['shallow_vid'], s['shallow_vid'])
        else:
            ws, we = s['window']
            assert torch.equal(s['shallow_vid'], r['shallow_vid'][:, ws:we]) and s['shallow_vid'].size(1) == s['vid'].size(1)
            cropped += 1
    assert cropped


def test_reference_mode_refuses_a_shallow_stream_that_does_not_fit(data, tree):
    _, ref = replay(data, tree, 'crop', 'reference')
    _, same = replay(data, tree, 'crop', 'same')
    T, L = META['input_vid_len'], META['configs']['crop']['max_text_len']
    k = next(k for k, s in enumerate(ref) if s['shallow_vid'].size(1) > T)
    with pytest.raises(ValueError, match='shallow_vid.*do not fit'):
        data.collate_host([ref[k]], T, L)
    b = data.collate_host([same[k]], T, L)
    assert b['shallow'].shape == b['vid'].shape and bool(b['vid_masks'].all())


def _impossible(tmp_path, data):
    """one video of 30 clips that fits, cropped to 6 clips, with a segment of 20: no window holds half of it"""
    unit = 16 / 30.0
    g = np.random.default_rng(3)
    arrays = {'tree/imp/featA': g.standard_normal((30, 3)).astype(np.float32), 'tree/imp/featB': g.standard_normal((30, 3)).astype(np.float32),
              'tree/imp/shallow': g.standard_normal((30, 6)).astype(np.float32), 'tree/text/imp_0': g.standard_normal((4, 5)).astype(np.float32),
              'tree/sentences': TT.blob(['a long event']), 'tree/cls_rows': g.standard_normal((1, 6)).astype(np.float32),
              'tree/anno_json': TT.blob({'train': {'imp': {'fps': 30.0, 'num_frames': 480, 'num_clips': 30, 'annotations': [
                  {'segment': [2 * unit, 22 * unit], 'sentence': 'a long event', 'sentence_id': 'imp_0'}]}}})}
    TT.write_tree(str(tmp_path), arrays)
    cfg = TT.cfg_of(str(tmp_path), dict(downsample_rate=1, clip_size=16, clip_stride=16, max_vid_len=32, max_text_len=6, crop_ratio=(0.2, 0.2),
                                        trunc_thresh=0.5, max_num_text=2))
    return cfg


def test_no_valid_truncation(tmp_path, data):
    td = data.VideoCentricTrainData(_impossible(tmp_path, data), 1, 0)
    assert len(td) == 1
    with pytest.raises(ValueError, match='no valid truncation found'):
        td.decide(0, 0, num_trials=20)
    with pytest.raises(ValueError, match='no valid truncation found'):
        td.sample(0, 0, num_trials=3)


def test_refusals(tmp_path, data):
    cfg = _impossible(tmp_path, data)
    missing = dict(cfg, anno_file='/nonexistent/anno.json')                   # refused before anything is read
    with pytest.raises(NotImplementedError, match='to_fixed_len'):
        data.VideoCentricTrainData(dict(missing, to_fixed_len=True), 1, 0)
    with pytest.raises(NotImplementedError, match='tokenizer'):
        data.VideoCentricTrainData(dict(missing, tokenizer=object()), 1, 0)
    with pytest.raises(ValueError, match='shallow_window'):
        data.VideoCentricTrainData(cfg, 1, 0, shallow_window='none')
    with pytest.raises(ValueError, match='crop_ratio'):
        data.VideoCentricTrainData(dict(cfg, crop_ratio=0.9), 1, 0)
    for method in ('greedy', 'random', 'all'):                                # accepted, without effect on this path
        assert data.VideoCentricTrainData(dict(cfg, group_method=method), 1, 0).samples == (('imp', (0,)),)
    td = data.VideoCentricTrainData(cfg, 1, 0)
    with pytest.raises(IndexError):
        td.decide(1, 0)
    with pytest.raises(ValueError, match='another VideoCentricTrainData'):
        data.TrainLoader(data.VideoCentricTrainData(cfg, 1, 0), data.FeatureBank(td, device='cpu'), 1)


def test_shuffling_rule(data, tree):
    td = make(data, tree, 'crop', 'same')
    n = len(td)
    for epoch in range(3):
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(META['seed'] + epoch)).tolist()
        assert td.order(epoch) == perm and sorted(perm) == list(range(n))
        for w in (2, 5):
            shares = [td.order(epoch, r, w) for r in range(w)]
            assert all(s == perm[r::w][:n // w] for r, s in enumerate(shares))
            assert all(len(s) == n // w for s in shares) and len({i for s in shares for i in s}) == w * (n // w)
    assert td.order(0) != td.order(1)
    loader = data.TrainLoader(td, None, 5, rank=1, world_size=2, device='cpu')
    assert len(loader) == n // 2 // 5 == 1
    with pytest.raises(ValueError, match='rank'):
        td.order(0, 2, 2)


@pytest.mark.parametrize('microbatch', [None, 2])
def test_host_loader_yields_the_collated_order(data, tree, microbatch):
    """bank=None on the CPU: batches of the epoch's order, the tail dropped; micro-batches sliced as forward_backward slices them"""
    td, twin = make(data, tree, 'crop', 'same'), make(data, tree, 'crop', 'same')
    loader = data.TrainLoader(td, None, 4, microbatch_size=microbatch, device='cpu', vid_stride=2)
    order = twin.order(1)
    got = list(loader.epoch(1))
    assert len(got) == len(loader) == len(td) // 4
    for k, (batch, targets) in enumerate(got):
        ids = order[4 * k:4 * k + 4]
        groups = [ids] if microbatch is None else [ids[0:2], ids[2:4]]
        batches, tgs = ([batch], [targets]) if microbatch is None else (batch, targets)
        assert len(batches) == len(groups)
        for b, tg, grp in zip(batches, tgs, groups):
            want = data.collate_host([twin.sample(1, i) for i in grp], td.max_vid_len, td.max_text_len, vid_stride=2)
            assert 'targets' not in b and torch.equal(tg, want.pop('targets'))
            assert set(b) == set(want) and all(torch.equal(b[key], want[key]) for key in want)


def test_bank_layout_on_the_host(data, tree):
    """the bank's tables without a GPU: rows as the files store them, back to back; the CLS table; nbytes and max_bytes"""
    td = make(data, tree, 'nocrop', 'same')
    bank = data.FeatureBank(td, device='cpu')
    twin = make(data, tree, 'nocrop', 'same')
    for vid_id, v in twin.videos.items():
        vid, shallow = twin.video_streams(vid_id)
        for stream, cm in (('vid', vid), ('shallow', shallow)):
            r0, n = bank.rows[stream][vid_id]
            assert n == cm.size(1) and torch.equal(bank.data[stream][r0:r0 + n], cm.t())
        for t in v['text_ids']:
            r0, n = bank.rows['text'][t]
            assert torch.equal(bank.data['text'][r0:r0 + n], twin.token_features(t).t()) and n <= td.max_text_len
        rows = [bank.cls_row[s] for s in twin.sentences(vid_id, range(len(v['text_ids'])))]
        assert torch.equal(bank.cls[rows], twin.cls.lookup(twin.sentences(vid_id, range(len(v['text_ids'])))))
        assert td.video_length(vid_id) == twin.video_length(vid_id)
    for stream in bank.STREAMS:
        assert bank.data[stream].is_contiguous() and bank.row_offsets[stream].dtype == np.int64
        assert bank.row_offsets[stream].tolist() == [r0 for r0, _ in bank.rows[stream].values()]
        assert sum(n for _, n in bank.rows[stream].values()) == bank.data[stream].size(0)
    held = sum(t.numel() * t.element_size() for t in list(bank.data.values()) + [bank.cls])
    assert bank.nbytes == held
    with pytest.raises(ValueError, match=str(held)):
        data.FeatureBank(make(data, tree, 'nocrop', 'same'), device='cpu', max_bytes=held - 1)
    assert data.FeatureBank(make(data, tree, 'nocrop', 'same'), device='cpu', max_bytes=held).nbytes == held
    with pytest.raises(ValueError, match='holds'):
        bank.window('vid', 'long', 70, 90, 32)
    with pytest.raises(ValueError, match='do not fit'):
        bank.window('shallow', 'long', 0, 80, 32)
    assert bank.window('vid', 'long', 70, 80, 32) == ((bank.rows['vid']['long'][0] + 70) * 10, 10)
    with pytest.raises(RuntimeError, match='MI355X'):
        bank.assemble('vid', torch.zeros(1, 2, dtype=torch.int64), 32)


def test_bank_refuses_a_half_and_fp32_pair(tmp_path, data):
    root = str(tmp_path)
    TT.write_tree(root, Z)
    for vid in TT.js(Z, 'tree/anno_json')['train']:                            # the shallow files alone as float16
        np.save(f'{root}/shallow/{vid}.npy', np.array(Z[f'tree/{vid}/shallow']).astype(np.float16))
    td = data.VideoCentricTrainData(TT.cfg_of(root, dict(META['configs']['crop'], feature_dtype='stored')), 1, 0)
    with pytest.raises(ValueError, match='come as a pair'):
        data.FeatureBank(td, device='cpu')


# ---------------------------------------------------------------------------------------------- the declared boundary
def pending():
    L = load_pkg()._lib
    assert len(L.PENDING) == 1
    return L.PENDING[0]


def test_pending_record_equals_its_header():
    ext, L = pending(), load_pkg()._lib
    assert ext == L.Extension('batch', 'decafnet_hip_batch.h', 'dcf_batch_ext_version', 1, 'DCF_BATCH_EXT_VERSION', ('decafnet_hip.h',),
                              L.BATCH_TABLE)
    H.check_table(ext)
    assert H.param_names(ext.header, 'dcf_op_assemble_rows') == ['bank', 'elem_bytes', 'desc', 'B', 'C', 'T_out', 'out', 'mask', 'stream']
    assert ext.key not in {e.key for e in L.EXTENSIONS} and not any(e.table is ext.table for e in L.EXTENSIONS)
    taken = {n for e in L.EXTENSIONS for n in e.table}
    assert not taken & set(ext.table)
    assert not [n for n in dir(L) if n.endswith('SIGNATURES') and getattr(L, n) is ext.table]


def test_source_is_in_the_build():
    assert 'batch.hip' in load_pkg().build.SOURCES


def test_symbols_are_exported_and_version():
    ext = pending()
    h = ctypes.CDLL(load_pkg().build.build())
    syms = H.declared_symbols(ext.header)
    assert syms == sorted(ext.table)
    for s in syms:
        assert hasattr(h, s), f'{s} declared in include/{ext.header} but not exported'
    assert getattr(h, ext.version_symbol)() == ext.version
