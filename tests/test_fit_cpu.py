"""CPU checks that go with the multi-rank fit (include/decafnet_hip_fit.h, csrc/fit.hip, ``train.fit_parallel``).

1. The declared boundary of the ``_lib.FIT`` record: the table equals the header (tests/abi_headers.check_table), the built library
   exports the declared symbols and the version is 1, the source is part of the build with its flag, no name is shared with another
   table, ``EXTENSIONS`` / ``PENDING`` / ``STAGED`` are what they were, and hipcc compiles the source without a warning.
2. ``VideoCentricEvalData.targets`` against a numpy restatement of the two formulas (dataset.py:706-712, worker_v2.py:1037) on a
   generated tree, and ``sample()`` keeps its keys.
3. The restatement of tests/eval_loss_ref.py: its per-query and per-video stages against ``evaluator.calc_loss`` on the same per-row
   array (the objective replaced by the array: nothing is launched), its final pass against a plain sum where the order cannot matter.
4. The refusals of ``fit_parallel`` and of ``EvalBank.subset`` on stub objects: nothing is launched, nothing is written."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import abi_headers as H
import eval_loss_ref as R
import train_data_tree as TT
from conftest import load_pkg


# ---------------------------------------------------------------------------------------------- 1. the boundary
def test_fit_record_equals_its_header_and_the_library():
    pkg = load_pkg()
    L = pkg._lib
    assert len(L.FIT) == 1
    ext = L.FIT[0]
    assert ext == L.Extension('fit', 'decafnet_hip_fit.h', 'dcf_fit_ext_version', 1, 'DCF_FIT_EXT_VERSION',
                              ('decafnet_hip.h', 'decafnet_hip_guard.h'), L.FIT_TABLE)
    H.check_table(ext)
    assert sorted(ext.table) == ['dcf_fit_ext_version', 'dcf_guard_word_merge', 'dcf_guard_word_publish', 'dcf_op_loss_table_mean']
    assert 'fit.hip' in pkg.build.SOURCES and '-ffp-contract=off' in pkg.build.EXTRA['fit.hip']
    h = ctypes.CDLL(pkg.build.build())
    for s in H.declared_symbols(ext.header):
        assert hasattr(h, s), f'{s} declared in include/{ext.header} but not exported'
    assert h.dcf_fit_ext_version() == 1
    m = [line for line in H.source_of(ext.header).splitlines() if 'DCF_GUARD_REMOTE' in line]
    assert m and int(m[0].split()[-1], 0) == L.GUARD_REMOTE and L.GUARD_REMOTE & 1 == 0, 'the conv-gradient operators raise bit 0'


def test_source_compiles_without_warnings_under_the_project_flags(tmp_path):
    b = load_pkg().build
    cmd = [b.hipcc()] + b.FLAGS + b.EXTRA['fit.hip'] + ['-c', os.path.join(b.CSRC, 'fit.hip'), '-o', str(tmp_path / 'fit.o')]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0 and 'warning' not in r.stderr and 'warning' not in r.stdout, r.stderr


def test_the_other_records_are_unchanged_and_share_no_name():
    L = load_pkg()._lib
    assert [e.key for e in L.EXTENSIONS] == ['base', 'train', 'dist', 'attn', 'front', 'guard', 'clock', 'half', 'front_half', 'embd']
    assert [e.key for e in L.PENDING] == ['batch'] and [e.key for e in L.STAGED] == ['eval']
    assert not [n for n in dir(L) if n.endswith('SIGNATURES') and getattr(L, n) is L.FIT_TABLE]
    others = L.EXTENSIONS + L.PENDING + L.STAGED
    assert not {name for e in others for name in e.table} & set(L.FIT_TABLE)
    assert L.FIT[0].key not in {e.key for e in others} and L.FIT[0].header not in {e.header for e in others}
    for e in others:
        assert not set(H.declared_symbols(e.header)) & set(L.FIT_TABLE), e.header


# ---------------------------------------------------------------------------------------------- 2. the targets
@pytest.fixture(scope='module')
def eval_data(tmp_path_factory):
    pkg = load_pkg()
    root = str(tmp_path_factory.mktemp('tree'))
    arrays, data = TT.random_tree(11, 6, 8, 6, 40, 5, fps=29.97)
    TT.write_tree(root, arrays)
    cfg = dict(TT.cfg_of(root, dict(data, crop_ratio=None)), eval_split=('train',))
    return pkg.data.VideoCentricEvalData(cfg)


@pytest.mark.parametrize('vid_stride', [1, 2, 3])
def test_targets_are_the_two_formulas(eval_data, vid_stride):
    ed = eval_data
    assert len(ed.videos) == 6
    for vid_id, v in ed.videos.items():
        seg = np.asarray(v['segments'], dtype=np.float64)
        grid = (np.clip(seg * v['fps'], 0, v['num_frames']) / ed.clip_stride - 0.5 * ed.clip_size / ed.clip_stride).astype(np.float32)
        want = grid / np.float32(vid_stride)
        got = ed.targets(vid_id, vid_stride)
        assert got.dtype == torch.float32 and got.shape == (len(seg), 2) and want.dtype == np.float32
        assert np.array_equal(got.numpy().view(np.int32), want.view(np.int32)), vid_id
    assert torch.equal(ed.targets(vid_id), ed.targets(vid_id, 1))
    assert set(ed.sample(vid_id)) == {'fps', 'num_frames', 'duration', 'segment', 'clip_size', 'clip_stride', 'clip_id', 'text_id', 'vid',
                                      'shallow_vid', 'text', 'text_cls', 'ext_scores'}


# ---------------------------------------------------------------------------------------------- 3. the restatement
def calc_loss_on(pkg, monkeypatch, rows):
    """``evaluator.calc_loss`` with the objective replaced by ``rows``: its clamp, its two divisions and its NaN filter, on the CPU"""
    E = pkg.evaluator
    monkeypatch.setattr(E._loss, 'pt_gen_params', lambda opt, pt_gen=None: ((1.0, 0.5, 8), False))
    monkeypatch.setattr(E._loss, '_objective', lambda *a: (torch.from_numpy(rows), None))
    return E.calc_loss(((), (), ()), None, {'train': {'center_sampling_radius': 1.5}})


@pytest.mark.parametrize('seed', range(6))
def test_per_video_stage_is_calc_loss(monkeypatch, seed):
    pkg = load_pkg()
    for n in (1, 2, 5, 7):                                                       # below 8 values numpy adds in order
        rows, offsets = R.table([n], seed, special=True)
        if n > 1:
            rows[1:, :][np.random.default_rng(seed).random(n - 1) < 0.3, 1] = np.nan
        with np.errstate(all='ignore'):
            stats, per_row = calc_loss_on(pkg, monkeypatch, rows)
        values = R.per_query(rows)
        assert np.array_equal(values, per_row.astype(np.float64), equal_nan=True), 'the fp32 divisions'
        pv = R.per_video(values, offsets)
        want = np.array([stats['cls_loss'], stats['reg_loss']])
        assert np.array_equal(np.isnan(pv[0]), np.isnan(want)) and np.array_equal(pv[0][~np.isnan(want)], want[~np.isnan(want)]), (n, pv, want)


def test_a_video_of_nan_rows_or_of_no_row_is_nan_and_poisons_the_mean():
    rows, offsets = R.table([2, 3, 1], 4, special=False)
    rows[0:2, 1] = np.nan
    pv, out = R.loss_table_mean(rows, np.array([0, 2, 5, 5, 6]))
    assert np.isnan(pv[0, 0]) and not np.isnan(pv[0, 1]) and np.isnan(pv[2]).all() and np.isnan(out).all()
    assert R.bits(pv[2])[0] == 0x7ff8000000000000


@pytest.mark.parametrize('V', [1, 3, 256, 257, 600])
def test_final_pass_on_exact_values(V):
    """integers add exactly in any order: the lane-strided tree equals the plain sum"""
    g = np.random.default_rng(V)
    pv = g.integers(0, 1000, (V, 2)).astype(np.float64)
    assert np.array_equal(R.over_videos(pv), pv.sum(0) / V)
    pv[V // 2, 0] = np.inf
    assert R.over_videos(pv)[0] == np.inf and np.isfinite(R.over_videos(pv)[1])


# ---------------------------------------------------------------------------------------------- 4. the refusals
class _Loader:
    def __init__(self, rank, world_size):
        self.rank, self.world_size = rank, world_size


def _stub(T, world=2, **attrs):
    ts = object.__new__(T.DataParallelTrainStep)
    ts.group, ts.world, ts.skip_nonfinite, ts.agree_skips = object(), world, False, False
    for k, v in attrs.items():
        setattr(ts, k, v)
    return ts


def test_fit_parallel_refuses_before_anything_is_launched(monkeypatch, tmp_path):
    T = load_pkg().train
    import torch.distributed as dist
    monkeypatch.setattr(dist, 'get_rank', lambda group=None: 1)
    root = str(tmp_path)
    with pytest.raises(ValueError, match='rank 0 of 2'):
        T.fit_parallel(_stub(T), _Loader(0, 2), root)
    with pytest.raises(ValueError, match='rank 1 of 1'):
        T.fit_parallel(_stub(T), _Loader(1, 1), root)
    with pytest.raises(ValueError, match='agree_skips'):
        T.fit_parallel(_stub(T, skip_nonfinite=True), _Loader(1, 2), root)
    with pytest.raises(ValueError, match='eval_data'):
        T.fit_parallel(_stub(T), _Loader(1, 2), root, eval_run=1)
    with pytest.raises(ValueError, match='eval_data'):
        T.fit_parallel(_stub(T, skip_nonfinite=True, agree_skips=True), _Loader(1, 2), root, eval_run=2, eval_by='itr')
    with pytest.raises(ValueError, match='eval_by'):
        T.fit_parallel(_stub(T), _Loader(1, 2), root, eval_by='step')
    with pytest.raises(ValueError, match='EvalBank'):                            # a sharded evaluation needs the bank
        T.fit_parallel(_stub(T), _Loader(1, 2), root, eval_run=1, eval_data=[{}])
    one = object.__new__(T.TrainStep)                                            # one rank: the same argument checks
    with pytest.raises(ValueError, match='eval_data'):
        T.fit_parallel(one, None, root, eval_run=1)
    with pytest.raises(ValueError, match='EvalBank'):
        T.fit_parallel(one, None, root, eval_run=1, eval_data=[{}], val_loss=True)
    assert not os.listdir(root)
    with pytest.raises(NotImplementedError, match='fit_parallel'):               # fit still refuses, and names the new entry point
        T.fit(_stub(T), None, root)
    with pytest.raises(ValueError, match='agree_skips'):
        T.DataParallelTrainStep(None, None, agree_skips=1)


def test_eval_bank_subset_on_a_stub_bank():
    data = load_pkg().data
    bank = object.__new__(data.EvalBank)
    bank.index = {f'v{i}': i for i in range(5)}
    bank.item = lambda vid_id: {'clip_id': vid_id, 'bank': bank}
    sub = bank.subset([3, 0, 4])
    assert isinstance(sub, data.EvalBankSubset) and len(sub) == 3 and sub.indices == (3, 0, 4) and sub.bank is bank
    assert [d['clip_id'] for d in sub] == ['v3', 'v0', 'v4'] == [d['clip_id'] for d in sub], 'an iterable, not an iterator'
    assert iter(sub) is not sub and all(set(d) == {'clip_id', 'bank'} for d in sub), 'no key is added to the item'
    assert len(bank.subset([])) == 0 and list(bank.subset([])) == []
    for bad in ([5], [-1], [1, 1], [0.5]):
        with pytest.raises(ValueError, match='subset'):
            bank.subset(bad)
