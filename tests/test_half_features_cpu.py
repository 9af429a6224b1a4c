"""CPU checks that go with the half-feature extension (include/decafnet_hip_half.h; its header and table: tests/test_abi_headers.py): the
names of ``_lib.HALF_SIGNATURES``, its host arrays and half operands; the feature loaders' ``dtype``; what is
refused before a GPU is touched; and, on the emulation of tests/f16x3_ref.py, the property the half A operand of the split tile GEMM
rests on: for a binary16-representable operand the ``mid`` plane is exactly zero, so the product without the a_mid . w_hi term equals
the full one -- and for an operand that is not representable it does not.  No GPU."""
import ctypes
import pickle

import numpy as np
import pytest
import torch

import abi_headers as H
from conftest import load_pkg
import f16x3_ref as F

NAMES = ['dcf_forward_eval_h', 'dcf_forward_eval_videos_h', 'dcf_half_ext_version', 'dcf_op_linear_cm_split_h', 'dcf_op_linear_cm_split_ld_h',
         'dcf_op_sidekick_h']


def params_of(name):
    return H.params_of('decafnet_hip_half.h', name)[0]


# ---------------------------------------------------------------------------------------------- the ABI
def test_half_table_names_host_arrays_and_half_operands():
    pkg = load_pkg()
    table = pkg._lib.HALF_SIGNATURES
    assert sorted(table) == NAMES and 'half.hip' in pkg.build.SOURCES
    for name, (_, args) in table.items():             # which pointers are HOST arrays and which device addresses
        for p, a in zip(params_of(name), args):
            if p.count('*') == 2 or 'int32_t*' in p.replace(' ', ''):
                assert a in (ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int32)), (name, p, a)
            elif '*' in p:
                assert a is ctypes.c_void_p, (name, p, a)
    # the half operands are the bits of binary16, and nothing else of the forwards changed type
    for name, base in (('dcf_forward_eval_h', 'dcf_forward_eval'), ('dcf_forward_eval_videos_h', 'dcf_forward_eval_videos'),
                       ('dcf_op_sidekick_h', 'dcf_op_sidekick')):
        assert table[name] == pkg._lib.SIGNATURES[base], name
        halves = [p.split()[-1].lstrip('*') for p in params_of(name) if 'uint16_t' in p]
        assert halves == (['shallow'] if 'sidekick' in name else ['vid', 'shallow_vid']), (name, halves)
    order = [p.split()[-1].lstrip('*') for p in params_of('dcf_op_linear_cm_split_h')]
    assert order == ['A_cm', 'W', 'bias', 'C', 'M', 'N', 'K', 'nterms', 'unscaled', 'stream']
    assert params_of('dcf_op_linear_cm_split_h')[0].startswith('const uint16_t')
    order = [p.split()[-1].lstrip('*') for p in params_of('dcf_op_linear_cm_split_ld_h')]
    assert order == ['A_cm', 'lda', 'W', 'bias', 'C', 'M', 'N', 'K', 'nterms', 'unscaled', 'stream']
    assert params_of('dcf_op_linear_cm_split_ld_h')[0].startswith('const uint16_t') and params_of('dcf_op_linear_cm_split_ld_h')[1] == 'int64_t lda'


# ---------------------------------------------------------------------------------------------- the loaders
def _tree(tmp_path, np_dtype):
    """one video 'v' of (T, C) = (9, 6) in every format the loaders read; -> the (T, C) array"""
    g = np.random.default_rng(5)
    a = g.standard_normal((9, 6)).astype(np_dtype)
    b = g.standard_normal((9, 6)).astype(np_dtype)
    np.save(tmp_path / 'v.npy', a)
    torch.save(torch.from_numpy(a.copy()), tmp_path / 'v.pt')
    with open(tmp_path / 'v.pk', 'wb') as fh:
        pickle.dump([a, b], fh)
    return a, b


@pytest.mark.parametrize('fmt', ['npy', 'pt', 'pk0', 'pk1'])
def test_a_float16_tree_stays_float16_when_asked(tmp_path, fmt):
    pkg = load_pkg()
    a, b = _tree(tmp_path, np.float16)
    want = b if fmt == 'pk1' else a
    path = str(tmp_path / 'v')
    stored = pkg.data.load_clip_features(path, fmt, dtype='stored')
    assert stored.dtype == np.float16 and stored.tobytes() == want.tobytes()
    dflt = pkg.data.load_clip_features(path, fmt)
    assert dflt.dtype == np.float32 and np.array_equal(dflt, want.astype(np.float32))
    assert pkg.data.load_clip_features(path, fmt, dtype=np.float32).dtype == np.float32
    # the (C, T) tensors of the two public loaders
    for load in (lambda **kw: pkg.data.load_video_features([str(tmp_path)], 'v', fmt, **kw), lambda **kw: pkg.evaluator.load_features(path, fmt, **kw)):
        t = load(dtype='stored')
        assert t.dtype == torch.float16 and t.shape == (6, 9) and torch.equal(t, torch.from_numpy(want.T.copy()))
        t = load()
        assert t.dtype == torch.float32 and torch.equal(t, torch.from_numpy(want.T.astype(np.float32)))


@pytest.mark.parametrize('fmt', ['npy', 'pt', 'pk0', 'pk_avg'])
def test_float32_files_come_back_bit_identical(tmp_path, fmt):
    """default, 'stored' and np.float32 all return what the loader returned before it took a dtype; np.float16 is a cast"""
    pkg = load_pkg()
    a, b = _tree(tmp_path, np.float32)
    want = (a + b) / 2 if fmt == 'pk_avg' else a
    path = str(tmp_path / 'v')
    for kw in ({}, dict(dtype='stored'), dict(dtype=np.float32), dict(dtype='float32')):
        got = pkg.data.load_clip_features(path, fmt, **kw)
        assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), kw
        t = pkg.evaluator.load_features(path, fmt, **kw)
        assert t.dtype == torch.float32 and t.numpy().tobytes() == np.ascontiguousarray(want.T).tobytes(), kw
    got = pkg.data.load_clip_features(path, fmt, dtype=np.float16)
    assert got.dtype == np.float16 and got.tobytes() == want.astype(np.float16).tobytes()
    two = pkg.data.load_video_features([str(tmp_path), str(tmp_path)], 'v', fmt, downsample_rate=2, dtype=np.float16)
    assert two.dtype == torch.float16 and two.shape == (12, 5)
    n = pkg.data.load_video_features([str(tmp_path)], 'v', fmt, normalize=True, dtype=np.float16)
    ref = torch.nn.functional.normalize(torch.from_numpy(want.astype(np.float16).T.copy()).float(), dim=0).half()
    assert n.dtype == torch.float16 and torch.equal(n, ref)


def test_the_dataset_key_feature_dtype(tmp_path):
    import json
    pkg = load_pkg()
    g = np.random.default_rng(6)
    for d in ('vid', 'shallow', 'text'):
        (tmp_path / d).mkdir()
    np.save(tmp_path / 'vid' / 'a.npy', g.standard_normal((7, 4)).astype(np.float16))
    np.save(tmp_path / 'shallow' / 'a.npy', g.standard_normal((7, 4)).astype(np.float32))
    np.save(tmp_path / 'text' / 'a_0000.npy', g.standard_normal((3, 5)).astype(np.float32))
    np.save(tmp_path / 'cls_val.npy', {'s': g.standard_normal((1, 4)).astype(np.float32)}, allow_pickle=True)
    anno = {'val': {'a': {'fps': 1.0, 'num_frames': 7, 'annotations': [{'segment': [1.0, 3.0], 'sentence': 's'}]}}}
    (tmp_path / 'anno.json').write_text(json.dumps(anno))
    cfg = dict(anno_file=str(tmp_path / 'anno.json'), eval_split='val', vid_feat_dir=[str(tmp_path / 'vid')],
               shallow_vid_feat_dir=[str(tmp_path / 'shallow')], text_feat_dir=str(tmp_path / 'text'),
               text_cls_fname=str(tmp_path / 'cls_{split}.npy'))
    s = pkg.data.VideoCentricEvalData(cfg).sample('a')
    assert s['vid'].dtype == s['shallow_vid'].dtype == torch.float32
    s = pkg.data.VideoCentricEvalData(dict(cfg, feature_dtype='stored')).sample('a')
    assert s['vid'].dtype == torch.float16 and s['shallow_vid'].dtype == torch.float32 and s['text'][0].dtype == torch.float32
    s = pkg.data.VideoCentricEvalData(dict(cfg, feature_dtype=np.float16)).sample('a')
    assert s['vid'].dtype == s['shallow_vid'].dtype == torch.float16 and s['text_cls'].dtype == torch.float32
    with pytest.raises(ValueError, match='feature dtype'):
        pkg.data.VideoCentricEvalData(dict(cfg, feature_dtype='bfloat16'))


# ---------------------------------------------------------------------------------------------- refused before the GPU
@pytest.mark.parametrize('bad', ['bfloat16', np.float64, 'int8', 16, torch.bfloat16])
def test_a_feature_dtype_that_is_not_offered_is_refused(tmp_path, bad):
    pkg = load_pkg()
    with pytest.raises(ValueError, match='feature dtype'):
        pkg.data.load_clip_features(str(tmp_path / 'nothing'), 'npy', dtype=bad)         # before the file is looked for
    with pytest.raises(ValueError, match='feature dtype'):
        pkg.evaluator.load_features(str(tmp_path / 'nothing'), 'npy', dtype=bad)
    with pytest.raises(ValueError, match='feature_dtype'):
        pkg.evaluator.GroundingEvaluator({}, None, feature_dtype=bad)                    # before opt or the model are read


def test_the_evaluator_takes_float16_by_its_names_and_none():
    pkg = load_pkg()
    opt = dict(model=dict(max_vid_len=64, num_fpn_levels=2, mha_win_size=0), eval=dict(pre_nms_topk=1, pre_nms_thresh=0.0, seg_len_thresh=0.0), nms={})
    assert pkg.evaluator.GroundingEvaluator(opt, None).feature_dtype is None
    for name in ('float16', torch.float16, np.float16):
        assert pkg.evaluator.GroundingEvaluator(opt, None, feature_dtype=name).feature_dtype is torch.float16
    to_half = pkg.evaluator.GroundingEvaluator._to_half
    x = torch.tensor([[1.0, -65504.0, 2.0 ** -24, float('inf')]])
    h = to_half(x, 'vid', 'v7')
    assert h.dtype == torch.float16 and torch.equal(h.float(), x), 'a stored inf stays, the largest finite half and a subnormal are exact'
    with pytest.raises(ValueError, match=r'video v7: 2 finite values of shallow_vid .*65504'):
        to_half(torch.tensor([1.0, 65520.0, -1e9]), 'shallow_vid', 'v7')
    assert to_half(h, 'vid', 'v7') is h


def _tiny_model(pkg):
    kw = dict(D=64, E=128, TE=32, text_in=32, n_levels=2, win=5, n_heads=4, sn=8, sratio=0.3, msf=True, norm=True, max_seq_len=64,
              text_layers=1, text_max_len=8)
    return pkg.modeling.create_model(pkg.config.make_opt(**kw)).eval()


@pytest.mark.parametrize('which', ['vid', 'shallow'])
def test_mixed_feature_dtypes_are_a_value_error(which):
    """on CPU tensors: the dtype check comes before the device check"""
    pkg = load_pkg()
    model = _tiny_model(pkg)
    assert model.half_features is True and model.last_feature_dtype is None
    vid, shallow = torch.zeros(1, 64, 64), torch.zeros(1, 64, 64)
    if which == 'vid':
        vid = vid.half()
    else:
        shallow = shallow.half()
    args = (vid, shallow, torch.ones(1, 64, dtype=torch.bool), (torch.zeros(1, 32, 4),), torch.zeros(1, 64), (torch.ones(1, 1, 4, dtype=torch.bool),))
    with pytest.raises(ValueError, match='float16 clip features come as a pair'):
        model(*args, eval=True)
    with pytest.raises(ValueError, match='float16 clip features come as a pair'):
        model.forward_videos([args])
    both = (vid.half(), shallow.half()) + args[2:]
    with pytest.raises(ValueError, match='all float16 or none'):
        model.forward_videos([both, (vid.float(), shallow.float()) + args[2:]])
    with pytest.raises(RuntimeError, match='MI355X only'):                  # a float16 pair passes the dtype check and meets the device check
        model(*both, eval=True)
    assert model.replica().half_features is True
    model.half_features = False
    assert model.replica().half_features is False


@pytest.mark.parametrize('M,N,K,nterms,addr,msg', [
    (6, 128, 32, 16, 4096, r'M %% 4 == 0'.replace('%%', '%')),        # the row pitch (lda = M halves) is not a multiple of 4
    (70, 128, 32, 6, 4096, 'M % 4 == 0'),
    (8, 128, 32, 16, 4096 + 2, '8-byte aligned'),
    (8, 128, 32, 16, 4096 + 4, '8-byte aligned'),
    (8, 64, 32, 16, 4096, 'N % 128 == 0'),
    (8, 128, 48, 16, 4096, 'K % 32 == 0'),
    (8, 128, 32, 3, 4096, 'nterms'),
])
def test_the_half_operator_refuses_bad_operands_before_a_launch(M, N, K, nterms, addr, msg):
    """the addresses are never dereferenced: the call fails in its argument checks (this machine has no GPU to launch on)"""
    pkg = load_pkg()
    lib = pkg._lib.lib()
    rc = lib.dcf_op_linear_cm_split_h(ctypes.c_void_p(addr), ctypes.c_void_p(4096), None, ctypes.c_void_p(4096), M, N, K, nterms, 0, None)
    assert rc == -1
    err = lib.dcf_last_error().decode()
    assert 'dcf_op_linear_cm_split_h' in err and msg in err, err


@pytest.mark.parametrize('M,lda,msg', [(8, 10, 'lda % 4 == 0'), (8, 14, 'lda % 4 == 0'), (8, 4, '>= M'), (8, 0, '>= M'), (6, 8, 'M % 4 == 0')])
def test_the_pitch_taking_half_operator_refuses_a_bad_pitch_before_a_launch(M, lda, msg):
    """a row pitch that is no multiple of four halves would put every second row of A_cm off the 8-byte grid of the kernel's loads"""
    pkg = load_pkg()
    lib = pkg._lib.lib()
    rc = lib.dcf_op_linear_cm_split_ld_h(ctypes.c_void_p(4096), lda, ctypes.c_void_p(4096), None, ctypes.c_void_p(4096), M, 128, 32, 16, 0, None)
    assert rc == -1
    err = lib.dcf_last_error().decode()
    assert msg in err, err


# ---------------------------------------------------------------------------------------------- the plane property
def _w(g, N, K):
    return torch.randn(N, K, generator=g) / K ** 0.5


def _without_mid_a(A, W, sa):
    ah, am = F.split(A, sa)
    wh, wm = F.split(W, F.SW)
    return (ah @ wh.t() + ah @ wm.t()) / (sa * F.SW), am


@pytest.mark.parametrize('sa', [1.0, F.SA])
@pytest.mark.parametrize('kind', ['normal', 'subnormal', 'large', 'zero-column'])
def test_a_representable_operand_has_no_mid_plane(sa, kind):
    g = torch.Generator().manual_seed(11)
    M, N, K = 68, 32, 64
    A = torch.randn(M, K, generator=g)
    if kind == 'subnormal':
        A = A * 2.0 ** -17                                 # |a| mostly below 2^-14, down to the last bit 2^-24
    elif kind == 'large':
        A = A * (4000.0 / float(A.abs().max()))            # the issue's range under scale 2^4: |a| < 4094
    A = A.half().float()                                   # binary16-representable
    if kind == 'zero-column':
        A[:, 5] = 0.0
    assert float(A.abs().max()) < (4094.0 if sa == F.SA else 65504.0)
    if kind == 'subnormal':
        assert int(((A != 0) & (A.abs() < F.F16_MIN_NORMAL)).sum()) > M * K // 2
    W = _w(g, N, K)
    hi, mid = F.split(A, sa)
    assert torch.equal(hi, A.double() * sa), 'the hi plane is the stored value times the power-of-two scale'
    assert int((mid != 0).sum()) == 0, 'the mid plane of a representable operand is all zero'
    two, _ = _without_mid_a(A, W, sa)
    assert torch.equal(two, F.gemm(A, W, sa=sa)), 'dropping a_mid . w_hi changes nothing'


@pytest.mark.parametrize('sa', [1.0, F.SA])
def test_an_operand_that_is_not_representable_needs_its_mid_plane(sa):
    """the check above can fail: for fp32 values with more than 11 significant bits the two-term product is another number"""
    g = torch.Generator().manual_seed(12)
    A, W = torch.randn(68, 64, generator=g), _w(g, 32, 64)
    assert not torch.equal(A.half().float(), A)
    two, am = _without_mid_a(A, W, sa)
    full = F.gemm(A, W, sa=sa)
    assert int((am != 0).sum()) > A.numel() // 2
    assert not torch.equal(two, full)
    assert float((two - full).abs().max()) > 2.0 ** -14 * float(full.abs().max()), 'an error of fp16 size, not of fp32 size'
    # and under scale 2^4 a half value of 4094 or more leaves the range: the envelope of unscaled = 0
    hi, _ = F.split(torch.tensor([4094.0, 4095.0, 4096.0]), F.SA)
    assert bool(torch.isinf(hi[1:]).all()) and float(hi[0]) == 65504.0
