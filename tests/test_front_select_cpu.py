"""CPU checks that go with the selected-clip training extension (include/decafnet_hip_front_select.h): the record
``_lib.FRONT_SELECT`` against its header (tests/abi_headers.py); the fp64 restatement of the two operators over (rows, row_first, pos)
(tests/front_select_ref.py) equals the restatement on dense features (tests/front_grad_ref.py) and meets the project's rule against the
reference's own fp64 yardstick on the fixtures (tests/golden/front_grad_<case>.npz); and ``train.training_forward`` /
``train.TrainStep`` refuse what their docstrings say before they look for a GPU.  No GPU."""
import pytest
import torch

import abi_headers as H
from conftest import load_pkg
import front_grad_ref as R
import front_select_ref as FS

NAMES = ['dcf_front_select_ext_version', 'dcf_op_vidmap_selected', 'dcf_op_vidmap_selected_bwd', 'dcf_op_vidmap_selected_bwd_h',
         'dcf_op_vidmap_selected_h']


# ---------------------------------------------------------------------------------------------- the ABI
def test_front_select_record_matches_its_header_and_is_staged():
    lb = load_pkg()._lib
    assert len(lb.FRONT_SELECT) == 1
    ext = lb.FRONT_SELECT[0]
    assert ext.table is lb.FRONT_SELECT_TABLE and sorted(ext.table) == NAMES
    assert (ext.key, ext.header, ext.version_symbol, ext.version) == ('front_select', 'decafnet_hip_front_select.h', 'dcf_front_select_ext_version', 1)
    H.check_table(ext)
    assert ext not in lb.EXTENSIONS                                    # staged after SELECT_VIDEOS: borders.TABLE has no row for it yet
    others = lb.EXTENSIONS + lb.PENDING + lb.STAGED + lb.FIT + lb.STEPLOG + lb.ATTN_DROP + lb.SELECT + lb.SELECT_VIDEOS
    assert not set(ext.table) & {n for e in others for n in e.table}
    assert 'front_select.hip' in load_pkg().build.SOURCES


# ---------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize('name', R.CASES)
def test_selected_formulas_equal_the_shared_formulas_and_meet_the_rule(name):
    f = R.Fixture(name)
    vid, shallow, gate, mask, correl, sizes, W, bias = f.operands(torch.float64, correl64=True)      # what the yardstick's vid_map saw
    dY = f.dY.double()
    rows, row_first, pos, counts = FS.fixture_pack(f)
    assert counts == [96, 31] and row_first == [0, 96, 127] and rows.shape == (127, f.D)
    assert int((pos[0] >= 0).sum()) == 96 and int((pos[1] >= 0).sum()) == 31
    y_s, (dw_s, db_s) = R.shared_forward(vid, shallow, gate, mask, correl, sizes, W, bias), R.shared_grads(vid, shallow, gate, mask, correl, sizes, dY)
    y_c = FS.selected_forward(rows, row_first, pos, shallow, gate, mask, correl, sizes, W, bias)
    dw_c, db_c = FS.selected_grads(rows, row_first, pos, shallow, gate, mask, correl, sizes, dY)
    for k, a, b, want in (('Y', y_c, y_s, f.y64), ('dW', dw_c, dw_s, f.dw64), ('db', db_c, db_s, f.db64)):
        top = float(b.abs().max())
        assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-12 * top, (name, k, float((a - b).abs().max()), top)
        assert float((a - want).abs().max()) <= R.rule(f.e_ref[k], f.top[k]), (name, k)


def test_restatement_ignores_capacity_rows_and_honours_a_missing_row():
    """rows beyond row_first[-1] are never read; pos = -1 under an open gate drops the expert half of that clip, forward and backward"""
    f = R.Fixture('msf+scat')
    vid, shallow, gate, mask, correl, sizes, W, bias = f.operands(torch.float64)
    dY = f.dY.double()
    rows, row_first, pos, _ = FS.fixture_pack(f)
    padded = torch.cat([rows, torch.full((5, f.D), float('nan'), dtype=rows.dtype)])
    base = FS.selected_forward(rows, row_first, pos, shallow, gate, mask, correl, sizes, W, bias)
    assert torch.equal(FS.selected_forward(padded, row_first, pos, shallow, gate, mask, correl, sizes, W, bias), base)
    assert torch.equal(FS.selected_grads(padded, row_first, pos, shallow, gate, mask, correl, sizes, dY)[0],
                       FS.selected_grads(rows, row_first, pos, shallow, gate, mask, correl, sizes, dY)[0])
    t = int((gate[0] != 0).nonzero()[0])
    assert mask[0, t] and pos[0, t] >= 0
    cut = pos.clone()
    cut[0, t] = -1
    y = FS.selected_forward(rows, row_first, cut, shallow, gate, mask, correl, sizes, W, bias)
    g0 = gate.clone()
    g0[:2, t] = 0.0                                                 # the same as a closed gate at that clip for the video's two queries
    assert float((y - R.shared_forward(vid, shallow, g0, mask, correl, sizes, W, bias)).abs().max()) <= 1e-12 * float(y.abs().max())
    dw = FS.selected_grads(rows, row_first, cut, shallow, gate, mask, correl, sizes, dY)[0]
    want = R.shared_grads(vid, shallow, g0, mask, correl, sizes, dY)[0]
    assert float((dw - want).abs().max()) <= 1e-12 * float(want.abs().max())


# ---------------------------------------------------------------------------------------------- what the Python layer refuses
def _model_and_batch(videos=None, **flags):
    import step_grad_ref as S
    pkg = load_pkg()
    f = S.Fixture('s2')
    opt = pkg.config.make_opt(**dict(f.opt_kwargs, **flags))
    model = pkg.modeling.PtTransformerEarlyFusionIterative(opt, second_fusion=f.second_fusion)
    batch = [f.vid, f.shallow, f.vid_masks, f.tokens.transpose(1, 2).contiguous(), f.text_cls, f.token_masks, f.text_size]
    if videos is not None:                                          # `videos` copies of the first video, one query each
        rep = lambda z: z[:1].expand(videos, *z.shape[1:]).contiguous()
        batch = [rep(z) for z in batch[:6]] + [[1] * videos]
    return pkg, model, batch


def test_an_unknown_expert_is_refused_before_anything_else():
    pkg = load_pkg()
    assert pkg.train.EXPERTS == ('dense', 'selected') and pkg.train.FRONT_ENDS == ('dense', 'shared')
    with pytest.raises(ValueError, match='expert'):
        pkg.train.training_forward(object(), None, None, None, None, None, None, expert='bogus')
    with pytest.raises(ValueError, match='expert'):
        pkg.train.TrainStep(None, None, expert='bogus')
    with pytest.raises(ValueError, match='expert_fn'):
        pkg.train.TrainStep(None, None, expert_fn=lambda b, clips: None)


def test_cdrop_is_refused_on_the_selected_path():
    from test_attn_drop_cpu import _opt_in_model
    pkg, model, args = _opt_in_model({('vid_net', 'cdrop'): 0.2}, 'all')
    with pytest.raises(ValueError, match="cdrop.*expert='dense'"):       # before the device check
        pkg.train.training_forward(model, *args, expert='selected')
    with pytest.raises(RuntimeError, match='MI355X'):
        pkg.train.training_forward(model, *args)


def test_sfonly_stays_refused_on_the_selected_path():
    pkg, model, batch = _model_and_batch(sfonly=True)
    with pytest.raises(NotImplementedError, match=r'model\.py:606-612'):
        pkg.train.training_forward(model, *batch, expert='selected')


def test_seventeen_videos_are_refused_with_the_way_out():
    pkg, model, batch = _model_and_batch(videos=17)
    with pytest.raises(ValueError, match='micro-batches'):
        pkg.train.training_forward(model, *batch, expert='selected')
    pkg, model, batch = _model_and_batch(videos=16)               # sixteen pass on to the device check
    with pytest.raises(RuntimeError, match='MI355X only'):
        pkg.train.training_forward(model, *batch, expert='selected')


def test_vid_rows_and_selection_come_together():
    pkg, model, batch = _model_and_batch()
    with pytest.raises(ValueError, match='come together'):
        pkg.train.training_forward(model, *batch, expert='selected', vid_rows=torch.zeros(4, 32))
    with pytest.raises(ValueError, match="expert='selected'"):
        pkg.train.training_forward(model, *batch, vid_rows=torch.zeros(4, 32), selection=object())


def test_selected_vid_map_refuses_gradients_mixes_shapes_and_the_cpu():
    pkg = load_pkg()
    f = R.Fixture('msf')
    _, shallow, gate, mask, correl, sizes, W, bias = f.operands(torch.float32)
    rows, row_first, pos, _ = FS.fixture_pack(f, torch.float32)
    call = lambda r=rows, first=row_first, sh=shallow, p=pos: pkg.autograd.selected_vid_map(r, first, p, sh, gate, mask, correl, sizes, W[:, :, None], bias)
    with pytest.raises(ValueError, match='requires a gradient'):
        call(r=rows.clone().requires_grad_(True))
    with pytest.raises(ValueError, match='float16 clip features come as a pair'):
        call(r=rows.half())
    with pytest.raises(RuntimeError, match='no CPU path'):
        call()
