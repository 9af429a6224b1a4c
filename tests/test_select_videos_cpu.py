"""Selected-clip inference on several videos per forward, without a GPU (include/decafnet_hip_select_videos.h):

1. The declared boundary of the ``_lib.SELECT_VIDEOS`` record: the table equals the header (tests/abi_headers.check_table), the built
   library exports the declared symbols and the version is 1, the source is part of the build, no name is shared with another
   record, and the case table of the border tests covers the record.
2. Self-checks of tests/select_videos_ref.py on a hand-made case (they pass without the feature and are not coverage of it).
3. The host-side refusals of the new methods and of the evaluator's switch, which come before any device check.
4. The precondition of the exact gate comparisons of tests/test_gpu_select_videos.py, from the oracle only: for every video and query
   of that file's seeded inputs and fixtures the gap between the k-th and the (k+1)-th pooled block score is printed (``SELVGAP``
   lines) and exceeds 1e-4 (the scoring kernels differ from the oracle by ~2e-6), for the fp32 features and for their float16
   rounding."""
import ctypes
import types

import pytest
import torch

import abi_headers as H
import forward_parity as P
import select_ref as S
import select_videos_abi_cases as C
import select_videos_ref as V
from conftest import load_pkg

NAMES = ['dcf_forward_eval_videos_selected', 'dcf_forward_eval_videos_selected_h', 'dcf_op_gather_clip_rows_videos',
         'dcf_op_gather_clip_rows_videos_h', 'dcf_op_select_clips_videos', 'dcf_select_videos', 'dcf_select_videos_ext_version',
         'dcf_select_videos_h']


# ---------------------------------------------------------------------------------------------- 1. the boundary
def test_select_videos_record_equals_its_header_and_the_library():
    pkg = load_pkg()
    L = pkg._lib
    assert len(L.SELECT_VIDEOS) == 1
    ext = L.SELECT_VIDEOS[0]
    assert ext == L.Extension('select_videos', 'decafnet_hip_select_videos.h', 'dcf_select_videos_ext_version', 1,
                              'DCF_SELECT_VIDEOS_EXT_VERSION', ('decafnet_hip.h',), L.SELECT_VIDEOS_TABLE)
    H.check_table(ext)
    assert sorted(ext.table) == NAMES
    assert 'select_videos.hip' in pkg.build.SOURCES and pkg.build.SOURCES[-1] == 'select.hip'
    h = ctypes.CDLL(pkg.build.build())
    for s in H.declared_symbols(ext.header):
        assert hasattr(h, s), f'{s} declared in include/{ext.header} but not exported'
    assert h.dcf_select_videos_ext_version() == 1
    # the forward: dcf_forward_eval_videos with (vid_rows, row_first, pos) in the place of vid and (gate, correl) in that of text_cls
    dense = L.SIGNATURES['dcf_forward_eval_videos'][1]
    IP = ctypes.POINTER(L.i32)
    assert L.SELECT_VIDEOS_TABLE['dcf_forward_eval_videos_selected'][1] == dense[:2] + [L.c_f32p, IP, L.c_i32p] + dense[3:10] + \
        [L.c_f32p, L.c_f32p] + dense[11:]
    assert L.SELECT_VIDEOS_TABLE['dcf_forward_eval_videos_selected_h'][1] == L.SELECT_VIDEOS_TABLE['dcf_forward_eval_videos_selected'][1]
    assert H.param_names(ext.header, 'dcf_forward_eval_videos_selected') == H.param_names(ext.header, 'dcf_forward_eval_videos_selected_h') == [
        'm', 'nvid', 'vid_rows', 'row_first', 'pos', 'shallow_vid', 'vid_mask', 'T', 'nq_per_video', 'text', 'text_mask', 'text_len', 'gate',
        'correl', 'logits_out', 'offsets_out', 'masks_out', 'stream']
    assert H.param_names(ext.header, 'dcf_select_videos') == H.param_names(ext.header, 'dcf_select_videos_h') == [
        'm', 'nvid', 'shallow_vid', 'vid_mask', 'T', 'nq_per_video', 'text_cls', 'gate_out', 'correl_out', 'clips_out', 'pos_out',
        'counts_out', 'stream']
    assert H.param_names(ext.header, 'dcf_op_select_clips_videos') == ['gate', 'vid_masks', 'T', 'nvid', 'nq_per_video', 'clips', 'pos',
                                                                       'counts', 'stream']
    assert H.param_names(ext.header, 'dcf_op_gather_clip_rows_videos') == H.param_names(ext.header, 'dcf_op_gather_clip_rows_videos_h') == [
        'X_cm', 'ldx', 'clips', 'T', 'nvid', 'row_first', 'D', 'rows', 'stream']
    src = open(pkg.build.CSRC + '/select_videos.hip').read() + open(pkg.build.CSRC + '/select.hip').read()
    assert src.count('select_clips_body(') == 2 and src.count('gather_clip_rows_tile<E>(') == 2, 'one device body, called by both kernels'


def test_the_new_names_collide_with_no_other_record():
    L = load_pkg()._lib
    others = L.EXTENSIONS + L.PENDING + L.STAGED + L.FIT + L.STEPLOG + L.ATTN_DROP + L.SELECT
    assert not {name for e in others for name in e.table} & set(L.SELECT_VIDEOS_TABLE)
    ext = L.SELECT_VIDEOS[0]
    assert ext.key not in {e.key for e in others} and ext.header not in {e.header for e in others}
    for e in others:
        assert not set(H.declared_symbols(e.header)) & set(L.SELECT_VIDEOS_TABLE), e.header
    assert not set(H.declared_symbols(ext.header)) & {name for e in others for name in e.table}
    assert not [n for n in dir(L) if n.endswith('SIGNATURES') and getattr(L, n) is L.SELECT_VIDEOS_TABLE]


def test_border_cases_cover_the_table():
    table = load_pkg()._lib.SELECT_VIDEOS_TABLE
    assert {c.export for c in C.CASES} | set(C.EXCLUDED) == set(table)
    ids = [f'{c.export}-{c.tag}' for c in C.CASES]
    assert len(set(ids)) == len(ids)


# ---------------------------------------------------------------------------------------------- 2. the restatement
def test_restatement_of_the_packed_lists():
    gate = torch.tensor([[1., 1, 0, 0, 0, 0, 1, 1], [0., 0, 0, 0, 1, 1, 1, 1],        # video 0: two queries
                         [0., 1, 1, 0, 0, 0, 0, 0]])                                   # video 1: one
    masks = torch.tensor([[1, 1, 1, 1, 1, 1, 1, 0], [1, 1, 0, 0, 0, 0, 0, 0]], dtype=torch.uint8)
    clips, pos, counts, row_first = V.select_clips_videos(gate, masks, [2, 1])
    assert counts == [5, 1] and row_first == [0, 5, 6]
    assert clips.tolist() == [[0, 1, 4, 5, 6, -7, -7, -7], [1, -7, -7, -7, -7, -7, -7, -7]]
    assert pos.tolist() == [[0, 1, -1, -1, 2, 3, 4, -1], [-1, 0, -1, -1, -1, -1, -1, -1]]
    for v, q in ((0, slice(0, 2)), (1, slice(2, 3))):                                  # per video it IS select_ref.select_clips
        c1, p1, n1 = S.select_clips(gate[q], masks[v])
        assert n1 == counts[v] and torch.equal(clips[v, :n1], c1) and torch.equal(pos[v], p1)
    xs = [torch.arange(24.).reshape(3, 8), 100 + torch.arange(24.).reshape(3, 8)]
    rows = V.gather_clip_rows_videos(xs, clips, counts)
    assert rows.tolist() == [[0, 8, 16], [1, 9, 17], [4, 12, 20], [5, 13, 21], [6, 14, 22], [101, 109, 117]]


# ---------------------------------------------------------------------------------------------- 3. the refusals
def _cpu_model(pkg, **over):
    kw = dict(V.KW3)
    kw.update(over)
    return pkg.modeling.create_model(pkg.config.make_opt(**kw))


def _video(T=128, nq=1):
    return (None, torch.zeros(1, 64, T), torch.ones(1, T, dtype=torch.bool), tuple(() for _ in range(nq)), torch.zeros(nq, 64),
            tuple(() for _ in range(nq)))


def _batch(counts, nqs, scores=None, T=128):
    pkg = load_pkg()
    nv = len(counts)
    return pkg.modeling.SelectionBatch(torch.zeros(sum(nqs), T), torch.zeros(nv, T, dtype=torch.int32), torch.zeros(nv, T, dtype=torch.int32),
                                       scores, counts, nqs)


@pytest.mark.parametrize('over,word', [(dict(sfonly=True), 'sfonly'), (dict(vid_stride=2), 'stride')])
def test_sfonly_and_stride_are_refused_before_any_device_check(over, word):
    model = _cpu_model(load_pkg(), **over)
    with pytest.raises(NotImplementedError, match=word):
        model.select_clips_videos([_video(), _video()])
    with pytest.raises(NotImplementedError, match=word):
        model.forward_videos_selected(torch.zeros(8, 64), _batch([4, 4], [1, 1]), [_video(), _video()])


def test_video_counts_lengths_scores_and_rows_are_refused_before_any_device_check():
    pkg = load_pkg()
    model = _cpu_model(pkg)
    with pytest.raises(ValueError, match='16 videos'):
        model.select_clips_videos([_video()] * 17)
    with pytest.raises(ValueError, match='16 videos'):
        model.forward_videos_selected(torch.zeros(17, 64), _batch([1] * 17, [1] * 17), [_video()] * 17)
    with pytest.raises(ValueError, match='padded length'):
        model.select_clips_videos([_video(128), _video(256)])
    with pytest.raises(ValueError, match='padded length'):
        model.forward_videos_selected(torch.zeros(8, 64), _batch([4, 4], [1, 1]), [_video(128), _video(256)])
    batch = _batch([4, 3], [1, 2])
    assert batch.row_first == [0, 4, 7] and batch.n_rows == 7 and batch.nvid == 2 and batch.T == 128
    sel = batch.selection(1)
    assert isinstance(sel, pkg.modeling.Selection) and sel.count == 3 and sel.nq == 2 and sel.pos.shape == (128,)
    videos = [_video(nq=1), _video(nq=2)]
    for bad in (torch.zeros(6, 64), torch.zeros(7, 60), torch.zeros(7 * 64)):                # row_first does not match vid_rows
        with pytest.raises(ValueError, match='vid_rows'):
            model.forward_videos_selected(bad, batch, videos)
    with pytest.raises(ValueError, match='selection'):
        model.forward_videos_selected(torch.zeros(7, 64), batch, [_video(nq=2), _video(nq=1)])
    with pytest.raises(ValueError, match='empty'):
        model.forward_videos_selected(torch.zeros(4, 64), _batch([4, 0], [1, 2]), videos)
    with pytest.raises(RuntimeError, match='GPU'):                                            # every host check passed
        model.forward_videos_selected(torch.zeros(7, 64), batch, videos)
    scat = _cpu_model(pkg, scat=True)
    with pytest.raises(ValueError, match='scat'):
        scat.forward_videos_selected(torch.zeros(7, 64), batch, videos)                       # a scat model and a batch without scores
    with pytest.raises(RuntimeError, match='GPU'):
        scat.forward_videos_selected(torch.zeros(7, 64), _batch([4, 3], [1, 2], scores=torch.zeros(3, 128)), videos)
    # the one-video methods keep their refusal of scat
    with pytest.raises(NotImplementedError, match='scat'):
        scat.select_clips(torch.zeros(1, 64, 128), torch.ones(1, 128, dtype=torch.bool), torch.zeros(1, 64))


def test_evaluator_switch():
    pkg = load_pkg()
    opt = pkg.config.make_opt(**V.TINY)
    model = pkg.modeling.create_model(opt)
    ev = pkg.evaluator.GroundingEvaluator
    assert ev(opt, model).select_videos is False and ev(opt, model, expert='selected').select_videos is False
    assert ev(opt, model, expert='selected', select_videos=True).select_videos is True
    with pytest.raises(ValueError, match='select_videos'):
        ev(opt, model, select_videos=True)
    with pytest.raises(ValueError, match='select_videos'):
        ev(opt, model, expert='dense', select_videos=True)
    with pytest.raises(NotImplementedError, match='batch_videos'):
        ev(opt, model, expert='selected').run([], batch_videos=2)
    counter = ev(opt, model, expert='selected', select_videos=True).run([], batch_videos=3)    # an empty dataset: no forward at all
    assert counter.n_queries == 0
    scat = pkg.modeling.create_model(pkg.config.make_opt(**dict(V.TINY, scat=True)))
    assert ev(pkg.config.make_opt(**dict(V.TINY, scat=True)), scat, expert='selected', select_videos=True).run([], batch_videos=2).n_queries == 0


# ---------------------------------------------------------------------------------------------- 4. the gaps
def _print_and_check(tag, gaps):
    for q, gap in enumerate(gaps):
        print(f'SELVGAP {tag} q{q}: {gap:.6e}')
    assert gaps and min(gaps) > S.GAP_MIN, (tag, gaps)


@pytest.mark.parametrize('half', [False, True])
def test_the_gates_of_the_three_videos_are_decided_by_a_margin(half):
    pkg = load_pkg()
    rnd = (lambda x: x.half().float()) if half else (lambda x: x)
    for kw in (V.KW3, dict(V.KW3, msf=False), dict(V.KW3, scat=True)):                     # (the gate reads sn, sratio and norm only)
        cfg = pkg.config.make_opt(**kw).model
        for v, inp in enumerate(V.three_inputs(pkg)):
            gaps = S.gate_gaps(cfg, rnd(inp['shallow_vid']), inp['vid_masks'], inp['text_cls'])
            assert len(gaps) == V.LENS3[v][1]
            _print_and_check(f'three-videos msf={kw["msf"]} scat={kw.get("scat", False)} half={half} v{v}', gaps)


@pytest.mark.parametrize('name', ['c1', 'scat'])
def test_the_gates_of_the_fixtures_and_their_second_video_are_decided_by_a_margin(name):
    pkg = load_pkg()
    c = P.e2e_case(name)
    assert bool(c.opt.model.get('scat', False)) == (name == 'scat')
    _print_and_check(f'e2e_{name}', S.gate_gaps(c.opt.model, c.inp['shallow_vid'], c.inp['vid_masks'], c.inp['text_cls']))
    second = V.second_input(pkg, c)
    assert second['shallow_vid'].shape == c.inp['shallow_vid'].shape
    _print_and_check(f'e2e_{name} second video', S.gate_gaps(c.opt.model, second['shallow_vid'], second['vid_masks'], second['text_cls']))


def test_the_gates_of_the_evaluator_samples_are_decided_by_a_margin():
    cfg = load_pkg().config.make_opt(**V.TINY).model
    for s in V.evaluator_samples():
        _print_and_check(f'evaluator {s["clip_id"]}', V.sample_gaps(cfg, s))
