"""Selected-clip inference without a GPU (include/decafnet_hip_select.h):

1. The declared boundary of the ``_lib.SELECT`` record: the table equals the header (tests/abi_headers.check_table), the built
   library exports the declared symbols and the version is 1, the source is part of the build, no name is shared with another table,
   the other records are what they were, and the case table of the border tests covers the record.
2. The premise, on the reference side alone.  For the fixtures e2e_c1, e2e_pe, e2e_nomsf and e2e_affine the union of the oracle's
   gates is formed, and every expert feature OUTSIDE it is replaced by zero and by a large finite value: ``oracle.forward_eval`` on
   either must be ``torch.equal`` to ``oracle.forward_eval`` on the fixture's own inputs (the fixture forward: the same function, the
   same weights and texts; what the reference recorded in the fixture agrees with it to the oracle's tolerance,
   tests/test_oracle_golden.py).  So the expert features of the clips that ``select_clips`` does not list cannot matter.
3. The precondition of the exact gate comparison of tests/test_gpu_select.py, from the oracle only: per query of these fixtures the
   gap between the k-th and the (k+1)-th pooled block score is printed (``SELGAP`` lines) and exceeds 1e-4.
4. Self-checks of tests/select_ref.py (they pass without the feature and are not coverage of it), and the host-side refusals of the
   new methods that come before a device check."""
import ctypes

import pytest
import torch

import abi_headers as H
import forward_parity as P
import select_abi_cases as C
import select_ref as S
from conftest import load_pkg


# ---------------------------------------------------------------------------------------------- 1. the boundary
def test_select_record_equals_its_header_and_the_library():
    pkg = load_pkg()
    L = pkg._lib
    assert len(L.SELECT) == 1
    ext = L.SELECT[0]
    assert ext == L.Extension('select', 'decafnet_hip_select.h', 'dcf_select_ext_version', 1, 'DCF_SELECT_EXT_VERSION', ('decafnet_hip.h',),
                              L.SELECT_TABLE)
    H.check_table(ext)
    assert sorted(ext.table) == ['dcf_forward_eval_selected', 'dcf_forward_eval_selected_h', 'dcf_op_gather_clip_rows',
                                 'dcf_op_gather_clip_rows_h', 'dcf_op_select_clips', 'dcf_select_ext_version']
    assert pkg.build.SOURCES[-1] == 'select.hip'
    h = ctypes.CDLL(pkg.build.build())
    for s in H.declared_symbols(ext.header):
        assert hasattr(h, s), f'{s} declared in include/{ext.header} but not exported'
    assert h.dcf_select_ext_version() == 1
    # the forwards: dcf_forward_eval_gated with (vid_rows, n_rows, pos) in the place of vid; the half form differs in pointer types only
    gated = L.SIGNATURES['dcf_forward_eval_gated'][1]
    assert L.SELECT_TABLE['dcf_forward_eval_selected'][1] == gated[:2] + [L.i32, L.c_i32p] + gated[2:]
    assert L.SELECT_TABLE['dcf_forward_eval_selected_h'][1] == L.SELECT_TABLE['dcf_forward_eval_selected'][1]
    assert H.param_names(ext.header, 'dcf_forward_eval_selected') == H.param_names(ext.header, 'dcf_forward_eval_selected_h') == [
        'm', 'vid_rows', 'n_rows', 'pos', 'shallow_vid', 'vid_mask', 'T', 'nq', 'text', 'text_mask', 'text_len', 'gate', 'logits_out',
        'offsets_out', 'masks_out', 'stream']
    assert H.param_names(ext.header, 'dcf_op_select_clips') == ['gate', 'vid_mask', 'T', 'nq', 'clips', 'pos', 'count', 'stream']
    assert H.param_names(ext.header, 'dcf_op_gather_clip_rows') == H.param_names(ext.header, 'dcf_op_gather_clip_rows_h') == [
        'X_cm', 'ldx', 'clips', 'n', 'D', 'rows', 'stream']


def test_the_other_records_are_unchanged_and_share_no_name():
    L = load_pkg()._lib
    assert [e.key for e in L.EXTENSIONS] == ['base', 'train', 'dist', 'attn', 'front', 'guard', 'clock', 'half', 'front_half', 'embd']
    assert [e.key for e in L.PENDING + L.STAGED + L.FIT + L.STEPLOG + L.ATTN_DROP] == ['batch', 'eval', 'fit', 'steplog', 'attn_drop']
    assert not [n for n in dir(L) if n.endswith('SIGNATURES') and getattr(L, n) is L.SELECT_TABLE]
    others = L.EXTENSIONS + L.PENDING + L.STAGED + L.FIT + L.STEPLOG + L.ATTN_DROP
    assert not {name for e in others for name in e.table} & set(L.SELECT_TABLE)
    assert L.SELECT[0].key not in {e.key for e in others} and L.SELECT[0].header not in {e.header for e in others}
    for e in others:
        assert not set(H.declared_symbols(e.header)) & set(L.SELECT_TABLE), e.header


def test_border_cases_cover_the_table():
    table = load_pkg()._lib.SELECT_TABLE
    assert {c.export for c in C.CASES} | set(C.EXCLUDED) == set(table)
    ids = [f'{c.export}-{c.tag}' for c in C.CASES]
    assert len(set(ids)) == len(ids)


# ---------------------------------------------------------------------------------------------- 2. the premise, 3. the gaps
def _oracle_forward(c, vid):
    texts = [t.float() for t in c.y64['text']]                 # one set of encoded texts for all three forwards
    with torch.no_grad():
        return S.R.forward_eval(c.sd, c.opt.model, vid, c.inp['shallow_vid'], c.inp['vid_masks'], texts, c.inp['text_cls'], c.tmasks)


@pytest.mark.parametrize('name', S.FIXTURES)
def test_expert_features_outside_the_union_of_the_gates_do_not_matter(name):
    c = P.e2e_case(name)
    cfg, inp = c.opt.model, c.inp
    assert not cfg.get('scat', False) and not cfg.get('sfonly', False)
    gate = S.oracle_gates(cfg, inp['shallow_vid'], inp['vid_masks'], inp['text_cls'])
    clips, pos, count = S.select_clips(gate, inp['vid_masks'][0])
    vid_len, T = int(inp['vid_masks'].sum()), inp['vid'].shape[-1]
    assert 0 < count < vid_len, 'the fixture must leave clips outside the union, or this test shows nothing'
    assert int(clips.max()) < vid_len and bool((pos[vid_len:] == -1).all())
    outside = torch.ones(T, dtype=torch.bool)
    outside[clips.long()] = False
    want = _oracle_forward(c, inp['vid'])
    for fill in (0.0, 3.0e4):
        vid = inp['vid'].clone()
        vid[:, :, outside] = fill
        assert not torch.equal(vid, inp['vid'])
        got = _oracle_forward(c, vid)
        for part_w, part_g in zip(want, got):
            for q in range(c.nq):
                for l in range(c.L):
                    assert torch.equal(part_w[q][l], part_g[q][l]), (name, fill, q, l)
    # what the reference recorded agrees with the oracle's forward on the same inputs (its own text encoding) to the oracle's tolerance
    for q in range(c.nq):
        for l in range(c.L):
            torch.testing.assert_close(want[0][q][l], c.y32['logits'][q][l], rtol=2e-5, atol=2e-5)
            assert torch.equal(want[2][q][l], c.masks[q][l])


@pytest.mark.parametrize('name', S.FIXTURES)
def test_the_gates_of_the_fixtures_are_decided_by_a_margin(name):
    c = P.e2e_case(name)
    gaps = S.gate_gaps(c.opt.model, c.inp['shallow_vid'], c.inp['vid_masks'], c.inp['text_cls'])
    assert len(gaps) == c.nq
    for q, gap in enumerate(gaps):
        print(f'SELGAP e2e_{name} q{q}: {gap:.6e}')
    assert min(gaps) > S.GAP_MIN, (name, gaps)


# ---------------------------------------------------------------------------------------------- 4. the restatement, the refusals
def test_restatement_of_the_clip_list():
    gate = torch.tensor([[1., 1, 0, 0, 0, 0, 1, 1], [0., 0, 0, 0, 1, 1, 1, 1]])
    mask = torch.tensor([1, 1, 1, 1, 1, 1, 1, 0], dtype=torch.uint8)
    clips, pos, n = S.select_clips(gate, mask)
    assert n == 5 and clips.tolist() == [0, 1, 4, 5, 6] and pos.tolist() == [0, 1, -1, -1, 2, 3, 4, -1]
    x = torch.arange(24.).reshape(3, 8)
    assert S.gather_clip_rows(x, clips).tolist() == [[0, 8, 16], [1, 9, 17], [4, 12, 20], [5, 13, 21], [6, 14, 22]]
    clips, pos, n = S.select_clips(torch.zeros(1, 4), torch.ones(4, dtype=torch.uint8))
    assert n == 0 and clips.numel() == 0 and pos.tolist() == [-1] * 4


def _cpu_model(pkg, **over):
    kw = dict(D=64, E=64, TE=32, text_in=32, n_levels=4, win=5, n_heads=4, sn=8, sratio=0.3, msf=True, norm=True, max_seq_len=128,
              text_layers=1, text_max_len=24)
    kw.update(over)
    return pkg.modeling.create_model(pkg.config.make_opt(**kw))


@pytest.mark.parametrize('over,word', [(dict(scat=True), 'scat'), (dict(sfonly=True), 'sfonly'), (dict(vid_stride=2), 'stride')])
def test_refusals_come_before_any_device_check(over, word):
    pkg = load_pkg()
    model = _cpu_model(pkg, **over)
    sh, mask, cls = torch.zeros(1, 64, 128), torch.ones(1, 128, dtype=torch.bool), torch.zeros(1, 64)
    with pytest.raises(NotImplementedError, match=word):
        model.select_clips(sh, mask, cls)
    with pytest.raises(NotImplementedError, match=word):
        model.forward_selected(torch.zeros(8, 64), None, sh, mask, (), ())


def test_evaluator_options():
    pkg = load_pkg()
    model = _cpu_model(pkg)
    opt = pkg.config.make_opt(D=64, E=64, TE=32, text_in=32, n_levels=4, win=5, n_heads=4, sn=8, sratio=0.3, msf=True, norm=True,
                              max_seq_len=128, text_layers=1, text_max_len=24, max_vid_len=128)
    ev = pkg.evaluator.GroundingEvaluator
    assert ev(opt, model).expert == 'dense'
    assert ev(opt, model, expert='selected').expert_fn is None
    with pytest.raises(ValueError, match='expert'):
        ev(opt, model, expert='sparse')
    with pytest.raises(ValueError, match='expert_fn'):
        ev(opt, model, expert_fn=lambda sample, clips: None)
    with pytest.raises(NotImplementedError, match='batch_videos'):
        ev(opt, model, expert='selected').run([], batch_videos=2)
