"""CPU checks of the training forward's dropout: the numpy restatement of the random stream (tests/philox_ref.py) against
Philox4x32-10's known answers, the dropout fixture's recorded masks against the restatement, and the refusals of
enable_dropout()'s forward -- all raised before anything touches the GPU."""
import numpy as np
import pytest
import torch

import philox_ref as P
from conftest import Golden, load_pkg


def test_philox_known_answers():
    cases = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
             ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
             ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in cases:
        assert tuple(int(x) for x in P.philox4x32_10(np.array(ctr, dtype=np.uint64), key)) == want


def test_element_words_follow_the_counter_layout():
    seed, s = 0x0123456789ABCDEF, P.site(3, 2, 1)
    e = np.array([0, 1, 2, 3, 4, (1 << 34) + 6], dtype=np.uint64)
    blocks = [P.philox4x32_10(np.array([j & 0xffffffff, j >> 32, s, 0], dtype=np.uint64), (seed & 0xffffffff, seed >> 32))
              for j in (0, 1, (1 << 32) + 1)]
    want = [blocks[0][0], blocks[0][1], blocks[0][2], blocks[0][3], blocks[1][0], blocks[2][2]]
    assert [int(x) for x in P.words(seed, s, e)] == [int(x) for x in want]


def test_fixture_masks_match_the_restatement():
    g = Golden('train_dropout.npz')
    for case in g.js('cases'):
        meta = g.js(f'{case}/meta')
        seed = meta['seed']
        sites = g.js(f'{case}/sites')
        groups = {s['site'] >> 16 for s in sites}
        assert groups == {1, 3, 4} | ({2} if g.js(f'{case}/opt_kwargs').get('n_stem', 0) else set())
        for s in sites:
            sub = s['site'] & 15
            p = meta['path_pdrop'] if sub in (P.PATH_ATTN, P.PATH_FFN) else meta['refine_pdrop'] if sub == P.TCN else meta['proj_pdrop']
            n = int(np.prod(s['shape']))
            want = np.packbits(P.keep(seed, s['site'], np.arange(min(n, 4096), dtype=np.uint64), p))
            assert np.array_equal(g.z[f'{case}/keep/{s["site"]}'], want), (case, s)
            if case == 'e64':                # the small case: the whole site's keep count
                assert int(P.keep(seed, s['site'], np.arange(n, dtype=np.uint64), p).sum()) == s['kept'], (case, s)
        # the seed was picked so that drop-path both fires and keeps
        assert int(g.z[f'{case}/path_fired']) > 0 and int(g.z[f'{case}/path_kept']) > 0


def _model(pkg, rates=None):
    kw = Golden('train.npz').js('opt_kwargs')
    opt = pkg.config.make_opt(**kw)
    for (part, key), v in (rates or {}).items():
        opt.model[part][key] = v
    return kw, opt


def _cpu_args(kw):
    T = 128
    return (torch.zeros(1, kw['D'], T), torch.zeros(1, kw['D'], T), torch.ones(1, T, dtype=torch.bool),
            torch.zeros(1, kw['text_in'], 4), torch.zeros(1, kw['D']), torch.ones(1, 1, 4, dtype=torch.bool))


@pytest.mark.parametrize('part,key', [('vid_net', 'attn_pdrop'), ('fusion', 'attn_pdrop'), ('vid_net', 'cdrop'),
                                      ('text_net', 'attn_pdrop'), ('text_net', 'proj_pdrop'), ('text_net', 'path_pdrop')])
def test_enabled_dropout_refuses_what_it_does_not_implement(part, key):
    pkg = load_pkg()
    kw, opt = _model(pkg, {(part, key): 0.1})
    model = pkg.modeling.create_model(opt)
    model.enable_dropout(seed=1)
    with pytest.raises(NotImplementedError, match=key):
        model(*_cpu_args(kw))


def test_enabled_dropout_refuses_second_fusion_and_single_head_classes():
    pkg = load_pkg()
    kw, opt = _model(pkg, {('vid_net', 'proj_pdrop'): 0.1})
    m = pkg.modeling.PtTransformerEarlyFusionIterative(opt, second_fusion=True)
    m.enable_dropout()
    with pytest.raises(NotImplementedError, match='second_fusion'):
        m(*_cpu_args(kw))
    for m in (pkg.modeling.PtTransformer(opt), pkg.modeling.PtTransformerEarlyFusion(opt, second_fusion=False)):
        m.enable_dropout()
        with pytest.raises(NotImplementedError, match='PtTransformerEarlyFusionIterative only'):
            m(*_cpu_args(kw))


def test_rates_outside_unit_interval_are_refused():
    pkg = load_pkg()
    kw, opt = _model(pkg)
    model = pkg.modeling.create_model(opt)
    for bad in (1.0, -0.1, 1.5, float('nan')):
        with pytest.raises(ValueError, match='refine_pdrop'):
            model.enable_dropout(refine_pdrop=bad)
    kw, opt = _model(pkg, {('fusion', 'path_pdrop'): 1.0})
    model = pkg.modeling.create_model(opt)
    model.enable_dropout()
    with pytest.raises(ValueError, match='fusion.path_pdrop'):
        model(*_cpu_args(kw))


def test_enabled_dropout_reaches_the_gpu_check_and_disable_restores_the_refusal():
    pkg = load_pkg()
    kw, opt = _model(pkg, {('vid_net', 'proj_pdrop'): 0.1, ('fusion', 'path_pdrop'): 0.1})
    model = pkg.modeling.create_model(opt)
    model.enable_dropout(seed=3)
    with pytest.raises(RuntimeError, match='GPU'):       # every check passed: the forward itself runs on the MI355X only
        model(*_cpu_args(kw))
    model.disable_dropout()
    with pytest.raises(NotImplementedError, match='proj_pdrop'):
        model(*_cpu_args(kw))
