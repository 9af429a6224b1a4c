"""CPU checks that go with dropout on the attention map (include/decafnet_hip_attn_drop.h, csrc/attn_drop.hip, ``autograd.DropSpec.attn_p``).

1. The declared boundary of the ``_lib.ATTN_DROP`` record: the table equals the header (tests/abi_headers.check_table), the built
   library exports the declared symbols and the version is 1, the source is part of the build, no name is shared with another table,
   ``EXTENSIONS`` / ``PENDING`` / ``STAGED`` / ``FIT`` / ``STEPLOG`` are what they were, and hipcc compiles the source for gfx950 without a
   warning under the project's flags.
2. Self-checks of the test-side restatement (they pass without the feature and are not coverage of it): tests/attn_drop_ref.py's hand-written backward equals autograd through its forward to fp64 rounding; with
   every element kept and p = 0 it is the dropout-free restatement of tests/attn_grad_ref.py; the element index is the flat index of
   the (bs, H, T, W) map with the sample offset by b0; a dropped map element removes exactly its key from the output.
3. ``DropSpec`` with and without ``attn_p``, and the refusals that come before a device check.
4. The opt-in: default ``enable_dropout()`` refuses as before; ``sites='all'`` is refused by ``model(...)`` and accepted by
   ``_train_dropout_rates()`` with every rate the reference takes, ``second_fusion`` and ``mha_win_size = 0`` included; rates outside
   [0, 1), ``cdrop`` with ``front_end='shared'`` and the single-head classes are refused, all before a device check.
5. tests/golden/attn_drop_ops.npz (make_golden_attn_drop.py): the restatement reproduces the reference's MaskedMHA under the stream,
   forward and ``backward()``, to fp64 rounding -- what ties the index convention to the reference -- and the conditions the generator
   asserted hold on the committed file."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import abi_headers as H
import attn_drop_abi_cases as C
import attn_drop_ref as R
import attn_grad_ref as G
import philox_ref as P
from conftest import load_pkg
from test_attn_grad_cpu import holes

SEED = 0x9E3779B97F4A7C15
SITE = P.site(2, 1, R.DROP_ATTN)


# ---------------------------------------------------------------------------------------------- 1. the boundary
def test_attn_drop_record_equals_its_header_and_the_library():
    pkg = load_pkg()
    L = pkg._lib
    assert len(L.ATTN_DROP) == 1
    ext = L.ATTN_DROP[0]
    assert ext == L.Extension('attn_drop', 'decafnet_hip_attn_drop.h', 'dcf_attn_drop_ext_version', 1, 'DCF_ATTN_DROP_EXT_VERSION',
                              ('decafnet_hip.h',), L.ATTN_DROP_TABLE)
    H.check_table(ext)
    assert sorted(ext.table) == ['dcf_attn_drop_ext_version', 'dcf_op_channel_dropout', 'dcf_op_global_attn_drop_bwd', 'dcf_op_local_attn_drop',
                                 'dcf_op_local_attn_drop_bwd', 'dcf_op_xattn_drop', 'dcf_op_xattn_drop_bwd']
    assert 'attn_drop.hip' in pkg.build.SOURCES
    h = ctypes.CDLL(pkg.build.build())
    for s in H.declared_symbols(ext.header):
        assert hasattr(h, s), f'{s} declared in include/{ext.header} but not exported'
    assert h.dcf_attn_drop_ext_version() == 1
    # every operator takes b0, seed, site, p after the arguments of its dropout-free form, in the order dcf_op_dropout has them
    tail = L.TRAIN_SIGNATURES['dcf_op_dropout'][1][-5:]
    assert L.ATTN_DROP_TABLE['dcf_op_local_attn_drop'][1] == L.SIGNATURES['dcf_op_local_attn'][1][:-1] + tail
    assert L.ATTN_DROP_TABLE['dcf_op_local_attn_drop_bwd'][1] == L.SIGNATURES['dcf_op_local_attn_bwd'][1][:-1] + tail
    assert L.ATTN_DROP_TABLE['dcf_op_global_attn_drop_bwd'][1] == L.ATTN_SIGNATURES['dcf_op_global_attn_bwd'][1][:-1] + tail
    assert L.ATTN_DROP_TABLE['dcf_op_xattn_drop'][1] == L.SIGNATURES['dcf_op_xattn'][1][:-1] + tail
    assert L.ATTN_DROP_TABLE['dcf_op_xattn_drop_bwd'][1] == L.SIGNATURES['dcf_op_xattn_bwd'][1][:-1] + tail
    assert L.ATTN_DROP_TABLE['dcf_op_channel_dropout'] == L.TRAIN_SIGNATURES['dcf_op_dropout']


def test_source_compiles_without_warnings_under_the_project_flags(tmp_path):
    b = load_pkg().build
    cmd = [b.hipcc()] + b.FLAGS + b.EXTRA.get('attn_drop.hip', []) + ['-c', os.path.join(b.CSRC, 'attn_drop.hip'), '-o', str(tmp_path / 'attn_drop.o')]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0 and 'warning' not in r.stderr and 'warning' not in r.stdout, r.stderr


def test_the_other_records_are_unchanged_and_share_no_name():
    L = load_pkg()._lib
    assert [e.key for e in L.EXTENSIONS] == ['base', 'train', 'dist', 'attn', 'front', 'guard', 'clock', 'half', 'front_half', 'embd']
    assert [e.key for e in L.PENDING] == ['batch'] and [e.key for e in L.STAGED] == ['eval'] and [e.key for e in L.FIT] == ['fit']
    assert [e.key for e in L.STEPLOG] == ['steplog']
    assert sorted(L.STEPLOG_TABLE) == ['dcf_op_steplog_add', 'dcf_op_steplog_flush', 'dcf_steplog_ext_version']
    assert not [n for n in dir(L) if n.endswith('SIGNATURES') and getattr(L, n) is L.ATTN_DROP_TABLE]
    others = L.EXTENSIONS + L.PENDING + L.STAGED + L.FIT + L.STEPLOG
    assert not {name for e in others for name in e.table} & set(L.ATTN_DROP_TABLE)
    assert L.ATTN_DROP[0].key not in {e.key for e in others} and L.ATTN_DROP[0].header not in {e.header for e in others}
    for e in others:
        assert not set(H.declared_symbols(e.header)) & set(L.ATTN_DROP_TABLE), e.header


def test_border_cases_cover_the_table_and_their_key_drops_and_keeps():
    table = load_pkg()._lib.ATTN_DROP_TABLE
    assert {c.export for c in C.CASES} | set(C.EXCLUDED) == set(table)
    for B, Cn in ((3, 4), (2, 68)):                       # the channel cases: some channel dropped, some kept
        keep = R.channel_keep(C.SEED, 7 << 16 | 7, B, Cn, C.P_DROP, C.B0)
        assert bool(keep.any()) and not bool(keep.all())


# ---------------------------------------------------------------------------------------------- 2. the restatement
def rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


def _case(B, T, Cn, seed):
    gen = torch.Generator().manual_seed(seed)
    q, k, v, dO = (torch.randn(B, T, Cn, dtype=torch.float64, generator=gen) for _ in range(4))
    return q, k, v, dO, holes(B, T, gen)


@pytest.mark.parametrize('B,T,Cn,heads,window,p,b0', [(2, 24, 16, 2, 5, 0.5, 0), (2, 40, 32, 4, 9, 0.1, 3), (3, 50, 16, 2, 19, 0.5, 3),
                                                      (2, 1, 16, 2, 9, 0.5, 0), (1, 11, 8, 1, 35, 0.1, 0)])
def test_closed_forms_equal_autograd_through_the_forward(B, T, Cn, heads, window, p, b0):
    q, k, v, dO, mask = _case(B, T, Cn, T * 31 + window)
    keep = R.window_keep(SEED, SITE, B, heads, T, window, p, b0)
    leaves = [z.clone().requires_grad_(True) for z in (q, k, v)]
    want = torch.autograd.grad((R.window_attention_drop(*leaves, mask, heads, window, keep, p) * dO).sum(), leaves)
    got = R.window_attention_drop_grads(q, k, v, mask, dO, heads, window, keep, p)
    for a, b in zip(got, want):
        assert rel(a, b) <= 1e-12 or float(b.abs().max()) == 0.0 == float(a.abs().max())


def test_without_dropout_it_is_the_dropout_free_restatement():
    B, T, Cn, heads, window = 2, 30, 16, 2, 9
    q, k, v, dO, mask = _case(B, T, Cn, 5)
    keep = R.window_keep(SEED, SITE, B, heads, T, window, 0.0)
    assert bool(keep.all()) and float(P.scale(0.0)) == 1.0
    assert torch.equal(R.window_attention_drop(q, k, v, mask, heads, window, keep, 0.0), G.window_attention(q, k, v, mask, heads, window))
    for a, b in zip(R.window_attention_drop_grads(q, k, v, mask, dO, heads, window, keep, 0.0),
                    G.window_attention_grads(q, k, v, mask, dO, heads, window)):
        assert torch.equal(a, b)


def test_element_index_is_the_flat_index_of_the_map_offset_by_b0():
    B, heads, T, window, p = 3, 2, 7, 5, 0.5
    big = R.window_keep(SEED, SITE, B + 2, heads, T, window, p)
    assert torch.equal(R.window_keep(SEED, SITE, B, heads, T, window, p, b0=2), big[2:])
    flat = P.keep(SEED, SITE, np.arange((B + 2) * heads * T * window, dtype=np.uint64), p)
    b, h, t, j = 3, 1, 4, 2
    assert bool(big[b, h, t, j]) == bool(flat[((b * heads + h) * T + t) * window + j])
    ck = R.channel_keep(SEED, 7 << 16 | 7, B + 2, 12, p)
    assert torch.equal(R.channel_keep(SEED, 7 << 16 | 7, B, 12, p, b0=2), ck[2:])
    assert bool(ck[3, 5]) == bool(P.keep(SEED, 7 << 16 | 7, np.array([3 * 12 + 5], dtype=np.uint64), p)[0])


def test_slot_j_of_row_t_is_key_t_minus_half_plus_j():
    """one dropped slot removes exactly the unit vector of its key from the output, scaled rows elsewhere"""
    B, T, heads, d, window, p = 1, 12, 1, 16, 5, 0.5
    v = torch.zeros(B, T, d, dtype=torch.float64)
    v[0, torch.arange(T), torch.arange(T)] = 1.0
    z = torch.zeros(B, T, d, dtype=torch.float64)
    keep = torch.ones(B, heads, T, window, dtype=torch.bool)
    t, j = 6, 1
    keep[0, 0, t, j] = False
    out = R.window_attention_drop(z, z, v, None, heads, window, keep, p)
    row = out[0, t]
    assert float(row[t - window // 2 + j]) == 0.0 and int((row != 0).sum()) == window - 1
    assert torch.allclose(row[row != 0], torch.tensor(float(P.scale(p)) / window, dtype=torch.float64))
    assert int((out[0, t - 1] != 0).sum()) == window


# ---------------------------------------------------------------------------------------------- 3. DropSpec and refusals
def test_drop_spec_round_trips_with_and_without_attn_p():
    A = load_pkg().autograd
    old = A.DropSpec(7, 2, 0.1, 0.2, A.DROP_G_STEM, 3)
    assert tuple(old) == (7, 2, 0.1, 0.2, A.DROP_G_STEM, 3, 0.0) and old.attn_p == 0.0 and old.active
    assert A.DropSpec(*old) == old and A.DropSpec(**old._asdict()) == old
    assert old.at(A.DROP_G_BRANCH, 1).attn_p == 0.0
    new = A.DropSpec(7, 2, group=A.DROP_G_STEM, layer=3, attn_p=0.25)
    assert new.active and new.proj_p == 0.0 == new.path_p and new.attn_p == 0.25
    assert A.DropSpec(*new) == new and new.at(A.DROP_G_BRANCH, 1).attn_p == 0.25
    assert new.site(A.DROP_ATTN) == P.site(A.DROP_G_STEM, 3, 6) and (A.DROP_ATTN, A.DROP_CHANNEL, A.DROP_G_INPUT) == (6, 7, 7)
    assert not A.DropSpec(7).active
    for bad in (-0.1, 1.0, 1.5, float('nan')):
        with pytest.raises(ValueError, match='attn_p'):
            A.DropSpec(7, attn_p=bad)


def test_drop_arguments_are_checked_before_a_device_check():
    A = load_pkg().autograd
    x = torch.zeros(1, 8, 64)                             # on the CPU: nothing may be launched
    for fn, args in ((A.window_attention, (x, x, x, None, 2, 9)), (A.global_attention, (x, x, x, None, 2)), (A.cross_attention, (x, x, x, None, 2))):
        with pytest.raises(TypeError, match='DropSpec'):
            fn(*args, drop=0.1)
    assert (A.DROP_G_TEXT, A.DROP_G_FUSION2, A.DROP_G_INPUT) == (5, 6, 7)


# ---------------------------------------------------------------------------------------------- 4. the opt-in
def _opt_in_model(rates, sites=None, **make):
    from test_dropout_cpu import _cpu_args, _model
    pkg = load_pkg()
    kw, opt = _model(pkg, rates)
    model = pkg.modeling.create_model(opt) if not make else pkg.modeling.PtTransformerEarlyFusionIterative(opt, **make)
    if sites is None:
        model.enable_dropout(seed=1)
    else:
        model.enable_dropout(seed=1, sites=sites)
    return pkg, model, _cpu_args(kw)


@pytest.mark.parametrize('part,key', [('vid_net', 'attn_pdrop'), ('vid_net', 'cdrop')])
def test_default_enable_dropout_refuses_the_new_sites_as_before(part, key):
    pkg, model, args = _opt_in_model({(part, key): 0.1})
    with pytest.raises(NotImplementedError, match=key):
        pkg.train.training_forward(model, *args)
    with pytest.raises(NotImplementedError, match=key):
        model._train_dropout_rates()
    with pytest.raises(NotImplementedError, match=key):
        model(*args)


def test_sites_all_is_refused_by_the_model_and_accepted_by_the_training_path():
    rates = {('vid_net', 'attn_pdrop'): 0.1, ('vid_net', 'cdrop'): 0.2, ('vid_net', 'proj_pdrop'): 0.3, ('fusion', 'path_pdrop'): 0.4}
    pkg, model, args = _opt_in_model(rates, 'all')
    with pytest.raises(NotImplementedError, match='attn_pdrop'):
        model(*args)                                      # the engine's training forward keeps refusing the key
    r = model._train_dropout_rates()
    M = pkg.modeling
    assert r == M.TrainDropRates(M.PartDropRates(0.3, 0.0, 0.1), M.PartDropRates(0.0, 0.4, 0.0), M.PartDropRates(0.0, 0.0, 0.0), 0.2, 0.5)
    with pytest.raises(RuntimeError, match='MI355X'):     # every check passed: the forward itself runs on the GPU only
        pkg.train.training_forward(model, *args)
    with pytest.raises(ValueError, match='cdrop'):        # before the device check
        pkg.train.training_forward(model, *args, front_end='shared')
    model.disable_dropout()
    with pytest.raises(NotImplementedError, match='attn_pdrop'):
        pkg.train.training_forward(model, *args)
    with pytest.raises(ValueError, match='sites'):
        model.enable_dropout(sites='everything')


def test_sites_engine_hands_the_training_path_the_engines_rates():
    pkg, model, args = _opt_in_model({('vid_net', 'proj_pdrop'): 0.1, ('fusion', 'path_pdrop'): 0.2}, 'engine')
    e, r = model._dropout_rates(), model._train_dropout_rates()
    assert e == (0.1, 0.0, 0.0, 0.2, 0.5)
    assert (r.vid_net, r.fusion, r.text_net, r.cdrop, r.refine) == ((0.1, 0.0, 0.0), (0.0, 0.2, 0.0), (0.0, 0.0, 0.0), 0.0, 0.5)
    model.disable_dropout()
    with pytest.raises(NotImplementedError, match='proj_pdrop'):
        model._train_dropout_rates()


@pytest.mark.parametrize('part,key,bad', [('vid_net', 'attn_pdrop', 1.0), ('vid_net', 'cdrop', -0.1), ('vid_net', 'attn_pdrop', float('nan')),
                                          ('fusion', 'proj_pdrop', 1.5)])
def test_sites_all_refuses_rates_outside_the_unit_interval(part, key, bad):
    pkg, model, args = _opt_in_model({(part, key): bad}, 'all')
    with pytest.raises(ValueError, match=f'{part}.{key}'):
        pkg.train.training_forward(model, *args)


def test_sites_all_accepts_every_rate_the_reference_takes():
    rates = {(part, key): 0.1 for part in ('vid_net', 'fusion', 'text_net') for key in ('attn_pdrop', 'proj_pdrop', 'path_pdrop')}
    rates[('vid_net', 'cdrop')] = 0.1
    for extra, make in (({}, {}), ({}, {'second_fusion': True}), ({('vid_net', 'mha_win_size'): 0}, {})):
        pkg, model, args = _opt_in_model({**rates, **extra}, 'all', **make)
        r = model._train_dropout_rates()
        assert r.vid_net == r.fusion == r.text_net == (0.1, 0.1, 0.1) and r.cdrop == 0.1 and r.refine == 0.5
        with pytest.raises(RuntimeError, match='MI355X'):     # every check passed: the forward itself runs on the GPU only
            pkg.train.training_forward(model, *args)
        with pytest.raises(NotImplementedError):              # the engine's training forward keeps refusing
            model(*args)
    pkg, model, args = _opt_in_model({('text_net', 'attn_pdrop'): 1.0}, 'all')
    with pytest.raises(ValueError, match='text_net.attn_pdrop'):
        pkg.train.training_forward(model, *args)


def test_sites_all_keeps_refusing_the_single_head_classes():
    from test_dropout_cpu import _cpu_args, _model
    pkg = load_pkg()
    kw, opt = _model(pkg, {('vid_net', 'attn_pdrop'): 0.1})
    for m in (pkg.modeling.PtTransformer(opt), pkg.modeling.PtTransformerEarlyFusion(opt, second_fusion=False)):
        m.enable_dropout(sites='all')
        with pytest.raises(NotImplementedError, match='PtTransformerEarlyFusionIterative only'):
            m._train_dropout_rates()


# ---------------------------------------------------------------------------------------------- 5. the fixture of the reference
OPS = 'attn_drop_ops.npz'


def ops_case(name, dtype):
    """(x token-major, mask, state dict, upstream gradient token-major, heads, window, p, key, site, keep, fixture) of case `name`"""
    from conftest import Golden
    g = Golden(OPS)
    meta = g.js('meta')
    c = meta['cases'][name]
    tm = lambda z: z.transpose(1, 2).contiguous().to(dtype)
    sd = {k: v.to(dtype) for k, v in g.sub('param/').items()}
    key, x = int(meta['key']), g.t(f'{name}/x')
    keep = R.window_keep(key, meta['site'], x.size(0), meta['heads'], c['T'], c['window'], meta['p'])
    return tm(x), g.t(f'{name}/mask'), sd, tm(g.t(f'{name}/up')), meta['heads'], c['window'], meta['p'], key, meta['site'], keep, g


@pytest.mark.parametrize('name', ['w9', 'w19'])
def test_restatement_reproduces_the_reference_with_map_dropout(name):
    """what ties the index convention to the reference: its fp64 forward and backward() under the stream, to fp64 rounding"""
    x, mask, sd, up, heads, window, p, key, site, keep, g = ops_case(name, torch.float64)
    xs = x.clone().requires_grad_(True)
    ps = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    y = R.masked_mha_drop(xs, xs, xs, mask, ps, heads, window, keep, p)
    grads = torch.autograd.grad((y * up).sum(), [xs] + list(ps.values()))
    assert rel(y.detach().transpose(1, 2), g.t(f'{name}/out64')) <= 1e-12
    assert rel(grads[0].transpose(1, 2), g.t(f'{name}/gx64')) <= 1e-12
    top = max(float(g.t(f'{name}/gp64/{k}').abs().max()) for k in ps)
    for k, gr in zip(ps, grads[1:]):
        want = g.t(f'{name}/gp64/{k}')
        assert float((gr - want).abs().max()) <= 1e-12 * (top if k == 'key.bias' else float(want.abs().max())), k
    # the hand-written backward of the core, through the projections by autograd
    q, k_, v = (G.conv1(x, sd, n) for n in ('query', 'key', 'value'))
    ctx = R.window_attention_drop(q, k_, v, mask, heads, window, keep, p).requires_grad_(True)
    dctx, = torch.autograd.grad((G.conv1(ctx, sd, 'proj') * up).sum(), ctx)
    dq, dk, dv = R.window_attention_drop_grads(q, k_, v, mask, dctx, heads, window, keep, p)
    gx = sum(d @ sd[n + '.weight'][:, :, 0] for d, n in ((dq, 'query'), (dk, 'key'), (dv, 'value')))
    assert rel(gx.transpose(1, 2), g.t(f'{name}/gx64')) <= 1e-12


@pytest.mark.parametrize('name', ['w9', 'w19'])
def test_conditions_on_the_committed_fixture(name):
    x, mask, sd, up, heads, window, p, key, site, keep, g = ops_case(name, torch.float64)
    assert p == 0.25 and site == P.site(P.G_BRANCH, 2, R.DROP_ATTN) and up.abs().min() > 0
    assert not bool(mask[1].all()) and bool(mask[0].all()), 'one sequence has a padded tail'
    assert bool(keep.any()) and not bool(keep.all()), 'the key both drops and keeps'
    valid = R.valid_slots(mask, window)[:, None].expand_as(keep)
    assert int((valid.any(-1) & ~(valid & keep).any(-1)).sum()) >= 1, 'a (row, head) loses all of its valid keys'
    for n in ['gx{}'] + ['gp{}/' + k for k in sd if k != 'key.bias']:          # key.bias: zero by symmetry, three roundings of 0
        g64, g32 = g.t(f'{name}/' + n.format('64')), g.t(f'{name}/' + n.format('32'))
        assert float((g32.double() - g64).abs().max()) <= 2.0 ** -15 * float(g64.abs().max()), n
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', OPS)) < (1 << 20)


@pytest.mark.parametrize('name', ['global', 'cross'])
def test_conditions_on_the_committed_dense_fixture(name):
    """tests/golden/attn_drop_ops_dense.npz (make_golden_attn_drop_dense.py): the global branch of the reference under the stream"""
    from conftest import Golden
    g = Golden('attn_drop_ops_dense.npz')
    meta = g.js('meta')
    q, mask = g.t(f'{name}/q'), g.t(f'{name}/mask')
    kv = q if name == 'global' else g.t(f'{name}/kv')
    keep = R.dense_keep(int(meta['key']), meta['site'], kv.size(0), meta['heads'], q.size(2), kv.size(2), meta['p'])
    assert bool(keep.any()) and not bool(keep.all()) and not bool(mask.all()) and bool(mask.any(1).all())
    assert meta['cases']['cross']['kv_size'] == [2, 1] and meta['cases']['global']['kv_size'] is None
    # the restatement reproduces the reference's fp64 output: the index of the map's dropout is key-minor
    sd = {k: v.double() for k, v in g.sub('param/').items()}
    tm = lambda z: z.double().transpose(1, 2)
    qp, kp, vp = G.conv1(tm(q), sd, 'query'), G.conv1(tm(kv), sd, 'key'), G.conv1(tm(kv), sd, 'value')
    if name == 'cross':
        qp = qp.repeat_interleave(torch.tensor([2, 1]), dim=0)
    y = G.conv1(R.dense_attention_drop(qp, kp, vp, mask, meta['heads'], keep, meta['p']), sd, 'proj').transpose(1, 2)
    assert rel(y, g.t(f'{name}/out64')) <= 1e-12
    names = ['gq{}'] + (['gkv{}'] if name == 'cross' else []) + ['gp{}/' + k for k in sd if k != 'key.bias']
    for n in names:
        g64, g32 = g.t(f'{name}/' + n.format('64')), g.t(f'{name}/' + n.format('32'))
        assert float((g32.double() - g64).abs().max()) <= 2.0 ** -15 * float(g64.abs().max()), n


@pytest.mark.parametrize('case', ['s2a', 's1g'])
def test_conditions_on_the_committed_step_fixtures(case):
    """tests/golden/step_grad_attn_drop_<case>*.npz (make_golden_step_grad_attn_drop.py): the reference's whole step with every site"""
    import step_grad_ref as S
    f = S.Fixture(f'attn_drop_{case}')
    m = f.meta
    assert (m['attn_pdrop'], m['proj_pdrop'], m['path_pdrop'], m['cdrop'], m['refine_pdrop'], m['text_dropout']) == (0.1, 0.2, 0.3, 0.1, 0.5, True)
    assert f.second_fusion == (case == 's2a') and f.opt_kwargs['win'] == (0 if case == 's1g' else 3)
    nq, n_layers = sum(f.text_size), 2
    sites = {s['site']: s for s in m['sites']}
    groups = {s >> 16 for s in sites}
    assert groups == {1, 2, 3, 4, 5, 7} | ({6} if case == 's2a' else set())
    paths = []
    for site, s in sites.items():
        n, sub = int(np.prod(s['shape'])), site & 15
        keep = P.keep(m['seed'], site, np.arange(n, dtype=np.uint64), {P.PATH_ATTN: 0.3, P.PATH_FFN: 0.3, P.TCN: 0.5, 6: 0.1, 7: 0.1}.get(sub, 0.2))
        assert int(keep.sum()) == s['kept'], (site, 'the recorded count is the stream\'s')
        if sub in (P.PATH_ATTN, P.PATH_FFN):
            assert s['shape'] == [nq]
            paths.append(keep)
        else:
            assert 0 < s['kept'] < n, (site, 'every dropout site both drops and keeps')
        if sub == 6:
            assert len(s['shape']) == 4, 'the attention map'
    # no drop-path site drops every row, at least one drops a row, at least one keeps all
    assert all(k.any() for k in paths) and any(not k.all() for k in paths) and any(k.all() for k in paths)
    assert sorted(m['path_sites']) == sorted(s for s in sites if s & 15 in (P.PATH_ATTN, P.PATH_FFN))
    if case == 's2a':                                     # the second fusion: layer l * n_layers + i of group 6, every sub of the fusion
        assert sorted((s >> 4) & 4095 for s in sites if s >> 16 == 6 and s & 15 == 6) == list(range(m['n_levels'] * n_layers))
        assert {s & 15 for s in sites if s >> 16 == 6} == {s & 15 for s in sites if s >> 16 == 1}
    ch = sites[P.site(R.DROP_G_INPUT, 0, R.DROP_CHANNEL)]
    assert ch['shape'][0] == nq
    keep = R.channel_keep(m['seed'], P.site(R.DROP_G_INPUT, 0, R.DROP_CHANNEL), nq, ch['shape'][1], 0.1)
    assert bool((keep.any(0) & ~keep.all(0)).any()), 'a channel is dropped for one sample and kept for another'
    for k in f.gp['64']:                                  # e_ref <= 2^-15 max|g_64|; every parameter takes a gradient
        g64, g32 = f.gp['64'][k], f.gp['32'][k]
        assert float((g32.double() - g64).abs().max()) <= 2.0 ** -15 * f.top(k), k
        assert bool(g32.any()) or k.endswith(('key.bias', 'k_norm.bias')), k
