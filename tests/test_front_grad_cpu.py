"""CPU checks that go with the training-front-end extension (include/decafnet_hip_front.h; its header and table:
tests/test_abi_headers.py): the names of ``_lib.FRONT_SIGNATURES`` and the flag the header defines; the fp64 restatement of vid_map on shared products
(tests/front_grad_ref.py) equals the dense formula and the reference's own fp64 yardstick on the fixtures
(tests/golden/front_grad_<case>.npz) and central finite differences; the fixtures are what their generator says they are; and
``train.training_forward`` admits and refuses what its docstring says.  No GPU."""
import os

import pytest
import torch

import abi_headers as H
from conftest import GOLDEN, load_pkg
import front_grad_ref as R

NAMES = ['dcf_front_ext_version', 'dcf_op_vidmap_shared', 'dcf_op_vidmap_shared_bwd']
LIMIT = 1 << 20
E_REF_CAP = 2.0 ** -15


# ---------------------------------------------------------------------------------------------- the ABI
def test_front_table_names_flag_and_source():
    pkg = load_pkg()
    assert sorted(pkg._lib.FRONT_SIGNATURES) == NAMES
    assert f'#define DCF_FRONT_NO_SKIP {pkg._lib.FRONT_NO_SKIP}' in H.source_of('decafnet_hip_front.h')
    assert 'front_grad.hip' in pkg.build.SOURCES


# ---------------------------------------------------------------------------------------------- the fixtures
@pytest.mark.parametrize('name', R.CASES)
def test_fixture_is_what_the_generator_says(name):
    f = R.Fixture(name)
    assert 0 < os.path.getsize(os.path.join(GOLDEN, f'front_grad_{name}.npz')) < LIMIT
    me = f.meta
    assert (f.D, f.E, f.T, me['lens'], f.text_size, me['sn'], me['sratio'], me['norm']) == (32, 64, 200, [200, 139], [2, 1], 8, 0.25, True)
    assert (f.msf, f.scat) == ('nomsf' not in name, 'scat' in name)
    cin = f.D * (2 if f.msf else 1) + int(f.scat)
    assert f.W.shape == (f.E, cin) == f.dw32.shape and f.bias.shape == (f.E,) == f.db32.shape
    assert f.gate.shape == f.mask.shape == (3, f.T) and f.dY.shape == f.y32.shape == (3, f.T, f.E)
    # (the generator compared the gate and the mask of the fp32 run with those of the fp64 run before it wrote either)
    valid = f.vid_masks.repeat_interleave(torch.tensor(f.text_size), 0)
    assert torch.equal(f.mask, valid if f.msf else valid & f.gate) and not bool(f.gate[~valid].any())
    # the two-query video: a tile closed for both queries, a tile kept by exactly one; a gate edge inside a tile
    kept = [[bool(f.gate[q, t0:t0 + R.TILE].any()) for q in (0, 1)] for t0 in range(0, f.T, R.TILE)]
    assert any(not any(k) for k in kept) and any(sum(k) == 1 for k in kept), kept
    assert any(b == 0 for b, _, _ in f.closed_tiles())
    edges = torch.nonzero(f.gate[:, 1:] != f.gate[:, :-1])[:, 1] + 1
    assert bool((edges % R.TILE != 0).any())
    # features and weights lie on the 2^-10 grid; the upstream gradient is not all zero
    for z in (f.vid, f.shallow, f.text_cls, f.W, f.bias):
        assert torch.equal(z * 1024, torch.round(z * 1024))
    assert float(f.dY.abs().max()) > 0
    for k in ('Y', 'dW', 'db'):
        assert f.e_ref[k] <= E_REF_CAP * f.top[k], (name, k, f.e_ref[k], f.top[k])
        assert abs(f.e_ref[k] / f.top[k] - me['e_ref_rel'][k]) <= 1e-9


# ---------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize('name', R.CASES)
def test_shared_formulas_equal_the_dense_formula_and_the_yardstick(name):
    f = R.Fixture(name)
    vid, shallow, gate, mask, correl, sizes, W, bias = f.operands(torch.float64, correl64=True)      # what the yardstick's vid_map saw
    dY = f.dY.double()
    x = R.dense_input(vid, shallow, gate, correl, sizes)
    assert x.shape == (3, f.T, W.size(1))
    y_d, (dw_d, db_d) = R.dense_forward(x, mask, W, bias), R.dense_grads(x, mask, dY)
    y_s, (dw_s, db_s) = R.shared_forward(vid, shallow, gate, mask, correl, sizes, W, bias), R.shared_grads(vid, shallow, gate, mask, correl, sizes, dY)
    for k, a, b, want in (('Y', y_s, y_d, f.y64), ('dW', dw_s, dw_d, f.dw64), ('db', db_s, db_d, f.db64)):
        top = float(b.abs().max())
        assert float((a - b).abs().max()) <= 1e-12 * top, (name, k)
        # the yardstick is stored as x_32 + fp32(x_64 - x_32): exact to 2^-24 of the difference
        assert float((a - want).abs().max()) <= 1e-12 * top + 2.0 ** -23 * f.e_ref[k], (name, k, float((a - want).abs().max()))


def test_restatement_matches_finite_differences():
    """W1, W2, w3 and the bias, on a small problem with two videos, [2, 1] queries, a mask with holes and a live gate"""
    gen = torch.Generator().manual_seed(11)
    nvid, D, T, E, sizes = 2, 4, 9, 3, [2, 1]
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    vid, shallow, correl, dY = r(nvid, D, T), r(nvid, D, T), r(3, T), r(3, T, E)
    gate = (torch.rand(3, T, generator=gen) < 0.5).double()
    mask = torch.rand(3, T, generator=gen) < 0.8
    W, bias = r(E, 2 * D + 1), r(E)
    dw, db = R.shared_grads(vid, shallow, gate, mask, correl, sizes, dY)
    f = lambda w, b: float((R.shared_forward(vid, shallow, gate, mask, correl, sizes, w, b) * dY).sum())
    h = 1e-6
    for e in range(E):
        for c in (0, D - 1, D, 2 * D - 1, 2 * D):          # W1, W2 and w3
            wp, wm = W.clone(), W.clone()
            wp[e, c] += h
            wm[e, c] -= h
            fd = (f(wp, bias) - f(wm, bias)) / (2 * h)
            assert abs(fd - float(dw[e, c])) <= 1e-7 * max(1.0, abs(fd)), (e, c, fd, float(dw[e, c]))
        bp, bm = bias.clone(), bias.clone()
        bp[e] += h
        bm[e] -= h
        fd = (f(W, bp) - f(W, bm)) / (2 * h)
        assert abs(fd - float(db[e])) <= 1e-7 * max(1.0, abs(fd)), (e, fd, float(db[e]))
    # the same through autograd, every element, without the shallow half and without the score channel too
    for sh, co, w in ((shallow, correl, W), (None, correl, W[:, D:].clone()[:, :D + 1]), (shallow, None, W[:, :2 * D].clone()), (None, None, W[:, :D].clone())):
        wa, ba = w.clone().requires_grad_(True), bias.clone().requires_grad_(True)
        (R.shared_forward(vid, sh, gate, mask, co, sizes, wa, ba) * dY).sum().backward()
        dw, db = R.shared_grads(vid, sh, gate, mask, co, sizes, dY)
        assert float((dw - wa.grad).abs().max()) <= 1e-12 and float((db - ba.grad).abs().max()) <= 1e-12


# ---------------------------------------------------------------------------------------------- what training_forward admits
def _model_and_batch(**flags):
    import step_grad_ref as S
    pkg = load_pkg()
    f = S.Fixture('s2')
    opt = pkg.config.make_opt(**dict(f.opt_kwargs, **flags))
    model = pkg.modeling.PtTransformerEarlyFusionIterative(opt, second_fusion=f.second_fusion)
    batch = (f.vid, f.shallow, f.vid_masks, f.tokens.transpose(1, 2).contiguous(), f.text_cls, f.token_masks, f.text_size)
    return pkg, model, batch


def test_a_scat_model_reaches_the_gpu_only_error():
    """before the shared front end, training_forward raised NotImplementedError for opt.model.scat"""
    pkg, model, batch = _model_and_batch(scat=True)
    assert model.scat and model.vid_map.conv.weight.shape[1] == 2 * 32 + 1
    for fe in ('dense', 'shared'):
        with pytest.raises(RuntimeError, match='MI355X only'):
            pkg.train.training_forward(model, *batch, front_end=fe)


def test_sfonly_stays_refused():
    pkg, model, batch = _model_and_batch(sfonly=True)
    with pytest.raises(NotImplementedError, match=r'model\.py:606-612'):
        pkg.train.training_forward(model, *batch)


def test_an_unknown_front_end_is_refused_before_anything_else():
    pkg = load_pkg()
    with pytest.raises(ValueError, match='front_end'):
        pkg.train.training_forward(object(), None, None, None, None, None, None, front_end='nonsense')
    with pytest.raises(ValueError, match='front_end'):
        pkg.train.TrainStep(None, None, front_end='nonsense')
    assert pkg.train.FRONT_ENDS == ('dense', 'shared')


def test_gated_vid_map_refuses_features_that_want_a_gradient_and_the_cpu():
    pkg = load_pkg()
    f = R.Fixture('msf')
    vid, shallow, gate, mask, correl, sizes, W, bias = f.operands(torch.float32)
    with pytest.raises(ValueError, match='requires a gradient'):
        pkg.autograd.gated_vid_map(vid.clone().requires_grad_(True), shallow, gate, mask, correl, sizes, W[:, :, None], bias)
    with pytest.raises(RuntimeError, match='no CPU path'):
        pkg.autograd.gated_vid_map(vid, shallow, gate, mask, correl, sizes, W[:, :, None], bias)
