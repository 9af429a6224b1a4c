"""CPU checks that go with the attention-gradient extension (include/decafnet_hip_attn.h; its header and table:
tests/test_abi_headers.py): the names of ``_lib.ATTN_SIGNATURES``; the fp64 restatement of the global attention backward
(tests/global_attn_grad_ref.py) matches the reference's own fp64 `backward()` (tests/golden/global_attn_grad.npz) and central finite
differences, and obeys the conventions of the header; the fixture is what its generator says it is.  No GPU."""
import os

import pytest
import torch

from conftest import Golden, load_pkg
import global_attn_grad_ref as R

F_SHAPES = [s[0] for s in R.SHAPES if s[7]]


def test_attn_table_names():
    assert sorted(load_pkg()._lib.ATTN_SIGNATURES) == ['dcf_attn_ext_version', 'dcf_op_global_attn_bwd']


# ---------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize('name', F_SHAPES)
def test_restatement_matches_the_reference_in_fp64(name):
    f = R.OpFixture(name)
    g = R.grads(f.q.double(), f.k.double(), f.v.double(), f.mask, f.do.double(), f.heads)
    for key, mine in zip(('dq', 'dk', 'dv'), g):
        err, top = float((f.at_rows(mine) - f.g64[key]).abs().max()), f.top[key]
        assert err <= 1e-12 * top, (name, key, err, top)
        # the fp32 evaluation of the restatement errs like the reference's fp32 backward: within a factor of 4 either way
        e32 = float((R.grads(f.q, f.k, f.v, f.mask, f.do, f.heads)['dq dk dv'.split().index(key)].double() - mine).abs().max())
        assert e32 <= 4 * f.e_ref[key] and f.e_ref[key] <= 4 * e32, (name, key, e32, f.e_ref[key])
    assert len(f.rows) == f.B * f.T or name != 'below_tile'


def test_fixture_operands_are_exact_in_fp32():
    """x, up and the parameters lie on the grid the generator describes: the projections are the same numbers in fp32 and fp64"""
    for name in F_SHAPES:
        f = R.OpFixture(name)
        for n, z in (('query', f.q), ('key', f.k), ('value', f.v)):
            exact = f.x.double() @ f.sd[f'{n}.weight'][:, :, 0].double().t() + f.sd[f'{n}.bias'].double()
            assert torch.equal(z.double(), exact), (name, n)
        assert torch.equal(f.do.double(), f.up.double() @ f.sd['proj.weight'][:, :, 0].double()), name
        assert set(f.g64) >= {'dq', 'dk', 'dv'} and all(f.e_ref[k] > 0 for k in ('dq', 'dk', 'dv'))
        assert (len(f.gp64) == 8) == (name == 'below_tile') and {k for k in f.gp64 if k.endswith('bias')} == {f'{n}.bias' for n in ('query', 'key', 'value', 'proj')}


def test_restatement_matches_finite_differences():
    B, T, C, heads = 2, 7, 64, 2
    gen = torch.Generator().manual_seed(7)
    q, k, v, do = (torch.randn(B, T, C, generator=gen, dtype=torch.float64) for _ in range(4))
    mask = torch.ones(B, T, dtype=torch.bool)
    mask[1, 2] = mask[1, 5] = mask[1, 6] = False
    g = R.grads(q, k, v, mask, do, heads)
    f = lambda a, b, c: float((R.forward(a, b, c, mask, heads) * do).sum())
    h = 1e-5
    pick = torch.Generator().manual_seed(8)
    for i, (name, x) in enumerate((('dq', q), ('dk', k), ('dv', v))):
        for _ in range(12):
            b, t, c = int(torch.randint(B, (1,), generator=pick)), int(torch.randint(T, (1,), generator=pick)), int(torch.randint(C, (1,), generator=pick))
            xp, xm = x.clone(), x.clone()
            xp[b, t, c] += h
            xm[b, t, c] -= h
            ops = lambda z: [z if j == i else w for j, w in enumerate((q, k, v))]
            fd = (f(*ops(xp)) - f(*ops(xm))) / (2 * h)
            assert abs(fd - float(g[i][b, t, c])) <= 1e-8 * max(1.0, abs(fd)), (name, b, t, c, fd, float(g[i][b, t, c]))
    # the same through autograd, every element
    qa, ka, va = (z.clone().requires_grad_(True) for z in (q, k, v))
    (R.forward(qa, ka, va, mask, heads) * do).sum().backward()
    for mine, z in zip(g, (qa, ka, va)):
        assert float((mine - z.grad).abs().max()) <= 1e-13


def test_conventions():
    """a padded key gives exactly 0; a padded query row is live; a sequence with no valid key gives zeros"""
    q, k, v, do, mask, heads = R.shape_case('no_valid_key', torch.float64)
    mask[0, 30:] = False
    mask[0, 7] = False
    o = R.forward(q, k, v, mask, heads)
    dq, dk, dv = R.grads(q, k, v, mask, do, heads)
    assert bool((dk[~mask] == 0).all()) and bool((dv[~mask] == 0).all())
    assert bool((o[0, 30:].abs().amax(-1) > 0).all()) and bool((dq[0, 30:].abs().amax(-1) > 0).all()) and float(dq[0, 7].abs().max()) > 0
    do2 = do.clone()
    do2[0, 35] += 1.0                                        # dO at a padded query row reaches dK and dV of the valid keys
    _, dk2, dv2 = R.grads(q, k, v, mask, do2, heads)
    assert float((dk2[0, :30] - dk[0, :30]).abs().max()) > 0 and float((dv2[0, :30] - dv[0, :30]).abs().max()) > 0
    for z in (o[1], dq[1], dk[1], dv[1]):
        assert bool((z == 0).all())
    # the output does not depend on what a padded key or value holds
    k2, v2 = k.clone(), v.clone()
    k2[~mask], v2[~mask] = 1e6, -1e6
    assert torch.equal(R.forward(q, k2, v2, mask, heads), o)


# ---------------------------------------------------------------------------------------------- the block cases of the fixture
def test_block_cases_of_the_fixture():
    g = Golden('global_attn_grad.npz')
    meta = g.js('meta')
    assert meta['shapes'] == F_SHAPES and meta['enc_cases'] == {'s1': 1, 's2': 2}
    enc = meta['enc']
    sd = g.sub('enc/param/')
    assert len([k for k in sd]) == 27 and enc['E'] // enc['heads'] == 32
    for name, stride in meta['enc_cases'].items():
        pre = f'enc/{name}/'
        x, mask, up = g.t(pre + 'x'), g.t(pre + 'mask'), g.t(pre + 'up')
        assert x.shape == (enc['B'], enc['E'], enc['Ta'] * stride) and up.shape == (enc['B'], enc['E'], enc['Ta'])
        assert torch.equal(g.t(pre + 'mask_out'), mask[:, ::stride]) and not bool(up.transpose(1, 2)[~mask[:, ::stride]].any())
        assert int((~mask[1, :enc['lens'][1] * stride:stride]).sum()) == len(enc['holes'])
        gp = g.sub(pre + 'gp/')
        assert len(gp) == 2 * 27
        for k in sd:
            g32, d = gp[f'{k}/32'], gp[f'{k}/d']
            assert g32.shape == sd[k].shape and float(g32.abs().max()) > 0, k
            if not k.endswith(('key.bias', 'k_norm.bias')):           # zero in exact arithmetic
                assert float(d.abs().max()) <= 2.0 ** -15 * float(g32.abs().max()), (name, k)


# ---------------------------------------------------------------------------------------------- case g1 of the whole step
def test_step_case_g1_meets_the_conditions_on_the_reference():
    """the conditions profiles/step_grad.md lists for s1 / s2, by the same code (tests/test_step_grad_cpu.py), on the committed files:
    the precisions agree on gate, masks and labels; every parameter takes a gradient; no positive point sits on a non-smooth point of
    the IoU loss; e_ref <= 2^-15 max |g64| for every parameter that is not zero in exact arithmetic"""
    import global_step_fixture as G
    import test_step_grad_cpu as SC
    f = G.fixture()
    assert len(G.files()) == 1 + len(G.param_files()) + len(f.meta['parts'])
    for path in G.files():
        assert 0 < os.path.getsize(path) < SC.LIMIT, path
    kw = f.opt_kwargs
    assert (kw['E'], kw['n_heads'], kw['win'], kw['n_levels'], kw['vid_stride'], kw['msf']) == (64, 2, 0, 3, 1, False)
    assert f.meta['T'] == 80 and f.meta['lens'] == [80, 55] and f.text_size == [2, 1] and f.tokens.size(0) == 3 and not f.second_fusion
    model = f.model(load_pkg())
    names = [k for k, _ in model.named_parameters()]
    assert len(names) == f.meta['n_params'] and sorted(names) == sorted(f.gp['32']) == sorted(f.gp['64'])
    for k, p in model.named_parameters():
        assert f.gp['32'][k].shape == f.gp['64'][k].shape == p.shape and torch.equal(p.detach(), f.sd[k]), k
    assert all(b.attn.attn.window_size == 0 and b.attn.attn.n_heads == 2 for b in list(model.vid_net.stem) + list(model.vid_net.branch))
    SC.test_reference_error_is_under_the_cap(f)
    SC.test_discrete_decisions(f)
    SC.test_positive_points(f)
    SC.test_total_is_the_objective_of_the_recorded_outputs(f)
