"""GPU checks of the training step WITH dropout and drop-path (train.training_forward after model.enable_dropout, TrainStep):

1. Gradients against the reference: tests/golden/step_grad_drop_<case>*.npz (make_golden_step_grad_drop.py) is the reference's own
   step in .train() with proj_pdrop 0.2, path_pdrop 0.3 and the TCN's 0.5, its draws replaced by the stated stream.  With the
   fixture's key, outputs at rtol = atol = 2e-4 (tests/test_gpu_dropout.py's tolerance for the same quantities), masks equal, and the
   gradient of EVERY named parameter under the project's rule (tests/test_gpu_step_grad.py), one `SGERR` line each.
2. The forward against the engine's fixture: the `e64` and `e256` cases of tests/golden/train_dropout.npz.
3. The same key twice gives equal bits, another key other bits; enable_dropout() + disable_dropout() is a model that never had it.
4. TrainStep with the reference's default rates (0.1): two steps, one key per forward, reproducible from the seed, resumable
   through state() / load_state() ('dropout_rng')."""
import pytest
import torch

from conftest import Golden, load_pkg
import dec_grad_ref as DR
import step_grad_drop_ref as D
import step_grad_ref as R
from test_gpu_train_step import batch_of, bits_differ, opt_of, state_of

pytestmark = pytest.mark.gpu
CASES = ('drop_s1d', 'drop_s2d')
_fixtures, _runs = {}, {}


@pytest.fixture(scope='module')
def pkg():
    return load_pkg()


def fixture(name):
    if name not in _fixtures:
        _fixtures[name] = R.Fixture(name)
    return _fixtures[name]


def drop_opt(pkg, f, proj, path):
    opt = opt_of(pkg, f)
    for part in ('vid_net', 'fusion'):
        opt.model[part]['proj_pdrop'], opt.model[part]['path_pdrop'] = proj, path
    return opt


def drop_model(pkg, f, proj=None, path=None, **enable):
    proj, path = f.meta.get('proj_pdrop', 0.1) if proj is None else proj, f.meta.get('path_pdrop', 0.1) if path is None else path
    model = pkg.modeling.PtTransformerEarlyFusionIterative(drop_opt(pkg, f, proj, path), second_fusion=False)
    model.load_state_dict(f.sd)
    model = model.cuda()
    model.enable_dropout(**enable)
    return model


def stepped(pkg, name, key):
    """a fresh model of the case, training_forward under `key`, the objective, backward() -> (outputs, total, {parameter: gradient})"""
    f = fixture(name)
    model = drop_model(pkg, f, refine_pdrop=f.meta['refine_pdrop'])
    batch, targets = batch_of(f)
    out = pkg.train.training_forward(model, **batch, dropout_seed=key)
    assert model.last_dropout_seed == key
    total = pkg.loss.PointObjective(f.opt(pkg))(out, targets)['total']
    total.backward()
    return out, total.detach(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}


def base(pkg, name):
    if name not in _runs:
        _runs[name] = stepped(pkg, name, fixture(name).meta['seed'])
    return _runs[name]


@pytest.mark.parametrize('name', CASES)
def test_every_parameter_gradient_matches_the_reference_step_with_dropout(pkg, name):
    f = fixture(name)
    (l1, l2, off, masks), total, gp = base(pkg, name)
    for l in range(f.L):
        assert torch.equal(masks[l].cpu(), f.masks[l]), f'mask of level {l}'
    for key, outs in (('logits1', l1), ('logits2', l2), ('offsets', off)):
        for l in range(f.L):
            torch.testing.assert_close(outs[l].detach().cpu(), f.out['32'][key][l].reshape(outs[l].shape), rtol=2e-4, atol=2e-4, msg=f'{key}/l{l}')
    torch.testing.assert_close(total.cpu(), f.total['32'], rtol=2e-4, atol=2e-4)
    missed = [D.check('SGERR', f'{name} {k}', gp[k], f.gp['64'][k], f.gp['32'][k], top=f.top(k)) for k in gp]
    assert len(gp) == f.meta['n_params'] == len(f.gp['64'])
    missed = [m for m in missed if m is not None]
    assert not missed, missed


@pytest.mark.parametrize('case', ['e64', 'e256'])
def test_training_forward_gives_the_engine_fixture(pkg, case):
    """the reference's forward with the stated masks that tests/test_gpu_dropout.py checks the engine against, through
    training_forward: the fixture's four outputs at that test's tolerance.

    `e64` has a text encoder of 4 heads on 32 channels: heads of 8 channels, which autograd.xattn_mha runs as padded heads of 16."""
    g = Golden('train_dropout.npz')
    meta, kw = g.js(f'{case}/meta'), g.js(f'{case}/opt_kwargs')
    opt = pkg.config.make_opt(**kw)
    for part in ('vid_net', 'fusion'):
        opt.model[part]['proj_pdrop'], opt.model[part]['path_pdrop'] = meta['proj_pdrop'], meta['path_pdrop']
    model = pkg.modeling.PtTransformerEarlyFusionIterative(opt, second_fusion=False)
    model.load_state_dict(pkg.synth.make_state_dict(g.js(f'{case}/shapes'), meta['wseed']))
    model = model.cuda()
    model.enable_dropout(refine_pdrop=meta['refine_pdrop'])
    c = lambda k: g.t(f'{case}/{k}').cuda().contiguous()
    with torch.no_grad():
        out = pkg.train.training_forward(model, c('vid'), c('shallow'), c('vid_masks'), c('tokens'), c('text_cls'), c('token_masks'),
                                         text_size=meta['sizes'], dropout_seed=meta['seed'])
    for part, key in zip(out, ('logits1', 'logits2', 'offsets', 'masks')):
        for l, x in enumerate(part):
            want = g.t(f'{case}/{key}/l{l}')
            if key == 'masks':
                assert torch.equal(x.cpu().reshape(want.shape), want), f'{key}/l{l}'
            else:
                torch.testing.assert_close(x.cpu().reshape(want.shape), want, rtol=2e-4, atol=2e-4, msg=f'{key}/l{l}')


def test_same_key_same_bits_other_key_other_bits(pkg):
    f = fixture('drop_s1d')
    _, t0, g0 = base(pkg, 'drop_s1d')
    _, t1, g1 = stepped(pkg, 'drop_s1d', f.meta['seed'])
    assert torch.equal(t0, t1) and not [k for k in g0 if not torch.equal(g0[k].view(torch.int32), g1[k].view(torch.int32))]
    _, t2, g2 = stepped(pkg, 'drop_s1d', f.meta['seed'] + 1)
    assert not torch.equal(t0, t2) and sum(not torch.equal(g0[k], g2[k]) for k in g0) > len(g0) // 2


def test_disable_dropout_gives_the_bits_of_a_model_that_never_had_it(pkg):
    f = R.Fixture('s1')
    batch, targets = batch_of(f)
    runs = []
    for toggled in (False, True):
        model = f.model(pkg).cuda()
        if toggled:
            model.enable_dropout(seed=3)
            model.disable_dropout()
        d = pkg.loss.PointObjective(f.opt(pkg))(pkg.train.training_forward(model, **batch), targets)
        d['total'].backward()
        runs.append((d['total'].detach(), [p.grad.clone() for p in model.parameters()]))
    assert torch.equal(runs[0][0], runs[1][0]) and all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))


def test_arguments_that_are_refused(pkg):
    f = fixture('drop_s1d')
    batch, _ = batch_of(f)
    model = drop_model(pkg, f)
    with pytest.raises(ValueError, match='dropout'):
        pkg.train.training_forward(model, **batch, dropout=(1, 0.5, 0))
    model.disable_dropout()
    with pytest.raises(NotImplementedError, match='proj_pdrop'):                     # opt's rates without enable_dropout: as before
        pkg.train.training_forward(model, **batch)
    plain = R.Fixture('s1').model(pkg).cuda()
    with pytest.raises(ValueError, match='dropout_seed'):
        pkg.train.training_forward(plain, **batch, dropout_seed=5)
    second = pkg.modeling.PtTransformerEarlyFusionIterative(drop_opt(pkg, f, 0.1, 0.1), second_fusion=True).cuda()
    second.enable_dropout()
    with pytest.raises(NotImplementedError, match='second_fusion'):
        pkg.train.training_forward(second, **batch)


def train_step(pkg, f, seed):
    model = drop_model(pkg, f, 0.1, 0.1, seed=seed)                  # the reference's default rates
    opt = drop_opt(pkg, f, 0.1, 0.1)
    opt.train.warmup_epochs = 0
    return pkg.train.TrainStep(model, opt, itrs_per_epoch=1)


def test_train_step_with_dropout(pkg):
    f = R.Fixture('s1')
    batch, targets = batch_of(f)
    a, b = train_step(pkg, f, 11), train_step(pkg, f, 11)
    keys, after_first = [], None
    for k in range(2):
        out = a.step(batch, targets)
        assert all(bool(torch.isfinite(out[n]).all()) for n in ('cls', 'reg', 'total', 'grad_norm'))
        keys.append(a.model.last_dropout_seed)
        if k == 0:
            after_first = a.state()
    assert keys[0] != keys[1] and all(0 <= s < 1 << 64 for s in keys)
    for _ in range(2):
        b.step(batch, targets)
    assert b.model.last_dropout_seed == keys[1] and not bits_differ(state_of(a), state_of(b))
    # resume: the state after the first step, loaded into a TrainStep whose model was seeded differently, gives the second step's bits
    assert 'dropout_rng' in after_first[1]
    c = train_step(pkg, f, 0).load_state(*after_first)
    c.step(batch, targets)
    assert c.model.last_dropout_seed == keys[1] and not bits_differ(state_of(c), state_of(a))
    # two micro-batches draw two keys
    d = train_step(pkg, f, 11)
    parts = [batch_of(f, [0]), batch_of(f, [1])]
    seen, inner = [], pkg.train.training_forward

    def spy(model, *args, **kw):
        out = inner(model, *args, **kw)
        seen.append(model.last_dropout_seed)
        return out

    pkg.train.training_forward = spy
    try:
        d.step([p for p, _ in parts], [t for _, t in parts])
    finally:
        pkg.train.training_forward = inner
    assert len(seen) == 2 and seen[0] == keys[0] and seen[1] == keys[1]
    # a model without enable_dropout keeps its checkpoint keys
    plain = pkg.train.TrainStep(f.model(pkg).cuda(), opt_of(pkg, f), itrs_per_epoch=1)
    assert 'dropout_rng' not in plain.state()[1]
    unseeded = drop_model(pkg, f, 0.1, 0.1)                          # enable_dropout() without an int seed: torch's default generator
    assert 'dropout_rng' not in pkg.train.TrainStep(unseeded, drop_opt(pkg, f, 0.1, 0.1), itrs_per_epoch=1).state()[1]


def test_heads_of_eight_channels_meet_the_rule(pkg):
    """the global attention of xattn_mha at head dimension 8 (the text encoder of `e64`), which runs as zero-padded heads of 16 with q and k
    scaled by 2^1/4: output, dQ, dK and dV against tests/dec_grad_ref.py's restatement in fp64 / fp32 under the gradient rule; masked keys
    take an exact zero"""
    A = pkg.autograd
    B, T, Lk, C, heads = 3, 10, 7, 32, 4
    g = torch.Generator().manual_seed(17)
    q, k, v, up = (torch.randn(B, n, C, generator=g) for n in (T, Lk, Lk, T))
    mask = DR.holes(B, Lk, g)
    ref = {}
    for tag, dt in (('64', torch.float64), ('32', torch.float32)):
        qq, kk, vv = (z.to(dt).clone().requires_grad_() for z in (q, k, v))
        o = DR.cross_attention(qq, kk, vv, mask, heads)
        (o * up.to(dt)).sum().backward()
        ref[tag] = (o.detach(), qq.grad, kk.grad, vv.grad)
    qq, kk, vv = (z.cuda().requires_grad_() for z in (q, k, v))
    o = A._narrow_head_attention(qq, kk, vv, mask.cuda(), heads)
    (o * up.cuda()).sum().backward()
    got = (o, qq.grad, kk.grad, vv.grad)
    missed = [D.check('SGERR', f'heads of 8 {n}', a, b, c) for n, a, b, c in zip(('O', 'dQ', 'dK', 'dV'), got, ref['64'], ref['32'])]
    assert not [m for m in missed if m], missed
    assert bool((kk.grad.cpu()[~mask] == 0).all()) and bool((vv.grad.cpu()[~mask] == 0).all())
    assert A._global_attention_limit(65, 32, 4) and A._global_attention_limit(64, 32, 4) is None and A._global_attention_limit(7, 24, 6)
    # the block function keeps its stated limit unless asked; the text encoder asks
    block = pkg.modeling.TransformerEncoder(32, 0, 4, 0).cuda()
    z = torch.randn(2, 9, 32, generator=g).cuda()
    with pytest.raises(ValueError, match='head dimension'):
        A.transformer_encoder(z, None, block)
    y, _ = A.transformer_encoder(z, None, block, narrow_heads=True)
    assert y.shape == z.shape and bool(torch.isfinite(y).all())
