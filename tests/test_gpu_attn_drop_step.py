"""GPU checks of the training step with the sites of ``model.enable_dropout(sites='all')`` (train.training_forward, TrainStep): attn_pdrop
on the attention maps of the video encoder, the fusion and the text encoder, the text encoder's proj / path dropouts, the fusion's
dropouts again per pyramid level with ``second_fusion=True``, and ``vid_net.cdrop``; on the models and batches of
tests/golden/step_grad_<case>.npz (`s1`: stride 1, no msf, T 40; `s2`: stride 2, msf, T 80, with and without its second fusion).

1. The opt-in alone changes nothing: with the new rates at 0, ``sites='all'`` gives the bits of ``sites='engine'`` under the same key.
2. Plumbing: which sites the forward draws from, recorded at the autograd functions -- text block i at (DROP_G_TEXT, i), decoder layer
   i at (DROP_G_FUSION, i), stem block i at (DROP_G_STEM, i), the block of level l at (DROP_G_BRANCH, l), the second fusion of level l
   at (DROP_G_FUSION2, l * n_layers + i), all at sub DROP_ATTN, the channels at (DROP_G_INPUT, 0, DROP_CHANNEL); one key, b0 = 0, opt's rates.
3. Channel dropout, exactly: cdrop = 0.5 has the keep factors 0 and 2, so on one video with one query the step equals, bit for bit,
   the dropout-free step on features multiplied by those factors (tests/philox_ref.py) beforehand.
4. The whole step against the reference: tests/golden/step_grad_attn_drop_<case>*.npz (make_golden_step_grad_attn_drop.py) is the
   reference's own step in .train() with attn_pdrop 0.1, proj_pdrop 0.2, path_pdrop 0.3 on vid_net, fusion and text_net alike, cdrop 0.1
   and the TCN at 0.5, its draws replaced by the stated stream: `s2a` (`s2` WITH its second fusion) and `s1g` (`s1` with
   mha_win_size = 0 on one head of 32 channels).  With the fixture's key: masks equal, the four outputs at rtol = atol = 2e-4
   (tests/test_gpu_step_grad_drop.py's tolerance for the same quantities), and the gradient of EVERY named parameter under the
   project's rule, one `SGERR` line each.  This is what ties the model-level site numbers and element indices to the reference.
5. On the same cases and key: every parameter takes a gradient, the same key twice gives equal bits, another key other bits, and each
   map dropout moves the result.  One ``TrainStep.step`` with the same seed twice gives equal bits, another seed other bits."""
import pytest
import torch

import attn_drop_ref as AR
import philox_ref as P
import step_grad_drop_ref as D
import step_grad_ref as R
from conftest import load_pkg
from test_gpu_train_step import batch_of, bits_differ, opt_of, state_of

pytestmark = pytest.mark.gpu
KEY = 0x9E3779B97F4A7C15
RATES = dict(attn=0.1, proj=0.2, path=0.3, cdrop=0.1, refine=0.5, text=True)
MODELS = [('s1', False), ('s2', False), ('s2', True)]           # (fixture, second_fusion)
REF_CASES = ('attn_drop_s2a', 'attn_drop_s1g')
_fixtures = {}


@pytest.fixture(scope='module')
def pkg():
    return load_pkg()


def fixture(name):
    if name not in _fixtures:
        _fixtures[name] = R.Fixture(name)
    return _fixtures[name]


def rated_opt(pkg, f, attn=0.0, proj=0.0, path=0.0, cdrop=0.0, text=False, fattn=None, tattn=None, **_):
    """attn / proj / path on vid_net and fusion (`fattn`: the fusion's own map rate), with `text` on text_net too (`tattn` likewise)"""
    opt = opt_of(pkg, f)
    for part in ('vid_net', 'fusion') + (('text_net',) if text else ()):
        opt.model[part]['proj_pdrop'], opt.model[part]['path_pdrop'], opt.model[part]['attn_pdrop'] = proj, path, attn
    if fattn is not None:
        opt.model['fusion']['attn_pdrop'] = fattn
    if tattn is not None:
        opt.model['text_net']['attn_pdrop'] = tattn
    opt.model['vid_net']['cdrop'] = cdrop
    return opt


def rated_model(pkg, f, sites='all', seed=None, refine=0.5, second_fusion=False, **rates):
    model = pkg.modeling.PtTransformerEarlyFusionIterative(rated_opt(pkg, f, **rates), second_fusion=second_fusion)
    model.load_state_dict(f.sd)                           # (the second fusion of `s2` is the first one's modules: no weights of its own)
    model = model.cuda()
    model.enable_dropout(seed=seed, refine_pdrop=refine, sites=sites)
    return model


def stepped(pkg, f, model, key, batch=None, targets=None):
    """training_forward under `key`, the objective, backward() -> (total, {parameter: gradient})"""
    if batch is None:
        batch, targets = batch_of(f)
    out = pkg.train.training_forward(model, **batch, **({} if key is None else {'dropout_seed': key}))
    total = pkg.loss.PointObjective(f.opt(pkg))(out, targets)['total']
    total.backward()
    return total.detach(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}


def same(a, b):
    return torch.equal(a[0], b[0]) and not [k for k in a[1] if not torch.equal(a[1][k].view(torch.int32), b[1][k].view(torch.int32))]


@pytest.mark.parametrize('name', ['s1', 's2'])
def test_the_opt_in_alone_changes_no_bit(pkg, name):
    f = fixture(name)
    runs = [stepped(pkg, f, rated_model(pkg, f, sites=s, proj=0.2, path=0.3), KEY) for s in ('engine', 'all')]
    assert same(*runs)


@pytest.mark.parametrize('name,second', MODELS)
def test_sites_keys_and_rates_the_forward_draws_from(pkg, name, second, monkeypatch):
    f = fixture(name)
    A = pkg.autograd
    model = rated_model(pkg, f, second_fusion=second, **RATES)
    seen = {'map': [], 'cross': [], 'chan': []}
    inner = {k: getattr(A, k).apply for k in ('_WindowAttentionFn', '_CrossAttentionFn', '_ChannelDropoutFn')}

    def map_apply(q, k, v, mask, n_heads, window, drop):       # drop: None, or (key, site, p, b0)
        if drop is not None:
            seen['map'].append(tuple(drop))
        return inner['_WindowAttentionFn'](q, k, v, mask, n_heads, window, drop)

    def cross_apply(q, k, v, mask, n_heads, drop):
        if drop is not None:
            seen['cross'].append(tuple(drop))
        return inner['_CrossAttentionFn'](q, k, v, mask, n_heads, drop)

    def chan_apply(x, key, site, p, b0):
        seen['chan'].append((key, site, p, b0, tuple(x.shape)))
        return inner['_ChannelDropoutFn'](x, key, site, p, b0)

    monkeypatch.setattr(A._WindowAttentionFn, 'apply', staticmethod(map_apply))
    monkeypatch.setattr(A._CrossAttentionFn, 'apply', staticmethod(cross_apply))
    monkeypatch.setattr(A._ChannelDropoutFn, 'apply', staticmethod(chan_apply))
    batch, _ = batch_of(f)
    with torch.no_grad():
        pkg.train.training_forward(model, **batch, dropout_seed=KEY)
    key = A.DropSpec(KEY).key
    n_stem, n_branch, n = len(model.vid_net.stem), len(model.vid_net.branch), len(model.fusion.layers)
    assert not model.vid_net.pool_only
    at = lambda g, i: (key, P.site(g, i, A.DROP_ATTN), RATES['attn'], 0)
    assert seen['map'] == [at(A.DROP_G_STEM, i) for i in range(n_stem)] + [at(A.DROP_G_BRANCH, l) for l in range(n_branch)]
    want = [at(A.DROP_G_TEXT, i) for i in range(len(model.text_net.transformer))] + [at(A.DROP_G_FUSION, i) for i in range(n)]
    if second:
        want += [at(A.DROP_G_FUSION2, l * n + i) for l in range(n_branch) for i in range(n)]
    assert seen['cross'] == want, (seen['cross'], want)
    nq, D, T = sum(f.text_size), f.vid.size(1), f.vid.size(2)
    assert seen['chan'] == [(key, P.site(A.DROP_G_INPUT, 0, A.DROP_CHANNEL), RATES['cdrop'], 0, (nq, T, D * (2 if model.msf else 1)))]
    assert model.last_dropout_seed == KEY


def test_channel_dropout_at_one_half_is_the_step_on_features_scaled_beforehand(pkg):
    f = fixture('s1')
    assert not f.model(pkg).msf, 'without msf the input of vid_map is the gated clip features alone'
    b = f.text_size.index(1)                              # one video with one query: B' = 1, sample 0 of the stream
    batch, targets = batch_of(f, [b])
    dropped = stepped(pkg, f, rated_model(pkg, f, cdrop=0.5, refine=0.0), KEY, batch, targets)
    D = f.vid.size(1)
    keep = AR.channel_keep(KEY, P.site(AR.DROP_G_INPUT, 0, AR.DROP_CHANNEL), 1, D, 0.5)
    assert 0 < int(keep.sum()) < D and float(P.scale(0.5)) == 2.0
    plain = f.model(pkg).cuda()
    scaled = dict(batch, vid=batch['vid'] * (keep.float() * 2.0).cuda()[:, :, None])
    want = stepped(pkg, f, plain, None, scaled, targets)
    assert same(dropped, want)
    assert not same(dropped, stepped(pkg, f, f.model(pkg).cuda(), None, batch, targets)), 'the dropout moves the step'


_runs = {}


def ref_run(pkg, name, key=None, **kw):
    """a fresh model of the fixture's case with the fixture's rates (`kw` overrides), training_forward under `key` (the fixture's),
    the objective, backward() -> (outputs, total, {parameter: gradient})"""
    f = fixture(name)
    m = f.meta
    assert (m['attn_pdrop'], m['proj_pdrop'], m['path_pdrop'], m['cdrop'], m['refine_pdrop']) == tuple(RATES[k] for k in ('attn', 'proj', 'path', 'cdrop', 'refine'))
    model = rated_model(pkg, f, second_fusion=f.second_fusion, **dict(RATES, **kw))
    batch, targets = batch_of(f)
    out = pkg.train.training_forward(model, **batch, dropout_seed=m['seed'] if key is None else key)
    total = pkg.loss.PointObjective(f.opt(pkg))(out, targets)['total']
    total.backward()
    return out, total.detach(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}


def base(pkg, name):
    if name not in _runs:
        _runs[name] = ref_run(pkg, name)
    return _runs[name]


@pytest.mark.parametrize('name', REF_CASES)
def test_every_parameter_gradient_matches_the_reference_step_with_every_site(pkg, name):
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


@pytest.mark.parametrize('name', REF_CASES)
def test_the_whole_step_with_every_site(pkg, name):
    """the key is the fixture's: picked on the CPU by the generator so that no drop-path site drops every row and, in the reference,
    every parameter takes a gradient"""
    _, t0, g0 = base(pkg, name)
    silent = [k for k, g in g0.items() if not bool(g.any())]
    assert not silent, f'parameters without a gradient: {silent}'
    _, t1, g1 = ref_run(pkg, name)
    assert same((t0, g0), (t1, g1))
    _, t2, g2 = ref_run(pkg, name, key=fixture(name).meta['seed'] + 1)
    assert not torch.equal(t0, t2) and sum(not torch.equal(g0[k], g2[k]) for k in g0) > len(g0) // 2
    # each map dropout moves the step: the video encoder's (with it the others'), the fusion's alone, the text encoder's alone
    for kw in (dict(attn=0.0), dict(fattn=0.0), dict(tattn=0.0)):
        assert not torch.equal(t0, ref_run(pkg, name, **kw)[1]), kw


def test_train_step_is_reproducible_from_its_seed(pkg):
    f = fixture('s1')
    batch, targets = batch_of(f)

    def train_step(seed):
        opt = rated_opt(pkg, f, **RATES)
        opt.train.warmup_epochs = 0
        return pkg.train.TrainStep(rated_model(pkg, f, seed=seed, **RATES), opt, itrs_per_epoch=1)

    a, b, c = train_step(11), train_step(11), train_step(12)
    for ts in (a, b, c):
        out = ts.step(batch, targets)
        assert all(bool(torch.isfinite(out[n]).all()) for n in ('cls', 'reg', 'total', 'grad_norm'))
    assert a.model.last_dropout_seed == b.model.last_dropout_seed != c.model.last_dropout_seed
    assert not bits_differ(state_of(a), state_of(b)) and bits_differ(state_of(a), state_of(c))
