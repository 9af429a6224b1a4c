"""GPU check of a WHOLE training step: the gate, vid_map, the text encoder, the first fusion, the video encoder, fuse_and_predict (with
the second fusion in case `s2`) and the Trainer's objective, composed from the package's own pieces by step_grad_ref.run_step and
differentiated by autograd, against the reference's own `backward()` of the same step (tests/golden/step_grad_<case>*.npz,
make_golden_step_grad.py).  The per-stage files check each stage on its own; this one checks the seams between them: the mask layouts
handed from stage to stage, the repeat by text_size, the gradients of tensors with more than one consumer (the text feeds 1 + n_levels
fusion calls, the fusion parameters are used as often, the heads are shared by the levels), the pooled masks of the levels.

The yardstick is the project's gradient rule (tests/test_gpu_dec_grad.py), unchanged, per tensor:

    e_gpu <= max(4 * e_ref, 2^-21 * max |g_64|),   e = max |g - g_64|

g_64 the reference's fp64 step, e_ref the error of its fp32 step.  For key.bias / k_norm.bias, zero in exact arithmetic, max |g_64| is
that of the same layer's weight (step_grad_ref.Fixture.top).  Every check prints an `SGERR` line; the figures are in
profiles/step_grad.md.

Cases (both E = 32, 3 levels, two videos, three queries, text_size [2, 1]): `s2` stride 2, msf, second fusion, T = 80 (lengths 80 / 55),
'radius' + DIoU; `s1` stride 1, no msf (the gate leaves holes in the mask of every stage), no second fusion, T = 40 (lengths 40 / 27),
'none' + GIoU."""
import pytest
import torch

from conftest import load_pkg
import step_grad_ref as R

pytestmark = pytest.mark.gpu
FLOOR = 2.0 ** -21


def check(tag, got, g64, g32, top=None):
    got, g64, g32 = got.detach().cpu().double(), g64.detach().double(), g32.detach().double()
    assert got.shape == g64.shape == g32.shape, (tag, got.shape, g64.shape, g32.shape)
    assert bool(torch.isfinite(got).all()), tag
    top = float(g64.abs().max()) if top is None else top
    e_ref, e_gpu = float((g32 - g64).abs().max()), float((got - g64).abs().max())
    bound = max(4 * e_ref, FLOOR * top)
    ok = e_gpu <= bound
    print(f'SGERR {tag}: max|g64| {top:.3e} e_ref {e_ref:.3e} e_gpu {e_gpu:.3e} bound {bound:.3e} ratio {e_gpu / bound if bound else 0.0:.3f}'
          f'{"" if ok else "  MISSED"}')
    return None if ok else (tag, e_gpu, bound)


@pytest.fixture(scope='module')
def pkg():
    return load_pkg()


_fixtures, _base = {}, {}


def fixture(name):
    if name not in _fixtures:
        _fixtures[name] = R.Fixture(name)
    return _fixtures[name]


def grads_of(model):
    return {k: None if p.grad is None else p.grad.detach().clone() for k, p in model.named_parameters()}


def stepped(pkg, name, scale=None, freeze=(), text_use=None, model=None):
    """a fresh model of case `name` (or `model`), one step and its backward() -> (model, the step, {parameter: gradient})"""
    f = fixture(name)
    if model is None:
        model = f.model(pkg).cuda()
        for k, p in model.named_parameters():
            if k.startswith(tuple(freeze)):
                p.requires_grad_(False)
    s = R.run_step(pkg, model, f, text_use=text_use)
    (s.total if scale is None else s.total * scale).backward()
    return model, s, grads_of(model)


def base(pkg, name):
    """the plain step of case `name`, run once per process: what the bit-for-bit tests compare with"""
    if name not in _base:
        _base[name] = stepped(pkg, name)
    return _base[name]


def same_bits(a, b, keys=None):
    bad = [k for k in (a if keys is None else keys) if (a[k] is None) != (b[k] is None) or (a[k] is not None and not torch.equal(a[k], b[k]))]
    return bad


@pytest.mark.parametrize('name', R.CASES)
def test_every_parameter_gradient_matches_the_reference_step(pkg, name):
    """outputs, masks, the total, the forward taps (to localise a failure: the first tap that departs names the stage), the gradients
    at the text-encoder output and at the first-fusion output, and the gradient of EVERY named parameter, vid_map.* included"""
    f = fixture(name)
    model, s, gp = base(pkg, name)
    l1, l2, off, masks = s.outputs
    missed = []
    for l in range(f.L):
        assert torch.equal(masks[l].cpu(), f.masks[l]), f'mask of level {l}'
    for k in R.TAPS + tuple(f'fpn{l}' for l in range(f.L)):
        missed.append(check(f'{name} tap/{k}', s.taps[k], f.taps['64'][k], f.taps['32'][k]))
    for key, outs in (('logits1', l1), ('logits2', l2), ('offsets', off)):
        for l in range(f.L):
            missed.append(check(f'{name} {key}/l{l}', outs[l], f.out['64'][key][l], f.out['32'][key][l]))
    missed.append(check(f'{name} total', s.total, f.total['64'], f.total['32']))
    for k in R.GTAPS:
        assert s.taps[k].grad is not None, k
        missed.append(check(f'{name} d tap/{k}', s.taps[k].grad, f.gtaps['64'][k], f.gtaps['32'][k]))
    seen = 0
    for k, p in model.named_parameters():
        assert gp[k] is not None, k
        missed.append(check(f'{name} {k}', gp[k], f.gp['64'][k], f.gp['32'][k], top=f.top(k)))
        seen += 1
    assert seen == len(list(model.parameters())) == f.meta['n_params'] == len(f.gp['64'])
    missed = [m for m in missed if m is not None]
    assert not missed, missed


@pytest.mark.parametrize('name', R.CASES)
def test_two_fresh_runs_give_the_same_bits(pkg, name):
    _, s0, g0 = base(pkg, name)
    _, s1, g1 = stepped(pkg, name)
    assert torch.equal(s0.total, s1.total)
    assert not same_bits(g0, g1)


@pytest.mark.parametrize('name', R.CASES)
def test_power_of_two_scaling_and_accumulation(pkg, name):
    """total * 256 gives every gradient times 256, bit for bit; backward() on two steps without zeroing gives exactly twice one step"""
    _, _, g0 = base(pkg, name)
    model, _, g256 = stepped(pkg, name, scale=256.0)
    assert not same_bits({k: v * 256.0 for k, v in g0.items()}, g256)
    for p in model.parameters():
        p.grad = None
    _, _, g1 = stepped(pkg, name, model=model)
    assert not same_bits(g0, g1)
    _, _, g2 = stepped(pkg, name, model=model)
    assert not same_bits({k: v * 2.0 for k, v in g0.items()}, g2)


@pytest.mark.parametrize('name,frozen', [('s2', 'text_net.'), ('s2', 'vid_map.'), ('s1', 'text_net.'), ('s1', 'vid_map.')])
def test_freezing_a_module_leaves_the_other_gradients_their_bits(pkg, name, frozen):
    _, _, g0 = base(pkg, name)
    _, _, g1 = stepped(pkg, name, freeze=(frozen,))
    cold = [k for k in g0 if k.startswith(frozen)]
    assert cold and all(g1[k] is None for k in cold)
    assert not same_bits(g0, g1, [k for k in g0 if not k.startswith(frozen)])


def test_each_use_of_the_shared_text_counts(pkg):
    """case `s2`: the text feeds the first fusion and the second fusion of every level.  (a) With the text detached at the first fusion
    alone every gradient of text_net changes and text_net still takes the gradient of the second fusion's uses; every other gradient
    keeps its bits: the heads, the refinement and vid_net lie behind every use, and a detached operand cuts only the path INTO the text
    -- the fusion's own parameters (ln_xattn_kv, key, value included) and vid_map take their gradients from the values and from the
    upstream gradient, which are the same.  (b) The gradient at the text output is the sum of what the 1 + n_levels uses deliver, each
    taken from the package's own graph with torch.autograd.grad, none of them zero, and that sum meets the rule against the recorded
    gradient."""
    name = 's2'
    f = fixture(name)
    _, _, g0 = base(pkg, name)
    _, _, g1 = stepped(pkg, name, text_use=lambda i, t: t.detach() if i == 0 else t)
    others = [k for k in g0 if not k.startswith('text_net.')]
    assert any(k.startswith('refine.') for k in others) and not same_bits(g0, g1, others)
    for k in g0:
        if k.startswith('text_net.') and not k.endswith(R.ZERO_BY_SYMMETRY):
            assert g1[k] is not None and float(g1[k].abs().max()) > 0, k
            assert not torch.equal(g0[k], g1[k]), f'{k}: the first fusion\'s use of the text does not reach it'
    # (b)
    uses = []

    def alias(i, t):
        uses.append(t.view_as(t))
        return uses[-1]

    model = f.model(pkg).cuda()
    s = R.run_step(pkg, model, f, text_use=alias)
    assert len(uses) == 1 + f.L
    parts = torch.autograd.grad(s.total, uses, retain_graph=True)
    s.total.backward()
    whole = s.taps['text'].grad
    top = float(f.gtaps['64']['text'].abs().max())
    for i, part in enumerate(parts):
        share = float(part.abs().max())
        print(f'SGERR {name} d tap/text, use {i}: max |g| {share:.3e}')
        assert share > 0, f'use {i} of the text delivers nothing'
    total = sum(p.double() for p in parts)
    missed = [check(f'{name} d tap/text, sum of the {len(parts)} uses', total, f.gtaps['64']['text'], f.gtaps['32']['text']),
              check(f'{name} d tap/text, accumulated', whole, f.gtaps['64']['text'], f.gtaps['32']['text'])]
    assert float((whole.double() - total).abs().max()) <= 2.0 ** -21 * top, 'the accumulated gradient is not the sum of the uses'
    assert not [m for m in missed if m is not None], missed
