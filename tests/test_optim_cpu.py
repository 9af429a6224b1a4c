"""CPU checks of the training update's host side (cvpr2025-decafnet_amd/optim.py) against what the reference's own factories produced
(tests/golden/optim_ref.npz, make_golden_optim.py): the decay / no-decay parameter groups, the learning-rate sequences of the two
warm-up schedulers, the state-dict exchange with torch.optim.AdamW, the refusals, and the three new exports.  No GPU, no kernel runs."""
import copy
import warnings

import pytest
import torch

from conftest import Golden, load_pkg

G = Golden('optim_ref.npz')
GROUPS, SCHED = G.js('groups'), G.js('sched')


@pytest.fixture(scope='module')
def pkg():
    return load_pkg()


def model_of(pkg, name):
    if name == 'default':
        return pkg.modeling.create_model(pkg.config.make_opt())
    g = Golden(f'{name}.npz')
    return pkg.modeling.PtTransformerEarlyFusionIterative(pkg.config.make_opt(**g.js('opt_kwargs')), second_fusion=g.js('meta')['second_fusion'])


@pytest.mark.parametrize('name', sorted(GROUPS))
def test_parameter_groups_are_the_reference_s(pkg, name):
    want = GROUPS[name]
    assert want['weight_decay'] == [0.05, 0.0]
    model = model_of(pkg, name)
    decay, no_decay = pkg.optim.split_decay(model)
    assert decay == want['decay'] and no_decay == want['no_decay']
    opt = pkg.optim.make_optimizer(model, pkg.config.make_opt().optimizer)
    assert isinstance(opt, pkg.optim.AdamW) and isinstance(opt, torch.optim.Optimizer)
    named = dict(model.named_parameters())
    assert [g['weight_decay'] for g in opt.param_groups] == [0.05, 0.0]
    assert [g['lr'] for g in opt.param_groups] == [1e-3, 1e-3]
    for group, names in zip(opt.param_groups, (want['decay'], want['no_decay'])):
        assert len(group['params']) == len(names) and all(p is named[n] for p, n in zip(group['params'], names))
    if name == 'default':
        assert len(named) == 449 and sum(p.numel() for p in named.values()) == 14512236


def test_config_carries_the_reference_defaults(pkg):
    opt = pkg.config.make_opt()
    assert dict(opt.optimizer) == dict(name='adamw', lr=1e-3, weight_decay=0.05, clip_grad_norm=1.0)
    assert dict(opt.scheduler) == dict(name='multistep', steps=(-1,), gamma=0.1, epochs=5, warmup_epochs=5)
    ts_keys = {'epochs', 'warmup_epochs', 'ema_beta'}
    assert not ts_keys & set(opt.train), 'opt.train keeps its keys (tests/test_objective_cpu.py); TrainStep reads these with defaults'


@pytest.mark.parametrize('name', sorted(SCHED))
def test_learning_rate_sequence_is_the_reference_s(pkg, name):
    """double-precision host arithmetic on both sides: 1e-12 relative, exact where the recorded value is 0"""
    c = dict(SCHED[name])
    want, lr, n = G.t(f'lr/{name}').tolist(), c.pop('lr'), c.pop('n')
    assert len(want) == n and 40 <= n <= 60
    w = torch.nn.Parameter(torch.zeros(3))
    opt = pkg.optim.AdamW([{'params': [w]}, {'params': [torch.nn.Parameter(torch.zeros(2))], 'weight_decay': 0.0}], lr=lr)
    sched = pkg.optim.make_scheduler(opt, c)
    assert isinstance(sched, {'multistep': pkg.optim.LinearWarmupMultiStepLR, 'cosine': pkg.optim.LinearWarmupCosineAnnealingLR}[c['name']])
    got = []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                     # "scheduler.step() before optimizer.step()": there is no step on the CPU
        for _ in range(n):
            sched.step()
            got.append([g['lr'] for g in opt.param_groups])
    for k, (a, b) in enumerate(zip(got, want)):
        assert a[0] == a[1], 'both groups follow one schedule'
        assert (a[0] == b) if b == 0 else abs(a[0] - b) <= 1e-12 * abs(b), (name, k, a[0], b)
    # the state of the schedule moves with state_dict(): a fresh scheduler continues where this one stands
    opt2 = pkg.optim.AdamW([torch.nn.Parameter(torch.zeros(3))], lr=lr)
    sched2 = pkg.optim.make_scheduler(opt2, c)
    sched2.load_state_dict(copy.deepcopy(sched.state_dict()))
    assert sched2.last_epoch == sched.last_epoch == n and sched2.get_last_lr()[0] == got[-1][0]


def test_null_scheduler_and_unknown_names(pkg):
    opt = pkg.optim.AdamW([torch.nn.Parameter(torch.zeros(3))])
    assert pkg.optim.make_scheduler(opt, dict(name='null', itrs_per_epoch=4)) is None
    with pytest.raises(NotImplementedError):
        pkg.optim.make_scheduler(opt, dict(name='step', itrs_per_epoch=4))


def toy():
    g = torch.Generator().manual_seed(5)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((4, 3), (7,), (1,))]


def same_state(a, b):
    assert a['param_groups'] == b['param_groups']
    assert sorted(a['state']) == sorted(b['state'])
    for i in a['state']:
        assert sorted(a['state'][i]) == sorted(b['state'][i]) == ['exp_avg', 'exp_avg_sq', 'step']
        for k, v in a['state'][i].items():
            assert torch.equal(torch.as_tensor(v), torch.as_tensor(b['state'][i][k])), (i, k)


def test_state_dict_moves_between_torch_and_this_optimizer(pkg):
    g = torch.Generator().manual_seed(6)
    ps = toy()
    ref = torch.optim.AdamW([{'params': ps[:2], 'weight_decay': 0.05}, {'params': ps[2:], 'weight_decay': 0.0}], lr=2e-3)
    for _ in range(2):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g)
        ref.step()
    sd = copy.deepcopy(ref.state_dict())
    assert float(sd['state'][0]['step']) == 2.0
    mine = pkg.optim.AdamW([{'params': toy()[:2]}, {'params': toy()[2:]}])
    mine.load_state_dict(copy.deepcopy(sd))
    same_state(mine.state_dict(), sd)
    assert [g['weight_decay'] for g in mine.param_groups] == [0.05, 0.0] and mine.param_groups[0]['lr'] == 2e-3
    # ... and back: what this optimizer hands out is a state torch.optim.AdamW takes and steps from exactly as from its own
    back = toy()
    other = torch.optim.AdamW([{'params': back[:2]}, {'params': back[2:]}])
    other.load_state_dict(copy.deepcopy(mine.state_dict()))
    same_state(other.state_dict(), sd)
    with torch.no_grad():
        for p, q in zip(back, ps):
            p.copy_(q)
    for p, q in zip(back, ps):
        p.grad = torch.randn(p.shape, generator=g)
        q.grad = p.grad.clone()
    ref.step()
    other.step()
    assert all(torch.equal(p, q) for p, q in zip(back, ps))
    # a fresh optimizer of this class hands torch the group keys it reads
    fresh = pkg.optim.AdamW(toy(), lr=1e-3, weight_decay=0.05, mode='adam')
    assert fresh.state_dict()['param_groups'] == torch.optim.Adam(toy(), lr=1e-3, weight_decay=0.05).state_dict()['param_groups']
    assert pkg.optim.AdamW(toy()).state_dict()['param_groups'] == torch.optim.AdamW(toy()).state_dict()['param_groups']


def test_refusals(pkg):
    O = pkg.optim
    model = model_of(pkg, 'step_grad_s1')
    with pytest.raises(NotImplementedError, match='sgd'):
        O.make_optimizer(model, dict(name='sgd', lr=1e-3, weight_decay=0.05))
    with pytest.raises(NotImplementedError):
        O.make_optimizer(model, dict(name='lion', lr=1e-3, weight_decay=0.05))
    with pytest.raises(ValueError, match='float32'):
        O.AdamW([torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))])
    with pytest.raises(ValueError, match='parameter 1 of group 0.*contiguous'):
        O.AdamW([torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(4, 3).t())])
    half = model_of(pkg, 'step_grad_s1')
    half.vid_map.conv.weight.data = half.vid_map.conv.weight.data.half()
    with pytest.raises(ValueError, match="'vid_map.conv.weight'.*float32"):
        O.make_optimizer(half, pkg.config.make_opt().optimizer)
    with pytest.raises(ValueError, match='mode'):
        O.AdamW(toy(), mode='sgd')
    opt = O.AdamW(toy())
    for p in opt.param_groups[0]['params']:
        p.grad = torch.zeros_like(p)
    with pytest.raises(RuntimeError, match='GPU'):
        opt.step()
    with pytest.raises(RuntimeError, match='GPU'):
        O.clip_grad_norm_(opt.param_groups[0]['params'], 1.0)
    with pytest.raises(RuntimeError, match='GPU'):
        O.grad_norm_and_coef(opt.param_groups[0]['params'], 1.0)
    with pytest.raises(NotImplementedError, match='PtTransformerEarlyFusionIterative'):
        pkg.train.training_forward(pkg.modeling.PtTransformer(pkg.config.make_opt(n_levels=3, E=32, TE=32, D=32, text_in=32, n_heads=2,
                                                                                 max_seq_len=64, text_layers=1)), *[None] * 6)


def test_model_ema_is_the_trainer_s_copy(pkg):
    model = model_of(pkg, 'step_grad_s1').train()
    ema = pkg.optim.ModelEma(model, 0.999)
    assert not ema.module.training and all(not p.requires_grad for p in ema.module.parameters())
    assert all(p.requires_grad for p in model.parameters()) and model.training
    assert list(ema.state_dict()) == list(model.state_dict())
    pairs = ema.pairs()
    assert len(pairs) == len(list(model.parameters())) and all(p is not e and torch.equal(p, e) for p, e in pairs)
    with torch.no_grad():
        model.vid_map.conv.bias.add_(1.0)
    assert not torch.equal(model.vid_map.conv.bias, ema.module.vid_map.conv.bias)
    ema.init_from(model)
    assert torch.equal(model.vid_map.conv.bias, ema.module.vid_map.conv.bias)


def test_model_ema_leaves_behind_what_a_forward_left(pkg):
    """the engine, the output cache and the borrowed input / output buffers of the last forward are not part of the copy"""
    model = model_of(pkg, 'step_grad_s1')
    big = torch.zeros(1000)
    model._last_inputs, model._last_flat, model._out_cache = ([big], None), (big, big, big), {'k': (big, big, big)}
    ema = pkg.optim.ModelEma(model, 0.9)
    assert ema.module._last_inputs is None and ema.module._last_flat is None and ema.module._out_cache == {} and ema.module._engine is None
    assert model._last_flat[0] is big and model._out_cache['k'][0] is big


def test_a_generator_of_parameters_is_walked_once(pkg):
    """no gradient anywhere: the parameters themselves are still looked at (a generator would be spent by the first walk)"""
    ps = toy()
    with pytest.raises(RuntimeError, match='GPU'):
        pkg.optim.grad_norm_and_coef((p for p in ps), 1.0)
    with pytest.raises(RuntimeError, match='GPU'):
        pkg.optim.clip_grad_norm_(iter(ps), 1.0)


def test_the_constructor_s_mode_holds_where_a_loaded_group_lacks_the_key(pkg):
    """param_groups saved by a torch release without `decoupled_weight_decay` must not turn an 'adam' optimizer into AdamW"""
    for mode, code in (('adam', 1), ('adamw', 0)):
        opt = pkg.optim.AdamW(toy(), mode=mode)
        sd = opt.state_dict()
        for g in sd['param_groups']:
            del g['decoupled_weight_decay']
        opt.load_state_dict(sd)
        assert 'decoupled_weight_decay' not in opt.param_groups[0]
        assert opt._group_array({(0, 1.0): 0})[0].mode == code
    opt = pkg.optim.AdamW(toy(), mode='adam')                     # the key, where present, decides (torch's own meaning of it)
    opt.param_groups[0]['decoupled_weight_decay'] = True
    assert opt._group_array({(0, 1.0): 0})[0].mode == 0


def test_new_exports_and_abi_version(pkg):
    lib = pkg._lib.lib()
    assert lib.dcf_abi_version() == 12
    for s in ('dcf_optim_grad_norm', 'dcf_optim_scale', 'dcf_optim_adam_step'):
        assert s in pkg._lib.SIGNATURES and hasattr(lib, s)
    assert pkg.optim.CHUNK == pkg._lib.OPTIM_CHUNK == 4096


def test_bad_arguments_fail_with_a_message(pkg):
    """null table, negative count, too many groups, unknown mode: refused on the host before anything is launched"""
    import ctypes
    lib, lb = pkg._lib.lib(), pkg._lib
    err = lambda: lib.dcf_last_error().decode()
    assert lib.dcf_optim_adam_step(None, None, 1, 5, None, 0, None, 0, 0.0, None) == -1 and 'null table' in err()
    assert lib.dcf_optim_grad_norm(None, None, 1, 5, 1.0, None, None, None) == -1 and 'null table' in err()
    assert lib.dcf_optim_scale(None, None, 1, 5, None, None) == -1 and 'null table' in err()
    assert lib.dcf_optim_adam_step(None, None, -1, 0, None, 0, None, 0, 0.0, None) == -1 and 'negative count' in err()
    assert lib.dcf_optim_scale(None, None, 0, -2, None, None) == -1 and 'negative count' in err()
    groups = (lb.DcfOptimGroup * 9)()
    assert lib.dcf_optim_adam_step(None, None, 0, 0, ctypes.cast(groups, ctypes.c_void_p), 9, None, 0, 0.0, None) == -1 and '9 groups' in err()
    groups[1].mode = 7
    assert lib.dcf_optim_adam_step(None, None, 0, 0, ctypes.cast(groups, ctypes.c_void_p), 2, None, 0, 0.0, None) == -1
    assert 'unknown mode 7' in err()
    assert ctypes.sizeof(lb.DcfOptimGroup) == 40
