"""GPU checks of ``optim.AdamW(..., device_count=True)`` (include/decafnet_hip_clock.h) on toy parameters of shapes (4, 3), (7,), (1,)
and (4097,) in two groups, with an EMA copy and seeded gradients.

1. no guard: four steps have the bits of ``device_count=False`` in p, both moments and the EMA copy; ``state_dict()`` is equal by
   ``same_state`` of tests/test_optim_cpu.py.
2. with a guard, over g1, g_bad (a NaN in one tensor), g2, g3: bit for bit a plain host-count optimizer over g1, g2, g3; every ``step``
   of its ``state_dict()`` is 3; the same run with ``device_count=False`` differs (the documented departure: its corrections follow the
   attempts), which shows that the comparison is sensitive.
3. gradients that arrive late: ten parameters, parameter i with its first gradient at step i, so that a step has more than 8 (group,
   count) pairs.  ``device_count=False`` raises its NotImplementedError; ``device_count=True`` runs and meets the rule of
   tests/test_gpu_optim.py (``compare``, imported) against torch.optim.AdamW on the CPU in fp64 and fp32.  This check runs ten steps
   where the rule's other users run three, at betas (0.875, 1 - 2^-9), which fp32 holds exactly.  Why: ``adam_elem`` multiplies the
   moment by the fp32 beta; 0.9f is 2.6e-8 (relative) off 0.9, which compounds to k * 2.6e-8 after k steps, and torch's lerp form has
   no such term.  At k = 8 that is 0.44 of the rule's floor of 2^-21 before any rounding; with the default betas the run measured
   e_gpu 4.38e-08 against a bound of 3.68e-08 on exp_avg of the one-element tensor (count 8), a moment that does not depend on the
   count at all and has the bits of the default path (check 1).  What this check is about -- every row takes the corrections of ITS
   count; a neighbour's would be off by 5 % and more -- does not depend on the betas, so it uses betas without that term.
4. a state dict of torch.optim.AdamW with step = 2 loads, steps, and hands back step = 3; a group added later starts at 0 while the
   others keep their counts."""
import copy

import pytest
import torch

from conftest import load_pkg
from test_gpu_optim import compare
from test_optim_cpu import same_state

pytestmark = pytest.mark.gpu
SHAPES = ((4, 3), (7,), (1,), (4097,))
LATE = SHAPES + ((5,), (2, 2), (3,), (9,), (6,), (8,))
LR, WD, BETA = 2e-3, (0.05, 0.0), 0.999
EXACT_BETAS = (0.875, 1.0 - 2.0 ** -9)         # both, and 1 - b of both, are fp32 numbers
KINDS = ('p', 'exp_avg', 'exp_avg_sq', 'ema')


@pytest.fixture(scope='module')
def pkg():
    return load_pkg()


def values(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) for s in shapes]


class Toy:
    def __init__(self, pkg, shapes=SHAPES, **kw):
        self.p = [torch.nn.Parameter(v.cuda()) for v in values(shapes, 5)]
        self.ema = [(v + 0.01).cuda() for v in values(shapes, 5)]
        half = len(shapes) // 2
        self.opt = pkg.optim.AdamW([{'params': self.p[:half], 'weight_decay': WD[0]}, {'params': self.p[half:], 'weight_decay': WD[1]}], lr=LR, **kw)
        self.opt.attach_ema(self.ema, BETA)

    def set_grads(self, grads):
        for p, g in zip(self.p, grads):
            p.grad = None if g is None else g.cuda()

    def bits(self):
        st = self.opt.state
        moments = lambda k: [st[p][k].cpu().clone() if p in st and st[p] else None for p in self.p]
        return {'p': [p.detach().cpu().clone() for p in self.p], 'exp_avg': moments('exp_avg'), 'exp_avg_sq': moments('exp_avg_sq'),
                'ema': [e.cpu().clone() for e in self.ema]}

    def steps(self):
        return [float(s['step']) for s in self.opt.state_dict()['state'].values()]


def differ(a, b):
    return [(k, i) for k in KINDS for i, (u, v) in enumerate(zip(a[k], b[k]))
            if (u is None) != (v is None) or (u is not None and not torch.equal(u.view(torch.int32), v.view(torch.int32)))]


def grads_of(k, shapes=SHAPES):
    return values(shapes, 100 + k)


def test_four_steps_have_the_bits_of_the_host_count(pkg):
    on, off = Toy(pkg, device_count=True), Toy(pkg)
    for k in range(4):
        for t in (on, off):
            t.set_grads(grads_of(k))
            _, coef = pkg.optim.grad_norm_and_coef(t.p, 1.0)
            t.opt.step(clip_coef=coef)
        assert not differ(on.bits(), off.bits()), k
    same_state(on.opt.state_dict(), off.opt.state_dict())
    assert on.steps() == [4.0] * 4 and all(s['step'].dtype == torch.float32 and s['step'].device.type == 'cpu' and s['step'].numel() == 1
                                           for s in on.opt.state_dict()['state'].values())
    assert on.opt._steps.dtype == torch.int64 and on.opt._steps.tolist() == [4] * 4 and on.opt.table_uploads == off.opt.table_uploads


def guarded_run(pkg, toy, seq):
    guard = pkg.optim.StepGuard('cuda')
    for grads in seq:
        toy.set_grads(grads)
        _, coef = pkg.optim.grad_norm_and_coef(toy.p, 1.0, guard=guard)
        toy.opt.step(clip_coef=coef, guard=guard)
    return guard.report()


def test_under_a_guard_the_counts_follow_the_applied_steps(pkg):
    g1, g2, g3 = grads_of(1), grads_of(2), grads_of(3)
    bad = grads_of(7)
    bad[3][1234] = float('nan')
    on, off, plain = Toy(pkg, device_count=True), Toy(pkg), Toy(pkg)
    rep = guarded_run(pkg, on, [g1, bad, g2, g3])
    assert (rep['applied'], rep['skipped'], rep['last_skipped_attempt']) == (3, 1, 1)
    for grads in (g1, g2, g3):                            # a plain host-count optimizer that never saw the bad gradient
        plain.set_grads(grads)
        _, coef = pkg.optim.grad_norm_and_coef(plain.p, 1.0)
        plain.opt.step(clip_coef=coef)
    assert not differ(on.bits(), plain.bits())
    assert on.steps() == [3.0] * 4 == plain.steps()
    same_state(on.opt.state_dict(), plain.opt.state_dict())
    rep = guarded_run(pkg, off, [g1, bad, g2, g3])
    assert (rep['applied'], rep['skipped']) == (3, 1) and off.steps() == [4.0] * 4
    assert {k for k, _ in differ(on.bits(), off.bits())} >= {'p', 'ema'}, 'the host count follows the attempts: its corrections differ'
    assert not {k for k, _ in differ(on.bits(), off.bits())} & {'exp_avg', 'exp_avg_sq'}, 'the moments do not depend on the count'


def test_gradients_that_arrive_late_give_every_parameter_a_count_of_its_own(pkg):
    n, steps = len(LATE), len(LATE)
    seq = [[g if i <= k else None for i, g in enumerate(grads_of(20 + k, LATE))] for k in range(steps)]
    assert all(float(torch.tensor(b, dtype=torch.float32)) == b and float(torch.tensor(1.0 - b, dtype=torch.float32)) == 1.0 - b for b in EXACT_BETAS)
    off = Toy(pkg, LATE, betas=EXACT_BETAS)
    with pytest.raises(NotImplementedError, match='distinct') as e:
        for grads in seq:
            off.set_grads(grads)
            off.opt.step()
    # refused at the first step with nine pairs, before any count of that step advanced (the ninth parameter has its moments, at count 0)
    assert '9 distinct' in str(e.value) and off.steps() == [float(8 - i) for i in range(9)]
    on = Toy(pkg, LATE, betas=EXACT_BETAS, device_count=True)
    on.opt.attach_ema(None, None)
    for grads in seq:
        on.set_grads(grads)
        on.opt.step()
    assert on.steps() == [float(n - i) for i in range(n)] and on.opt._steps.tolist() == [n - i for i in range(n)]
    out = {}
    for dt in (torch.float64, torch.float32):
        ps = [torch.nn.Parameter(v.to(dt)) for v in values(LATE, 5)]
        ref = torch.optim.AdamW([{'params': ps[:n // 2], 'weight_decay': WD[0]}, {'params': ps[n // 2:], 'weight_decay': WD[1]}], lr=LR, betas=EXACT_BETAS,
                                foreach=False)
        for grads in seq:
            for p, g in zip(ps, grads):
                p.grad = None if g is None else g.to(dt)
            ref.step()
        assert [float(ref.state[p]['step']) for p in ps] == on.steps()
        out[dt] = {'p': [p.detach() for p in ps], 'exp_avg': [ref.state[p]['exp_avg'] for p in ps],
                   'exp_avg_sq': [ref.state[p]['exp_avg_sq'] for p in ps]}
    missed = compare('late gradients, ten counts', on.bits(), out[torch.float64], out[torch.float32], kinds=KINDS[:3])
    assert not missed, missed[:8]


def test_a_state_dict_of_torch_loads_steps_and_comes_back(pkg):
    ps = [torch.nn.Parameter(v) for v in values(SHAPES, 5)]
    ref = torch.optim.AdamW([{'params': ps[:2], 'weight_decay': WD[0]}, {'params': ps[2:], 'weight_decay': WD[1]}], lr=LR)
    for k in range(2):
        for p, g in zip(ps, grads_of(k)):
            p.grad = g
        ref.step()
    sd = copy.deepcopy(ref.state_dict())
    assert all(float(s['step']) == 2.0 for s in sd['state'].values())
    on, off = Toy(pkg, device_count=True), Toy(pkg)
    for t in (on, off):
        with torch.no_grad():
            for p, q in zip(t.p, ps):
                p.copy_(q)
        t.opt.load_state_dict(copy.deepcopy(sd))
    assert on.opt._steps.tolist() == [2] * 4 and on.steps() == [2.0] * 4
    same_state(on.opt.state_dict(), off.opt.state_dict())
    for t in (on, off):
        t.set_grads(grads_of(2))
        t.opt.step()
    assert on.steps() == [3.0] * 4 and not differ(on.bits(), off.bits())
    back = on.opt.state_dict()
    same_state(back, off.opt.state_dict())
    assert all(s['step'].dtype == torch.float32 and s['step'].device.type == 'cpu' and float(s['step']) == 3.0 for s in back['state'].values())
    other = torch.optim.AdamW([{'params': ps[:2]}, {'params': ps[2:]}])                 # ... and torch takes it back
    other.load_state_dict(copy.deepcopy(back))
    assert all(float(other.state[p]['step']) == 3.0 for p in ps)
    # a group added later: its parameter starts at 0, the others keep their counts
    extra = [torch.nn.Parameter(torch.full((6,), 0.5, device='cuda')) for _ in (on, off)]
    for t, x in zip((on, off), extra):
        t.opt.add_param_group({'params': [x], 'weight_decay': 0.0})
        t.set_grads(grads_of(3))
        x.grad = torch.full((6,), 0.25, device='cuda')
        t.opt.step()
    assert on.opt._steps.tolist() == [4, 4, 4, 4, 1] and on.steps() == [4.0] * 4 + [1.0] == off.steps()
    assert not differ(on.bits(), off.bits()) and torch.equal(extra[0], extra[1])
    eight = pkg.optim.AdamW([{'params': [torch.nn.Parameter(torch.zeros(2, device='cuda'))]} for _ in range(9)], device_count=True)
    for group in eight.param_groups:
        group['params'][0].grad = torch.ones(2, device='cuda')
    with pytest.raises(NotImplementedError, match='9 parameter groups'):
        eight.step()
