"""GPU checks of the training update: dcf_optim_grad_norm / dcf_optim_scale / dcf_optim_adam_step through cvpr2025-decafnet_amd/optim.py.

The yardstick is torch itself on the CPU, computed here, because the reference calls exactly these: torch.nn.utils.clip_grad_norm_,
torch.optim.AdamW / Adam (foreach=False) and p.lerp(ema, beta) (libs/worker_v2.py:320-325, :654-656).  It runs once in fp64 (x_64) and
once in fp32 (x_32) from the same fp32 inputs, and the project's rule (tests/test_gpu_dec_grad.py), unchanged, is applied per tensor to
each of p, exp_avg, exp_avg_sq and ema, and to the scalar norm and coefficient:

    e_gpu <= max(4 * e_ref, 2^-21 * max |x_64|),   e = max |x - x_64|,   e_ref = e of the fp32 CPU run

The two error sources are kept apart: the norm and the coefficient are checked against the fp64 norm; the update is checked against a
yardstick that is handed the GPU's own coefficient (read back and multiplied into the yardstick's gradients in both precisions), so the
norm's rounding is not counted again in every tensor.  Every check prints an `OPTERR` line.

Inputs (seeded): 311 tensors, about 31 000 elements: 1, 3, 4, 5, 255, 256, 257, CHUNK-1, CHUNK, CHUNK+1, 2*CHUNK+7 and 300 tensors of
1 - 64 elements; parameter scales log-uniform in 1e-3 .. 3, gradient scales log-uniform in 1e-9 .. 10 per tensor, one all-zero gradient,
one parameter a view one element into a larger buffer (4-byte aligned only; its moments and EMA copy stay aligned); two groups
(weight_decay 0.05 / 0), lr 1e-3, betas (0.9, 0.999), eps 1e-8, EMA beta 0.999, three steps with fresh gradients."""
import copy
import ctypes
import math

import numpy as np
import pytest
import torch

from conftest import load_pkg

pytestmark = pytest.mark.gpu
FLOOR = 2.0 ** -21
CHUNK = 4096
SIZES = [1, 3, 4, 5, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 7]
N_SMALL, STEPS = 300, 3
ZERO_GRAD, MISALIGNED, BIG = 13, 6, 10          # tensor 13 (group 1: weight_decay 0) has an all-zero gradient; 6 is the offset view
LR, BETAS, EPS, WD, BETA = 1e-3, (0.9, 0.999), 1e-8, (0.05, 0.0), 0.999
KINDS = ('p', 'exp_avg', 'exp_avg_sq', 'ema')


@pytest.fixture(scope='module')
def pkg():
    return load_pkg()


class Inputs:
    """the seeded CPU inputs, made once and never written: p0[i], ema0[i], grads[step][i]; group of tensor i = i % 2"""

    def __init__(self, seed=20260, steps=STEPS):
        rs = np.random.RandomState(seed)
        self.sizes = SIZES + [int(n) for n in rs.randint(1, 65, N_SMALL)]
        n = len(self.sizes)
        t = lambda k, s: torch.from_numpy((rs.standard_normal(k) * s).astype(np.float32))
        ps = np.exp(rs.uniform(math.log(1e-3), math.log(3.0), n))
        gs = np.exp(rs.uniform(math.log(1e-9), math.log(10.0), n))
        gs[BIG] = 10.0                                       # the norm of the set is well above max_norm = 1
        self.p0 = [t(k, s) for k, s in zip(self.sizes, ps)]
        self.ema0 = [p + t(p.numel(), 0.01 * s) for p, s in zip(self.p0, ps)]
        self.grads = [[t(k, s) for k, s in zip(self.sizes, gs)] for _ in range(steps)]
        for g in self.grads:
            g[ZERO_GRAD].zero_()
        self.group = [i % 2 for i in range(n)]
        assert n == 311 and 29000 < sum(self.sizes) < 33000 and self.group[ZERO_GRAD] == 1


_inputs = {}


def inputs():
    if 'x' not in _inputs:
        _inputs['x'] = Inputs()
    return _inputs['x']


def check(tag, got, x64, x32):
    got, x64, x32 = got.detach().cpu().double(), x64.detach().double(), x32.detach().double()
    assert got.shape == x64.shape == x32.shape, (tag, got.shape, x64.shape, x32.shape)
    top = float(x64.abs().max())
    e_ref, e_gpu = float((x32 - x64).abs().max()), float((got - x64).abs().max())
    bound = max(4 * e_ref, FLOOR * top)
    ok = bool(torch.isfinite(got).all()) and e_gpu <= bound
    print(f'OPTERR {tag}: max|x64| {top:.3e} e_ref {e_ref:.3e} e_gpu {e_gpu:.3e} bound {bound:.3e} ratio {e_gpu / bound if bound else 0.0:.3f}'
          f'{"" if ok else "  MISSED"}')
    return None if ok else (tag, e_gpu, bound)


def groups_of(ps, group, wd=WD, lr=LR):
    return [{'params': [p for p, g in zip(ps, group) if g == k], 'weight_decay': wd[k], 'lr': lr} for k in (0, 1)]


def gpu_param(src, misaligned=False):
    """a leaf on the GPU holding src; misaligned: a view one element into a larger buffer (address = 4 mod 16)"""
    if not misaligned:
        return torch.nn.Parameter(src.cuda())
    buf = torch.zeros(src.numel() + 8, device='cuda')
    buf[1:1 + src.numel()].copy_(src)
    p = torch.nn.Parameter(buf[1:1 + src.numel()])
    assert p.data_ptr() % 16 == 4 and p.is_contiguous()
    return p


class Device:
    """the inputs on the GPU with this package's optimizer over them.  `order`: the order in which the tensors are ALLOCATED (the table
    order stays that of the inputs)"""

    def __init__(self, pkg, x, mode='adamw', beta=BETA, attach=True, order=None, lr=LR):
        n = len(x.sizes)
        self.x, self.pkg = x, pkg
        self.p, self.ema = [None] * n, [None] * n
        for i in (range(n) if order is None else order):
            self.p[i] = gpu_param(x.p0[i], i == MISALIGNED)
            self.ema[i] = x.ema0[i].cuda()
        self.opt = pkg.optim.AdamW(groups_of(self.p, x.group, lr=lr), lr=lr, betas=BETAS, eps=EPS, mode=mode)
        self.flat = [p for g in self.opt.param_groups for p in g['params']]
        if attach:
            self.opt.attach_ema(dict(zip(self.p, self.ema)), beta)

    def set_grads(self, step, scale=1.0, skip=(), order=None):
        n = len(self.p)
        for i in (range(n) if order is None else order):
            self.p[i].grad = None if i in skip else (self.x.grads[step][i] * scale).cuda()

    def state(self):
        """{kind: [tensor per input index]} as CPU copies (exp_avg / exp_avg_sq: None before the first gradient)"""
        st = self.opt.state
        return {'p': [p.detach().cpu().clone() for p in self.p],
                'exp_avg': [st[p]['exp_avg'].cpu().clone() if p in st and st[p] else None for p in self.p],
                'exp_avg_sq': [st[p]['exp_avg_sq'].cpu().clone() if p in st and st[p] else None for p in self.p],
                'ema': [e.cpu().clone() for e in self.ema]}


def yardstick(x, dt, coefs, lrs=None, mode='adamw', beta=BETA, grads=None):
    """torch on the CPU in dtype dt: per step, every gradient times that step's coefficient (None: 1), AdamW / Adam .step() with
    foreach=False, then ema <- p.lerp(ema, beta).  -> per step {kind: [tensor per input index]}"""
    ps = [torch.nn.Parameter(p.to(dt)) for p in x.p0]
    emas = [e.to(dt) for e in x.ema0]
    cls = torch.optim.AdamW if mode == 'adamw' else torch.optim.Adam
    opt = cls(groups_of(ps, x.group), lr=LR, betas=BETAS, eps=EPS, foreach=False)
    out = []
    for k, coef in enumerate(coefs):
        if lrs is not None:
            for g in opt.param_groups:
                g['lr'] = lrs[k]
        for p, g in zip(ps, (x.grads if grads is None else grads)[k]):
            p.grad = g.to(dt) if coef is None else g.to(dt) * torch.tensor(coef, dtype=torch.float32).to(dt)
        opt.step()
        with torch.no_grad():
            for p, e in zip(ps, emas):
                e.copy_(p.detach().lerp(e, beta))
        out.append({'p': [p.detach().clone() for p in ps], 'exp_avg': [opt.state[p]['exp_avg'].clone() for p in ps],
                    'exp_avg_sq': [opt.state[p]['exp_avg_sq'].clone() for p in ps], 'ema': [e.clone() for e in emas]})
    return out


def compare(tag, got, y64, y32, kinds=KINDS):
    missed = []
    for kind in kinds:
        for i, (a, b, c) in enumerate(zip(got[kind], y64[kind], y32[kind])):
            missed.append(check(f'{tag} {kind}[{i}] n={a.numel()}', a, b, c))
    return [m for m in missed if m is not None]


def same_bits(a, b, kinds=KINDS):
    return [(k, i) for k in kinds for i, (u, v) in enumerate(zip(a[k], b[k]))
            if (u is None) != (v is None) or (u is not None and not torch.equal(u.view(torch.int32), v.view(torch.int32)))]


def cpu_norms(x, step, scale, max_norm):
    """(norm, coefficient) by torch.nn.utils.clip_grad_norm_ on the CPU in fp64 and fp32"""
    out = {}
    for dt in (torch.float64, torch.float32):
        ps = [torch.nn.Parameter(torch.zeros(k, dtype=dt)) for k in x.sizes]
        for p, g in zip(ps, x.grads[step]):
            p.grad = (g * scale).to(dt)
        norm = torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False)
        coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
        out[dt] = (norm, coef)
    return out


# ---------------------------------------------------------------------------------------------- 1: the norm and the coefficient
def test_norm_and_coefficient(pkg):
    x, O = inputs(), pkg.optim
    d = Device(pkg, x, attach=False)
    d.set_grads(0)
    norm, coef = O.grad_norm_and_coef(d.p, 1.0)
    assert norm.is_cuda and coef.is_cuda and norm.dtype == coef.dtype == torch.float32
    ref = cpu_norms(x, 0, 1.0, 1.0)
    assert float(ref[torch.float64][0]) > 1.0
    missed = [check('norm, above max_norm', norm, *(ref[dt][0] for dt in (torch.float64, torch.float32))),
              check('coef, above max_norm', coef, *(ref[dt][1] for dt in (torch.float64, torch.float32)))]
    assert float(coef) < 1.0
    # the same bits on a second run, and with the tensors allocated in another order (the table order kept)
    norm2, coef2 = O.grad_norm_and_coef(d.p, 1.0)
    assert norm2.view(torch.int32).item() == norm.view(torch.int32).item() and coef2.view(torch.int32).item() == coef.view(torch.int32).item()
    order = list(np.random.RandomState(3).permutation(len(x.sizes)))
    e = Device(pkg, x, attach=False, order=order)
    e.set_grads(0, order=order[::-1])
    assert [p.data_ptr() for p in e.p] != [p.data_ptr() for p in d.p]
    norm3, _ = O.grad_norm_and_coef(e.p, 1.0)
    assert norm3.view(torch.int32).item() == norm.view(torch.int32).item()
    # ... and with one gradient a view one element into a larger buffer: the 16-byte and the one-element path sum alike
    buf = torch.zeros(x.sizes[BIG] + 8, device='cuda')
    buf[1:1 + x.sizes[BIG]].copy_(x.grads[0][BIG])
    e.p[BIG].grad = buf[1:1 + x.sizes[BIG]]
    assert e.p[BIG].grad.data_ptr() % 16 == 4
    norm4, _ = O.grad_norm_and_coef(e.p, 1.0)
    assert norm4.view(torch.int32).item() == norm.view(torch.int32).item()
    # below max_norm: the coefficient is exactly 1
    scale = 0.25 / float(ref[torch.float64][0])
    d.set_grads(0, scale=scale)
    norm_s, coef_s = O.grad_norm_and_coef(d.p, 1.0)
    ref_s = cpu_norms(x, 0, scale, 1.0)
    missed.append(check('norm, below max_norm', norm_s, *(ref_s[dt][0] for dt in (torch.float64, torch.float32))))
    assert float(coef_s) == 1.0 and float(norm_s) < 1.0
    # max_norm = 0: no clipping, the norm still written
    d.set_grads(0)
    norm0, coef0 = O.grad_norm_and_coef(d.p, 0.0)
    assert float(coef0) == 1.0 and norm0.view(torch.int32).item() == norm.view(torch.int32).item()
    assert not [m for m in missed if m is not None], missed


# ---------------------------------------------------------------------------------------------- 2: three steps under the rule
@pytest.mark.parametrize('mode', ['adamw', 'adam'])
def test_three_steps_with_ema_meet_the_rule(pkg, mode):
    x, O = inputs(), pkg.optim
    d = Device(pkg, x, mode=mode)
    coefs, got = [], []
    for k in range(STEPS):
        d.set_grads(k)
        _, coef = O.grad_norm_and_coef(d.p, 1.0)
        d.opt.step(clip_coef=coef)
        coefs.append(float(coef))
        got.append(d.state())
    assert all(0.0 < c < 1.0 for c in coefs)
    y64, y32 = (yardstick(x, dt, coefs, mode=mode) for dt in (torch.float64, torch.float32))
    missed = []
    for k in range(STEPS):
        missed += compare(f'{mode} step {k}', got[k], y64[k], y32[k])
    assert not missed, missed[:8]
    assert d.opt.table_uploads <= STEPS


# ---------------------------------------------------------------------------------------------- 3: bit-exact properties
def run_three(pkg, x, **kw):
    d = Device(pkg, x, **kw)
    for k in range(STEPS):
        d.set_grads(k)
        _, coef = pkg.optim.grad_norm_and_coef(d.p, 1.0)
        d.opt.step(clip_coef=coef)
    return d


def test_two_fresh_runs_give_the_same_bits(pkg):
    x = inputs()
    assert not same_bits(run_three(pkg, x).state(), run_three(pkg, x).state())


def test_the_table_is_rebuilt_only_when_an_address_changed(pkg):
    x = inputs()
    d = Device(pkg, x)
    d.set_grads(0)
    d.opt.step()
    d.opt.step()                                                  # the same gradient tensors: nothing to upload
    assert d.opt.table_uploads == 1
    for p in d.p:
        p.grad.mul_(0.5)                                          # in place: the addresses stay
    d.opt.step()
    assert d.opt.table_uploads == 1
    d.p[3].grad = d.p[3].grad.clone()                             # one new address
    d.opt.step()
    assert d.opt.table_uploads == 2
    old = [p.grad for p in d.p]                                   # kept alive: the new gradients cannot land on these addresses
    d.opt.zero_grad(set_to_none=True)
    d.set_grads(1)
    d.opt.step()
    assert d.opt.table_uploads == 3 and len(old) == len(d.p)


def test_a_refused_step_leaves_the_counts_and_the_tensors(pkg):
    """what step() refuses after its walk over the parameters (an option it does not implement, a bad clip_coef) changes nothing:
    the step counts do not advance, nothing is launched; the next good step is the one the yardstick takes"""
    x = inputs()
    d = Device(pkg, x)
    d.set_grads(0)
    d.opt.step()
    before = d.state()
    versions = [p._version for p in d.p]
    d.set_grads(1)
    d.opt.param_groups[1]['amsgrad'] = True
    with pytest.raises(NotImplementedError, match='amsgrad'):
        d.opt.step()
    d.opt.param_groups[1]['amsgrad'] = False
    with pytest.raises(ValueError, match='clip_coef'):
        d.opt.step(clip_coef=torch.ones(2, device='cuda'))
    assert all(float(d.opt.state[p]['step']) == 1.0 for p in d.p)
    assert not same_bits(before, d.state()) and versions == [p._version for p in d.p]
    d.opt.step()
    assert all(float(d.opt.state[p]['step']) == 2.0 for p in d.p)
    y64, y32 = (yardstick(x, dt, [None, None])[-1] for dt in (torch.float64, torch.float32))
    missed = compare('after two refused steps', d.state(), y64, y32)
    assert not missed, missed[:8]


def test_written_tensors_advance_their_version_counter(pkg):
    """the kernels write through raw addresses; every tensor they wrote counts one in-place change, the others none"""
    x, O = inputs(), pkg.optim
    d = Device(pkg, x)
    d.set_grads(0, skip=(BIG,))
    d.opt.step()                                                  # creates the moments
    moments = lambda: [d.opt.state[p][k]._version for p in d.p if p is not d.p[BIG] for k in ('exp_avg', 'exp_avg_sq')]
    v0 = ([p._version for p in d.p], [e._version for e in d.ema], moments(), [p.grad._version for p in d.p if p.grad is not None])
    d.opt.step()
    v1 = ([p._version for p in d.p], [e._version for e in d.ema], moments(), [p.grad._version for p in d.p if p.grad is not None])
    assert [b - a for a, b in zip(v0[0], v1[0])] == [0 if i == BIG else 1 for i in range(len(d.p))]
    assert [b - a for a, b in zip(v0[1], v1[1])] == [1] * len(d.ema)                      # the EMA copy moves, gradient or not
    assert [b - a for a, b in zip(v0[2], v1[2])] == [1] * len(v0[2]) and v0[3] == v1[3]      # the gradients are only read
    O.clip_grad_norm_(d.p, 1.0)
    assert [p.grad._version for p in d.p if p.grad is not None] == [v + 1 for v in v1[3]]


@pytest.mark.parametrize('i', [BIG, MISALIGNED, 0])
def test_a_tensor_alone_gets_the_same_bits(pkg, i):
    x, O = inputs(), pkg.optim
    d = Device(pkg, x)
    d.set_grads(0)
    _, coef = O.grad_norm_and_coef(d.p, 1.0)
    d.opt.step(clip_coef=coef)
    p, ema = gpu_param(x.p0[i], i == MISALIGNED), x.ema0[i].cuda()
    solo = O.AdamW([p], lr=LR, betas=BETAS, eps=EPS, weight_decay=WD[x.group[i]])
    solo.attach_ema([ema], BETA)
    p.grad = x.grads[0][i].cuda()
    solo.step(clip_coef=coef)
    both = d.state()
    for kind, t in (('p', p.detach()), ('exp_avg', solo.state[p]['exp_avg']), ('exp_avg_sq', solo.state[p]['exp_avg_sq']), ('ema', ema)):
        assert torch.equal(t.cpu().view(torch.int32), both[kind][i].view(torch.int32)), kind


def test_no_gradient_keeps_the_tensor_and_moves_its_ema(pkg):
    x = inputs()
    d = Device(pkg, x)
    d.set_grads(0)
    d.opt.step()
    before = d.state()
    skip = (BIG, MISALIGNED, 20)
    d.set_grads(1, skip=skip)
    d.opt.step()
    after = d.state()
    changed = set(same_bits(before, after))
    for i in skip:
        assert not {('p', i), ('exp_avg', i), ('exp_avg_sq', i)} & changed, i
        assert ('ema', i) in changed, i
        assert float(d.opt.state[d.p[i]]['step']) == 1.0
    assert ('p', 21) in changed and float(d.opt.state[d.p[21]]['step']) == 2.0
    # the next step: the tensors that sat out are one step behind (their own bias correction), under the rule against torch
    d.set_grads(2)
    d.opt.step()
    last = d.state()
    out = {}
    for dt in (torch.float64, torch.float32):
        ps = [torch.nn.Parameter(p.to(dt)) for p in x.p0]
        opt = torch.optim.AdamW(groups_of(ps, x.group), lr=LR, betas=BETAS, eps=EPS, foreach=False)
        for k in range(3):
            for i, (p, g) in enumerate(zip(ps, x.grads[k])):
                p.grad = None if (k == 1 and i in skip) else g.to(dt)
            opt.step()
        out[dt] = {'p': [p.detach() for p in ps], 'exp_avg': [opt.state[p]['exp_avg'] for p in ps],
                   'exp_avg_sq': [opt.state[p]['exp_avg_sq'] for p in ps]}
    missed = compare('grad None at step 1, after step 2', last, out[torch.float64], out[torch.float32], kinds=KINDS[:3])
    assert not missed, missed[:8]


def test_zero_gradient_without_decay_keeps_p(pkg):
    x = inputs()
    d = Device(pkg, x)
    d.set_grads(0)
    d.opt.step()
    got = d.state()
    assert torch.equal(got['p'][ZERO_GRAD].view(torch.int32), x.p0[ZERO_GRAD].view(torch.int32))
    assert not got['exp_avg'][ZERO_GRAD].any() and not got['exp_avg_sq'][ZERO_GRAD].any()
    assert not torch.equal(got['p'][ZERO_GRAD + 2], x.p0[ZERO_GRAD + 2])


@pytest.mark.parametrize('beta', [1.0, 0.0])
def test_ema_end_points(pkg, beta):
    x = inputs()
    d = Device(pkg, x, beta=beta)
    d.set_grads(0)
    d.opt.step()
    got = d.state()
    want = x.ema0 if beta == 1.0 else got['p']
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got['ema'], want))
    assert not all(torch.equal(a, b) for a, b in zip(got['p'], x.p0))


def test_nothing_else_is_written(pkg):
    """no EMA attached: only p, exp_avg and exp_avg_sq change.  Every tensor of the step (p, gradient, both moments, an EMA copy that is
    NOT attached) is carved out of one pool with 8 guard words on either side; the guards, the gradients and the EMA copies keep their
    bits."""
    x, O = inputs(), pkg.optim
    GUARD, SENT = 8, 0x7FC12345
    n_words = sum(5 * (((k + 3) // 4) * 4 + 2 * GUARD + 4) for k in x.sizes) + GUARD
    pool = torch.full((n_words,), SENT, dtype=torch.int32, device='cuda')
    fpool = pool.view(torch.float32)
    assert fpool.data_ptr() % 16 == 0
    cursor, owned = [GUARD], torch.zeros(n_words, dtype=torch.bool)

    def carve(src, shift=0):
        a = cursor[0] + shift
        t = fpool[a:a + src.numel()]
        t.copy_(src)
        owned[a:a + src.numel()] = True
        cursor[0] = ((a + src.numel() + 3) // 4) * 4 + 2 * GUARD
        return t

    ps, grads, emas, state = [], [], [], {}
    for i, k in enumerate(x.sizes):
        p = torch.nn.Parameter(carve(x.p0[i], shift=1 if i == MISALIGNED else 0))
        grads.append(carve(x.grads[0][i]))
        emas.append(carve(x.ema0[i]))
        state[p] = {'step': torch.tensor(0.0), 'exp_avg': carve(torch.zeros(k)), 'exp_avg_sq': carve(torch.zeros(k))}
        ps.append(p)
    assert cursor[0] <= n_words and ps[MISALIGNED].data_ptr() % 16 == 4
    opt = O.AdamW(groups_of(ps, x.group), lr=LR, betas=BETAS, eps=EPS)
    for p, g in zip(ps, grads):
        opt.state[p] = state[p]
        p.grad = g
    snapshot = pool.clone()
    opt.step()
    torch.cuda.synchronize()
    guards = ~owned.cuda()
    assert bool((pool[guards] == SENT).all()), 'a guard word was written'
    for i, (g, e, p) in enumerate(zip(grads, emas, ps)):
        assert torch.equal(g.cpu().view(torch.int32), x.grads[0][i].view(torch.int32)), f'p.grad of tensor {i} changed'
        assert torch.equal(e.cpu().view(torch.int32), x.ema0[i].view(torch.int32)), f'the unattached EMA copy of tensor {i} changed'
        assert p.grad is g
    assert not torch.equal(pool, snapshot)
    # ... and what was written is what the ordinary allocation gets
    d = Device(pkg, x, attach=False)
    d.set_grads(0)
    d.opt.step()
    want = d.state()
    for i, p in enumerate(ps):
        assert torch.equal(p.detach().cpu().view(torch.int32), want['p'][i].view(torch.int32)), i
        assert torch.equal(state[p]['exp_avg_sq'].cpu().view(torch.int32), want['exp_avg_sq'][i].view(torch.int32)), i


# ---------------------------------------------------------------------------------------------- 4: clip_grad_norm_ in place
def test_clip_grad_norm_in_place(pkg):
    x, O = inputs(), pkg.optim
    d = Device(pkg, x, attach=False)
    d.set_grads(0)
    norm1, coef = O.grad_norm_and_coef(d.p, 1.0)
    norm = O.clip_grad_norm_(d.p, 1.0)
    assert norm.is_cuda and norm.view(torch.int32).item() == norm1.view(torch.int32).item()
    c = float(coef)
    missed = []
    for i, p in enumerate(d.p):
        g = x.grads[0][i]
        missed.append(check(f'clipped grad[{i}]', p.grad, g.double() * c, g * torch.tensor(c, dtype=torch.float32)))
    assert not [m for m in missed if m is not None], missed[:8]
    # a single tensor, as torch's function takes one
    d.set_grads(0)
    n_one = O.clip_grad_norm_(d.p[BIG], 1.0)
    missed = [check('norm of one tensor', n_one, x.grads[0][BIG].double().norm(), x.grads[0][BIG].norm())]
    assert not [m for m in missed if m is not None], missed


# ---------------------------------------------------------------------------------------------- 5: lr through param_groups
def test_learning_rate_change_takes_effect_on_the_next_step(pkg):
    x = inputs()
    lrs = [1e-3, 4e-4, 7e-5]
    d = Device(pkg, x)
    got = []
    for k in range(STEPS):
        for g in d.opt.param_groups:
            g['lr'] = lrs[k]
        d.set_grads(k)
        d.opt.step()
        got.append(d.state())
    y64, y32 = (yardstick(x, dt, [None] * STEPS, lrs=lrs) for dt in (torch.float64, torch.float32))
    missed = []
    for k in range(STEPS):
        missed += compare(f'lr {lrs[k]:g} step {k}', got[k], y64[k], y32[k])
    assert not missed, missed[:8]
    # and the change is not lost in rounding: the same steps at a constant lr end elsewhere
    flat = yardstick(x, torch.float64, [None] * STEPS)
    assert float((flat[-1]['p'][BIG] - y64[-1]['p'][BIG]).abs().max()) > 100 * FLOOR * float(y64[-1]['p'][BIG].abs().max())


# ---------------------------------------------------------------------------------------------- 6: state-dict hand-over on the device
def test_state_dict_hand_over_to_torch_on_the_device(pkg):
    x = inputs()
    d = Device(pkg, x, attach=False)
    for k in range(2):
        d.set_grads(k)
        d.opt.step()
    clones = [torch.nn.Parameter(p.detach().clone()) for p in d.p]
    theirs = torch.optim.AdamW(groups_of(clones, x.group), lr=LR, betas=BETAS, eps=EPS)
    theirs.load_state_dict(copy.deepcopy(d.opt.state_dict()))
    d.set_grads(2)
    for c, p in zip(clones, d.p):
        c.grad = p.grad.clone()
    d.opt.step()
    theirs.step()
    got = d.state()
    y64, y32 = (yardstick(x, dt, [None] * STEPS)[-1] for dt in (torch.float64, torch.float32))
    missed = compare('after the hand-over', got, y64, y32, kinds=KINDS[:3])
    worst = max(float((c.detach().cpu().double() - b).abs().max()) / max(FLOOR * float(b.abs().max()), 1e-300) for c, b in zip(clones, y64['p']))
    print(f'OPTERR torch.optim.AdamW on the GPU from the same state, worst e / (2^-21 max|x64|) over p: {worst:.3f} (not asserted)')
    assert float(theirs.state[clones[0]]['step']) == 3.0
    assert not missed, missed[:8]


# ---------------------------------------------------------------------------------------------- 7: a NaN in one gradient
def test_nan_gradient_gives_nan_norm_and_coefficient(pkg):
    """torch's default (error_if_nonfinite=False): the norm and the coefficient come back NaN.  Ordinary arithmetic on a NaN, no fault."""
    x, O = inputs(), pkg.optim
    d = Device(pkg, x, attach=False)
    d.set_grads(0)
    d.p[40].grad[0] = float('nan')
    norm, coef = O.grad_norm_and_coef(d.p, 1.0)                   # raises if the call does not return 0
    torch.cuda.synchronize()
    assert math.isnan(float(norm)) and math.isnan(float(coef))
    out = torch.zeros(2, device='cuda')
    lb = pkg._lib
    rc = lb.lib().dcf_optim_grad_norm(*O._CLIP_TABLE.args(), 1.0, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(out.data_ptr() + 4),
                                      lb.current_stream())
    torch.cuda.synchronize()
    assert rc == 0 and bool(torch.isnan(out).all())
    hip = ctypes.CDLL(None)                                       # the HIP runtime torch has loaded
    assert hip.hipGetLastError() == 0
