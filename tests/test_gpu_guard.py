"""GPU checks of the step-guard extension at operator level (include/decafnet_hip_guard.h, csrc/optim_guard.hip), on one table of eight
rows -- 1, 0, 3, 4095, 8200, 4096, 5 (DCF_OPTIM_NO_GRAD) and 4097 elements, three of them starting 4 bytes past a 16-byte boundary, one
without an EMA copy, two groups (AdamW and Adam):

1. all gradients finite: norm, coefficient, p, exp_avg, exp_avg_sq and ema of the guarded pair have the bits of dcf_optim_grad_norm +
   dcf_optim_adam_step on copies; the verdict is apply.
2. one NaN / +inf / -inf / 1e20 at the first element of row 0, the last element of a short last chunk, the first element after a chunk
   boundary, or in the last row: the verdict is skip, every byte of every tensor (and of the padding around it) is what it was, the
   record equals the restatement (tests/guard_ref.py).  The same value in the NO_GRAD row changes nothing.
3. finite again after a skip: the update applies with the unguarded bits; the record still names the last skip.
4. the conv-gradient word under an armed guard: no call fails, the guarded norm over finite gradients skips with conv_flag set and
   clears the word; disarmed, the one-shot failure of the next call is back.

Bit-exact throughout: no tolerance."""
import ctypes
import math

import numpy as np
import pytest
import torch

from conftest import load_pkg
import guard_ref as G

pytestmark = pytest.mark.gpu

SIZES = [1, 0, 3, 4095, 8200, 4096, 5, 4097]
MISALIGNED, NO_GRAD, NO_EMA = (3, 4, 7), 6, 5
PAD = 4                                          # floats of padding on each side of a tensor (a misaligned one starts at float 1 of it)
COLS = ('p', 'g', 'm', 'v', 'e')
# (row, element): first element of row 0; last element of a short last chunk; first element after a chunk boundary; the last row
POSITIONS = {'row0-first': (0, 0), 'short-chunk-last': (4, 8199), 'after-boundary': (4, 4096), 'last-row': (7, 17)}
VALUES = {'nan': float('nan'), '+inf': float('inf'), '-inf': -float('inf'), '1e20': 1e20}


@pytest.fixture(scope='module')
def pkg():
    return load_pkg()


class Problem:
    """the tensors of the table on the GPU (``back[col][i]`` with padding, ``view[col][i]`` the tensor itself) and its device table"""

    def __init__(self, pkg, back=None):
        self.pkg = pkg
        if back is None:
            g = torch.Generator().manual_seed(20)
            back = {c: [] for c in COLS}
            for i, n in enumerate(SIZES):
                for c, scale in zip(COLS, (1.0, 0.1, 0.01, None, 1.0)):
                    t = torch.rand(n + 2 * PAD, generator=g) * 1e-3 if scale is None else torch.randn(n + 2 * PAD, generator=g) * scale
                    back[c].append(t.cuda())
        self.back = back
        off = lambda i: 1 if i in MISALIGNED else PAD
        self.view = {c: [back[c][i][off(i):off(i) + n] for i, n in enumerate(SIZES)] for c in COLS}
        rec = np.zeros(len(SIZES), dtype=pkg.optim._ROW)
        for i, n in enumerate(SIZES):
            for c, f in zip(COLS, ('p', 'g', 'exp_avg', 'exp_avg_sq', 'ema')):
                rec[f][i] = self.view[c][i].data_ptr()
                assert rec[f][i] % 16 == (4 if i in MISALIGNED else 0)
            rec['n'][i], rec['group'][i], rec['flags'][i] = n, i % 2, int(i == NO_GRAD)
        rec['ema'][NO_EMA] = 0
        counts = -(-rec['n'] // G.CHUNK)
        rec['chunk0'] = np.cumsum(counts) - counts
        self.rows = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).cuda()
        self.cmap = torch.from_numpy(np.repeat(np.arange(len(rec), dtype=np.int32), counts)).cuda()
        self.args = (pkg._lib.ptr(self.rows), pkg._lib.ptr(self.cmap), len(rec), int(self.cmap.numel()))
        groups = (pkg._lib.DcfOptimGroup * 2)()
        for k, (wd, mode) in enumerate(((0.05, 0), (0.01, 1))):                  # group 0 AdamW, group 1 Adam
            h = groups[k]
            h.lr, h.weight_decay, h.b1, h.b2, h.eps = 1e-3, wd, 0.9, 0.999, 1e-8
            h.one_minus_b1, h.one_minus_b2 = 1.0 - 0.9, 1.0 - 0.999
            h.bc1, h.sqrt_bc2 = 1.0 - 0.9 ** 3, math.sqrt(1.0 - 0.999 ** 3)
            h.mode = mode
        self.groups = groups

    def clone(self):
        return Problem(self.pkg, {c: [t.clone() for t in self.back[c]] for c in COLS})

    def bytes(self):
        return [t.clone().view(torch.int32) for c in COLS for t in self.back[c]]

    def host_table(self):
        return [(self.view['g'][i].cpu().numpy(), int(i == NO_GRAD)) for i in range(len(SIZES))]

    def run(self, max_norm, with_ema, guard=None):
        """norm + update, unguarded or under `guard` -> (norm, coef) as int32 bit patterns"""
        lib, L = self.pkg._lib.lib(), self.pkg._lib
        out = torch.full((2,), 7.0, device='cuda')
        outs, st, gr = (ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(out.data_ptr() + 4)), L.current_stream(), ctypes.cast(self.groups, ctypes.c_void_p)
        if guard is None:
            L.check(lib.dcf_optim_grad_norm(*self.args, max_norm, *outs, st), 'dcf_optim_grad_norm')
            L.check(lib.dcf_optim_adam_step(*self.args, gr, 2, outs[1], with_ema, 0.999, st), 'dcf_optim_adam_step')
        else:
            s = guard._on(guard.device)
            L.check(lib.dcf_guard_grad_norm(*self.args, max_norm, *outs, s, st), 'dcf_guard_grad_norm')
            L.check(lib.dcf_guard_adam_step(*self.args, gr, 2, outs[1], s, with_ema, 0.999, st), 'dcf_guard_adam_step')
        torch.cuda.synchronize()
        return out.cpu().view(torch.int32).tolist()


def same(a, b):
    return all(torch.equal(u, v) for u, v in zip(a, b))


def record(pkg, guard):
    rec = guard._state.cpu().numpy().view(pkg.optim._GUARD)[0]
    return {k: int(rec[k]) for k in G.FIELDS}


@pytest.fixture(scope='module')
def base(pkg):
    return Problem(pkg)


@pytest.mark.parametrize('max_norm', [1.0, 0.0])
@pytest.mark.parametrize('with_ema', [1, 0])
def test_finite_gradients_give_the_unguarded_bits(pkg, base, with_ema, max_norm):
    plain, guarded = base.clone(), base.clone()
    before = plain.bytes()
    guard = pkg.optim.StepGuard('cuda')
    want, got = plain.run(max_norm, with_ema), guarded.run(max_norm, with_ema, guard)
    assert got == want and math.isfinite(torch.tensor(got, dtype=torch.int32).view(torch.float32)[0])
    assert same(plain.bytes(), guarded.bytes()) and not same(before, guarded.bytes())
    assert record(pkg, guard) == G.judge(base.host_table(), G.fresh_state())
    rep = guard.report()
    assert (rep['verdict'], rep['applied'], rep['skipped'], rep['first_bad'], rep['last_skipped_attempt']) == (0, 1, 0, None, -1)


@pytest.mark.parametrize('value', VALUES)
@pytest.mark.parametrize('where', POSITIONS)
def test_one_bad_value_skips_and_nothing_moves(pkg, base, where, value):
    row, at = POSITIONS[where]
    prob = base.clone()
    prob.view['g'][row][at] = VALUES[value]
    before = prob.bytes()
    guard = pkg.optim.StepGuard('cuda').load_counters(3, 1)
    norm, coef = prob.run(1.0, 1, guard)
    assert coef == 0, f'coef bits {coef:#x}: +0 on a skip'
    assert not math.isfinite(float(torch.tensor([norm], dtype=torch.int32).view(torch.float32)))
    assert same(before, prob.bytes()), 'a skipped update wrote something'
    want = G.judge(prob.host_table(), G.fresh_state(3, 1))
    assert want['verdict'] == 1 and (want['first_bad_row'], want['n_bad_rows'], want['skipped'], want['last_skipped_attempt']) == (row, 1, 2, 4)
    assert record(pkg, guard) == want
    assert guard.report(names=[f'w{i}' for i in range(len(SIZES))])['first_bad'] == f'w{row}'


def test_two_bad_rows_and_a_bad_value_in_the_no_grad_row(pkg, base):
    prob = base.clone()
    prob.view['g'][NO_GRAD][2] = float('nan')
    plain = prob.clone()
    guard = pkg.optim.StepGuard('cuda')
    assert prob.run(1.0, 1, guard) == plain.run(1.0, 1) and same(prob.bytes(), plain.bytes())
    assert record(pkg, guard) == G.judge(prob.host_table(), G.fresh_state()) and record(pkg, guard)['verdict'] == 0
    prob.view['g'][7][4096] = float('inf')
    prob.view['g'][2][1] = 1e20
    before = prob.bytes()
    prob.run(0.0, 0, guard)
    want = G.judge(prob.host_table(), G.fresh_state(1, 0))
    assert (want['first_bad_row'], want['n_bad_rows']) == (2, 2) and record(pkg, guard) == want and same(before, prob.bytes())


def test_finite_again_after_a_skip_applies(pkg, base):
    prob = base.clone()
    good = prob.view['g'][4][8199].clone()
    prob.view['g'][4][8199] = float('nan')
    guard = pkg.optim.StepGuard('cuda')
    before = prob.bytes()
    prob.run(1.0, 1, guard)
    assert same(before, prob.bytes()) and record(pkg, guard)['verdict'] == 1
    prob.view['g'][4][8199] = good
    plain = prob.clone()
    assert prob.run(1.0, 1, guard) == plain.run(1.0, 1)
    assert same(prob.bytes(), plain.bytes()) and not same(before, prob.bytes())
    assert record(pkg, guard) == dict(verdict=0, first_bad_row=4, n_bad_rows=1, applied=1, skipped=1, last_skipped_attempt=0, conv_flag=0)


def test_the_conv_gradient_word_under_an_armed_guard(pkg, base):
    """dcf_op_conv_bwd_weight at its smallest admitted shape (Cin = N = 32, k = 1, one sequence of 64 rows) with one NaN in dY"""
    lib, L = pkg._lib.lib(), pkg._lib
    g = torch.Generator().manual_seed(5)
    X, dY = torch.randn(64, 32, generator=g).cuda(), torch.randn(64, 32, generator=g).cuda()
    bad = dY.clone()
    bad[7, 3] = float('nan')
    mask = torch.ones(64, dtype=torch.uint8, device='cuda')
    dW, db = torch.empty(32, 1, 32, device='cuda'), torch.empty(32, device='cuda')

    def conv(dy):
        rc = lib.dcf_op_conv_bwd_weight(L.ptr(X), L.ptr(mask), L.ptr(dy), L.ptr(dW), L.ptr(db), 1, 64, 32, 32, 1, 0, L.current_stream())
        torch.cuda.synchronize()
        return rc

    guard, other = pkg.optim.StepGuard('cuda'), pkg.optim.StepGuard('cuda')
    prob = base.clone()
    plain = prob.clone()
    try:
        assert conv(dY) == 0
        guard.arm()
        assert conv(bad) == 0 and not bool(torch.isfinite(dW).all())
        assert conv(dY) == 0 and conv(dY) == 0, 'armed: the next conv-gradient calls succeed'
        assert bool(torch.isfinite(dW).all())
        before = prob.bytes()
        assert other.armed is False and prob.run(1.0, 1, other)[1] != 0           # a guard that is not the armed one does not see the word
        assert record(pkg, other)['verdict'] == 0 and not same(before, prob.bytes())
        prob = base.clone()
        norm, coef = prob.run(1.0, 1, guard)
        assert coef == 0 and norm == plain.clone().run(1.0, 1)[0], 'finite gradients: the norm is the unguarded one, the coefficient +0'
        assert same(before, prob.bytes())
        assert record(pkg, guard) == dict(verdict=1, first_bad_row=-1, n_bad_rows=0, applied=0, skipped=1, last_skipped_attempt=0, conv_flag=1)
        assert record(pkg, guard) == G.judge(prob.host_table(), G.fresh_state(), conv_word=1)
        assert prob.run(1.0, 1, guard) == plain.run(1.0, 1) and same(prob.bytes(), plain.bytes()), 'the word is clear afterwards'
        assert record(pkg, guard)['verdict'] == 0 and record(pkg, guard)['applied'] == 1
        guard.disarm()
        assert conv(dY) == 0, 'nothing was left pending'
        assert conv(bad) == 0                                                     # disarmed: the word reaches the host ...
        assert conv(dY) == -1                                                     # ... and the next call fails, once
        msg = lib.dcf_last_error().decode()
        assert 'dcf_op_conv_bwd_weight' in msg and 'earlier gradient call' in msg and 'non-finite' in msg, msg
        assert conv(dY) == 0
    finally:                                                                      # leave the process as it was found
        guard.disarm()
        torch.cuda.synchronize()
        conv(dY), conv(dY)


def test_argument_checks(pkg, base):
    lib, st = pkg._lib.lib(), pkg._lib.current_stream()
    guard = pkg.optim.StepGuard('cuda')
    s = guard._on(guard.device)
    out = torch.zeros(2, device='cuda')
    o = (pkg._lib.ptr(out), ctypes.c_void_p(out.data_ptr() + 4))
    assert lib.dcf_guard_grad_norm(None, None, 0, 0, 1.0, *o, s, st) == 0        # no chunks: the norm is 0 and the attempt counts
    torch.cuda.synchronize()
    assert out.tolist() == [0.0, 1.0] and record(pkg, guard)['applied'] == 1
    assert lib.dcf_guard_adam_step(None, None, 0, 0, None, 0, None, s, 1, 0.5, st) == 0
    for call, word in ((lambda: lib.dcf_guard_grad_norm(*base.args, 1.0, *o, None, st), 'null state'),
                       (lambda: lib.dcf_guard_grad_norm(*base.args, 1.0, *o, ctypes.c_void_p(guard._state.data_ptr() + 4), st), '8-byte'),
                       (lambda: lib.dcf_guard_grad_norm(None, None, 1, 1, 1.0, *o, s, st), 'null table'),
                       (lambda: lib.dcf_guard_adam_step(*base.args, None, 0, None, None, 1, 0.5, st), 'null state'),
                       (lambda: lib.dcf_guard_adam_step(*base.args, None, 0, None, s, 1, 0.5, st), 'no groups'),
                       (lambda: lib.dcf_guard_adam_step(None, None, -1, 0, None, 0, None, s, 1, 0.5, st), 'negative'),
                       (lambda: lib.dcf_guard_arm(None, st), 'null state')):
        assert call() == -1
        msg = lib.dcf_last_error().decode()
        assert 'dcf_guard_' in msg and word in msg, msg
    torch.cuda.synchronize()
    assert record(pkg, guard)['applied'] == 1
