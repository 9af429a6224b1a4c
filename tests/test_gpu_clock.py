"""GPU checks of the step-count extension at operator level (include/decafnet_hip_clock.h, csrc/optim_clock.hip), through the C ABI, on
the eight-row table of tests/test_gpu_guard.py (its ``Problem`` imported) -- 1, 0, 3, 4095, 8200, 4096, 5 (DCF_OPTIM_NO_GRAD) and 4097
elements, three rows starting 4 bytes past a 16-byte boundary, one without an EMA copy -- with group 0 AdamW at betas (0.9, 0.999),
group 1 Adam at betas (0.8, 0.99) and the start counts 0, 2, 2, 7, 11, 0, 5, 100000: every row that has a gradient has a (group, count)
pair of its own, the last one past the end of its group's table.

1. no guard: every tensor equals dcf_optim_adam_step run on copies, once per (group, count) pair on a table of that pair's rows with
   the host's by-value corrections (the NO_GRAD row in a launch of its own: its EMA copy moves); the counts are + 1 on the rows that
   have a gradient, the n = 0 row included, and unchanged on the NO_GRAD row.
2. verdict skip (a dcf_guard_grad_norm over one +inf first): every byte of every tensor, of its padding and of ``steps`` is what it was.
3. verdict apply after that skip: equals check 1 started from the same state.
4. argument refusals carry a message and launch nothing.

Bit-exact throughout: no tolerance."""
import ctypes
import math

import numpy as np
import pytest
import torch

from conftest import load_pkg
import clock_ref as C
import guard_ref as G
from test_gpu_guard import COLS, NO_EMA, NO_GRAD, SIZES, Problem, same

pytestmark = pytest.mark.gpu

BETAS = ((0.9, 0.999), (0.8, 0.99))
HYPER = ((0.05, 0), (0.01, 1))                   # (weight_decay, mode): group 0 AdamW, group 1 Adam
START = [0, 2, 2, 7, 11, 0, 5, 100000]
LR, EPS, COEF, EMA_BETA = 1e-3, 1e-8, 0.37, 0.999


@pytest.fixture(scope='module')
def pkg():
    return load_pkg()


def group_record(h, k, bc):
    """group k's record; bc = (bc1, sqrt_bc2) as doubles, or None: NaN there, which dcf_clock_adam_step must not read"""
    b1, b2 = BETAS[k]
    h.lr, h.weight_decay, h.b1, h.b2, h.eps = LR, HYPER[k][0], b1, b2, EPS
    h.one_minus_b1, h.one_minus_b2 = 1.0 - b1, 1.0 - b2
    h.bc1, h.sqrt_bc2 = bc if bc is not None else (float('nan'), float('nan'))
    h.mode = HYPER[k][1]


class Clock:
    """what dcf_clock_adam_step takes besides the table: the two group records, the uploaded tables, the counts, the coefficient"""

    def __init__(self, pkg, counts=START):
        self.pkg = pkg
        self.groups = (pkg._lib.DcfOptimGroup * 2)()
        for k in range(2):
            group_record(self.groups[k], k, None)
        self.host_tables = [pkg.optim.bias_correction_table(*b) for b in BETAS]
        assert len(self.host_tables[1]) < START[7] and all(c < len(self.host_tables[i % 2]) for i, c in enumerate(START[:7]))
        self.tables = [torch.from_numpy(t.reshape(-1).copy()).cuda() for t in self.host_tables]
        self.bc = (ctypes.c_void_p * 2)(*[t.data_ptr() for t in self.tables])
        self.len = (ctypes.c_int32 * 2)(*[len(t) for t in self.host_tables])
        self.steps = torch.tensor(counts, dtype=torch.int64).cuda()
        self.coef = torch.tensor([COEF], device='cuda')

    def call(self, prob, state=None, with_ema=1, **over):
        L = self.pkg._lib
        a = dict(groups=ctypes.cast(self.groups, ctypes.c_void_p), n_groups=2, bc=ctypes.cast(self.bc, ctypes.c_void_p),
                 len=ctypes.cast(self.len, ctypes.c_void_p), steps=L.ptr(self.steps), args=prob.args)
        a.update(over)
        rc = L.lib().dcf_clock_adam_step(*a['args'], a['groups'], a['n_groups'], a['bc'], a['len'], a['steps'], L.ptr(self.coef), state, with_ema,
                                         EMA_BETA, L.current_stream())
        torch.cuda.synchronize()
        return rc


def reference(pkg, prob, counts, with_ema=1):
    """dcf_optim_adam_step on `prob` (in place), once per (group, count) pair on a table of that pair's rows, with the corrections the
    host path passes by value; the NO_GRAD row in a launch of its own"""
    L, lib = pkg._lib, pkg._lib.lib()
    coef = torch.tensor([COEF], device='cuda')
    keys = {}
    for i in range(len(SIZES)):
        keys.setdefault(('no-grad',) if i == NO_GRAD else (i % 2, counts[i] + 1), []).append(i)
    full = prob.rows.cpu().numpy().view(pkg.optim._ROW)
    for key, rows in keys.items():
        rec = full[rows].copy()
        n_chunks = -(-rec['n'] // G.CHUNK)
        rec['chunk0'], rec['group'] = np.cumsum(n_chunks) - n_chunks, 0
        table = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).cuda()
        cmap = torch.from_numpy(np.repeat(np.arange(len(rec), dtype=np.int32), n_chunks)).cuda()
        group = (L.DcfOptimGroup * 1)()
        if key[0] == 'no-grad':
            group_record(group[0], NO_GRAD % 2, (1.0, 1.0))
        else:
            k, t = key
            group_record(group[0], k, (1.0 - BETAS[k][0] ** t, math.sqrt(1.0 - BETAS[k][1] ** t)))
        if int(cmap.numel()):
            L.check(lib.dcf_optim_adam_step(L.ptr(table), L.ptr(cmap), len(rec), int(cmap.numel()), ctypes.cast(group, ctypes.c_void_p), 1,
                                            L.ptr(coef), with_ema, EMA_BETA, L.current_stream()), 'dcf_optim_adam_step')
        torch.cuda.synchronize()
    return [c + int(i != NO_GRAD) for i, c in enumerate(counts)]


@pytest.fixture(scope='module')
def base(pkg):
    return Problem(pkg)


def test_the_table_has_a_pair_of_its_own_for_every_row(pkg):
    pairs = {(i % 2, START[i] + 1) for i in range(len(SIZES)) if i != NO_GRAD}
    assert len(pairs) == len(SIZES) - 1 and SIZES[1] == 0 and SIZES[NO_GRAD] == 5
    clock = Clock(pkg)
    for i, c in enumerate(START):                        # what the kernel reads is what the host path would pass
        assert C.from_table(clock.host_tables[i % 2], c + 1) == C.corrections(*BETAS[i % 2], c + 1), i


@pytest.mark.parametrize('with_ema', [1, 0])
def test_without_a_guard_every_row_steps_at_its_own_count(pkg, base, with_ema):
    got, want = base.clone(), base.clone()
    before = got.bytes()
    clock = Clock(pkg)
    assert clock.call(got, None, with_ema) == 0, pkg._lib.lib().dcf_last_error()
    counts = reference(pkg, want, START, with_ema)
    diff = [i for i, (u, v) in enumerate(zip(got.bytes(), want.bytes())) if not torch.equal(u, v)]
    assert not diff, f'backing buffers {diff} differ (buffer = column * {len(SIZES)} + row, columns {COLS})'
    assert not same(before, got.bytes())
    assert clock.steps.tolist() == counts == [1, 3, 3, 8, 12, 1, 5, 100001]
    for c in ('p', 'm', 'v'):                            # the NO_GRAD row keeps p and both moments; its EMA copy moved with with_ema
        assert torch.equal(got.view[c][NO_GRAD], base.view[c][NO_GRAD])
    assert torch.equal(got.view['e'][NO_GRAD], base.view['e'][NO_GRAD]) == (not with_ema)
    assert torch.equal(got.view['e'][NO_EMA], base.view['e'][NO_EMA])


def test_a_skip_writes_nothing_and_the_next_apply_steps_from_the_same_counts(pkg, base):
    prob = base.clone()
    good = prob.view['g'][4][8199].clone()
    prob.view['g'][4][8199] = float('inf')
    guard = pkg.optim.StepGuard('cuda')
    s = guard._on(guard.device)
    out = torch.zeros(2, device='cuda')
    norm = lambda: pkg._lib.check(pkg._lib.lib().dcf_guard_grad_norm(*prob.args, 1.0, pkg._lib.ptr(out), ctypes.c_void_p(out.data_ptr() + 4), s,
                                                                     pkg._lib.current_stream()), 'dcf_guard_grad_norm')
    clock = Clock(pkg)
    norm()
    before = prob.bytes()
    assert clock.call(prob, s) == 0
    assert guard.report()['verdict'] == 1
    assert same(before, prob.bytes()), 'a skipped update wrote something'
    assert clock.steps.tolist() == START, 'a skipped update advanced a count'
    prob.view['g'][4][8199] = good
    want = prob.clone()
    norm()
    assert clock.call(prob, s) == 0
    rep = guard.report()
    assert (rep['verdict'], rep['applied'], rep['skipped']) == (0, 1, 1)
    counts = reference(pkg, want, START)
    assert same(prob.bytes(), want.bytes()) and not same(before, prob.bytes())
    assert clock.steps.tolist() == counts


def test_two_launches_in_a_row_read_the_counts_the_first_one_left(pkg, base):
    got, want = base.clone(), base.clone()
    clock = Clock(pkg)
    assert clock.call(got) == 0 and clock.call(got) == 0
    counts = reference(pkg, want, reference(pkg, want, START))
    assert same(got.bytes(), want.bytes()) and clock.steps.tolist() == counts == [c + 2 * int(i != NO_GRAD) for i, c in enumerate(START)]


def test_argument_checks(pkg, base):
    lib = pkg._lib.lib()
    prob, clock = base.clone(), Clock(pkg)
    before = prob.bytes()
    neg = (ctypes.c_int32 * 2)(len(clock.host_tables[0]), -1)
    nullt = (ctypes.c_void_p * 2)(clock.tables[0].data_ptr(), None)
    nine = (pkg._lib.DcfOptimGroup * 9)()
    bad_mode = (pkg._lib.DcfOptimGroup * 2)()
    for k in range(2):
        group_record(bad_mode[k], k, None)
    bad_mode[1].mode = 7
    cases = ((dict(steps=None), 'null steps'),
             (dict(bc=None), 'null bc_tables'),
             (dict(len=None), 'null bc_tables'),
             (dict(len=ctypes.cast(neg, ctypes.c_void_p)), 'negative bc_len'),
             (dict(bc=ctypes.cast(nullt, ctypes.c_void_p)), 'null bc_tables entry'),
             (dict(steps=ctypes.c_void_p(clock.steps.data_ptr() + 4)), '8-byte'),
             (dict(groups=None, n_groups=0), 'no groups'),
             (dict(groups=None), 'null groups'),
             (dict(groups=ctypes.cast(nine, ctypes.c_void_p), n_groups=9), 'at most 8'),
             (dict(groups=ctypes.cast(bad_mode, ctypes.c_void_p)), 'unknown mode'),
             (dict(args=(None, None, len(SIZES), prob.args[3])), 'null table'),
             (dict(args=(None, None, len(SIZES), 0)), 'null table'),
             (dict(args=(prob.args[0], prob.args[1], -1, 0)), 'negative'))
    for over, word in cases:
        assert clock.call(prob, **over) == -1, over
        msg = lib.dcf_last_error().decode()
        assert 'dcf_clock_adam_step' in msg and word in msg, (over, msg)
    assert same(before, prob.bytes()) and clock.steps.tolist() == START, 'a refused call launched something'
    assert clock.call(prob, args=(None, None, 0, 0), steps=None, bc=None, len=None, groups=None, n_groups=0) == 0      # nothing to do
    # no chunks but rows: the counts of the rows that have a gradient still advance (here: rows of zero elements)
    rec = np.zeros(3, dtype=pkg.optim._ROW)
    rec['flags'][1] = pkg._lib.OPTIM_NO_GRAD
    rows = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).cuda()
    small = Clock(pkg, [4, 5, 6])
    assert small.call(prob, args=(pkg._lib.ptr(rows), None, 3, 0), bc=None, len=None) == 0, lib.dcf_last_error()
    assert small.steps.tolist() == [5, 5, 7]
    assert same(before, prob.bytes())
