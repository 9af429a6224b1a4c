"""GPU checks, in one process, of dcf_guard_word_publish / dcf_guard_word_merge (include/decafnet_hip_fit.h, csrc/fit.hip): the
conv-gradient word of the armed guard made known to the other ranks through one float.  The word is raised the way
tests/test_gpu_guard.py raises it (dcf_op_conv_bwd_weight at its smallest shape with an inf in dY); the guarded norm and update run
on that file's ``Problem``.

1. Armed and clear: the slot is 0.0.  After a raising conv-gradient call: the slot is 1.0 and the word is still set (a second publish
   says so again).
2. Merge with a slot of 0 changes nothing: the guarded norm that follows applies.  Merge with a slot of 1.0 (and 2.0, and NaN) on a
   clear word, then a guarded norm on finite gradients: the verdict is skip, ``conv_flag == DCF_GUARD_REMOTE``, no parameter byte moved;
   the norm after that applies -- the word was consumed.  A local word and a remote flag together give ``conv_flag == 1 | REMOTE``.
3. An unarmed state, a null or misaligned slot: refused with the export's name, nothing written."""
import ctypes

import pytest
import torch

from conftest import load_pkg
from test_gpu_guard import Problem, record, same

pytestmark = pytest.mark.gpu
UNWRITTEN = -7.0


@pytest.fixture(scope='module')
def pkg():
    return load_pkg()


@pytest.fixture(scope='module')
def base(pkg):
    return Problem(pkg)


class Conv:
    """dcf_op_conv_bwd_weight at its smallest admitted shape; ``raise_word()`` runs it with one inf in dY"""

    def __init__(self, pkg):
        self.lib, self.L = pkg._lib.lib(), pkg._lib
        g = torch.Generator().manual_seed(5)
        self.X, self.dY = torch.randn(64, 32, generator=g).cuda(), torch.randn(64, 32, generator=g).cuda()
        self.bad = self.dY.clone()
        self.bad[7, 3] = float('inf')
        self.dW = torch.empty(32, 1, 32, device='cuda')

    def __call__(self, dy=None):
        L = self.L
        rc = self.lib.dcf_op_conv_bwd_weight(L.ptr(self.X), None, L.ptr(self.dY if dy is None else dy), L.ptr(self.dW), None, 1, 64, 32, 32, 1, 0,
                                             L.current_stream())
        torch.cuda.synchronize()
        return rc

    def raise_word(self):
        assert self(self.bad) == 0 and not bool(torch.isfinite(self.dW).all())


def publish(pkg, guard, slot):
    L = pkg._lib
    L.check(L.lib().dcf_guard_word_publish(guard._on(guard.device), L.ptr(slot), L.current_stream()), 'dcf_guard_word_publish')
    torch.cuda.synchronize()
    return float(slot[0])


def merge(pkg, guard, value):
    L = pkg._lib
    slot = torch.tensor([value], device='cuda')
    L.check(L.lib().dcf_guard_word_merge(guard._on(guard.device), L.ptr(slot), L.current_stream()), 'dcf_guard_word_merge')
    torch.cuda.synchronize()
    assert torch.equal(slot.cpu().view(torch.int32), torch.tensor([value]).view(torch.int32)), 'merge only reads the slot'


def test_publish_says_whether_the_word_is_set_and_leaves_it(pkg, base):
    conv, guard = Conv(pkg), pkg.optim.StepGuard('cuda')
    pair = torch.full((2,), UNWRITTEN, device='cuda')                             # the slot is element 1 of [norm, flag]
    try:
        assert conv() == 0
        guard.arm()
        assert publish(pkg, guard, pair[1:]) == 0.0 and float(pair[0]) == UNWRITTEN
        conv.raise_word()
        assert publish(pkg, guard, pair[1:]) == 1.0 and float(pair[0]) == UNWRITTEN
        assert publish(pkg, guard, pair[1:]) == 1.0, 'publish does not clear the word'
        prob = base.clone()
        before = prob.bytes()
        assert prob.run(1.0, 1, guard)[1] == 0 and same(before, prob.bytes())      # the guarded norm still finds it, and consumes it
        assert record(pkg, guard)['conv_flag'] == 1 and record(pkg, guard)['verdict'] == 1
        assert publish(pkg, guard, pair[1:]) == 0.0
    finally:
        guard.disarm()
        torch.cuda.synchronize()
        conv(), conv()


@pytest.mark.parametrize('flag', [1.0, 2.0, float('nan')], ids=['one', 'two', 'nan'])
def test_merge_makes_the_next_guarded_norm_skip(pkg, base, flag):
    REMOTE = pkg._lib.GUARD_REMOTE
    conv, guard = Conv(pkg), pkg.optim.StepGuard('cuda')
    plain = base.clone()
    want = plain.run(1.0, 1)
    try:
        guard.arm()
        prob = base.clone()
        merge(pkg, guard, 0.0)                                                     # nothing raised anywhere: nothing changes
        assert prob.run(1.0, 1, guard) == want and same(prob.bytes(), plain.bytes())
        assert record(pkg, guard) == dict(verdict=0, first_bad_row=-1, n_bad_rows=0, applied=1, skipped=0, last_skipped_attempt=-1, conv_flag=0)
        prob = base.clone()
        before = prob.bytes()
        merge(pkg, guard, flag)                                                    # raised on another rank
        norm, coef = prob.run(1.0, 1, guard)
        assert coef == 0 and norm == want[0], 'finite gradients: the norm is the unguarded one, the coefficient +0'
        assert same(before, prob.bytes()), 'a skipped update wrote something'
        assert record(pkg, guard) == dict(verdict=1, first_bad_row=-1, n_bad_rows=0, applied=1, skipped=1, last_skipped_attempt=1, conv_flag=REMOTE)
        assert guard.report()['conv_flag'] == REMOTE
        assert prob.run(1.0, 1, guard) == want and same(prob.bytes(), plain.bytes()), 'the word is clear afterwards'
        conv.raise_word()                                                          # this rank and another one
        merge(pkg, guard, flag)
        prob = base.clone()
        assert prob.run(1.0, 1, guard)[1] == 0 and same(before, prob.bytes())
        assert record(pkg, guard)['conv_flag'] == 1 | REMOTE
    finally:
        guard.disarm()
        torch.cuda.synchronize()
        conv(), conv()


def test_an_unarmed_state_and_a_bad_slot_are_refused(pkg):
    L = pkg._lib
    lib, st = L.lib(), L.current_stream()
    guard, other = pkg.optim.StepGuard('cuda'), pkg.optim.StepGuard('cuda')
    slot = torch.full((2,), UNWRITTEN, device='cuda')
    state = lambda g: g._on(g.device)

    def refused(fn, *args):
        assert fn(*args, st) != 0
        return lib.dcf_last_error().decode()

    for fn, name in ((lib.dcf_guard_word_publish, 'dcf_guard_word_publish'), (lib.dcf_guard_word_merge, 'dcf_guard_word_merge')):
        msg = refused(fn, state(guard), L.ptr(slot))
        assert name in msg and 'armed' in msg, msg                                 # nobody is armed
    try:
        guard.arm()
        for fn, name in ((lib.dcf_guard_word_publish, 'dcf_guard_word_publish'), (lib.dcf_guard_word_merge, 'dcf_guard_word_merge')):
            assert name in refused(fn, state(other), L.ptr(slot)) and 'armed' in lib.dcf_last_error().decode()    # another guard is
            assert name in refused(fn, None, L.ptr(slot))
            assert name in refused(fn, state(guard), None)
            assert name in refused(fn, state(guard), ctypes.c_void_p(slot.data_ptr() + 2))
        torch.cuda.synchronize()
        assert bool((slot == UNWRITTEN).all())
        assert lib.dcf_guard_word_publish(state(guard), L.ptr(slot), st) == 0
        torch.cuda.synchronize()
        assert slot.tolist() == [0.0, UNWRITTEN]
    finally:
        guard.disarm()
        torch.cuda.synchronize()
