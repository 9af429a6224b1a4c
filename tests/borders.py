"""The driver of the poisoned-border tests (tests/test_gpu_borders.py and one tests/test_gpu_<key>_borders.py per extension, each two
assignments long) and of tools/abi_digest.py: the context a case's call gets, the run of one case, the table that maps every key of
``_lib.EXTENSIONS`` to its case module, to what is asserted of the plain run of its cases beyond the bits and to what its case table
is pinned to, and the two tests a border file is made of."""
import ctypes
from collections import namedtuple

import pytest
import torch

import abi_cases
import arena
import attn_abi_cases
import clock_abi_cases
import dist_abi_cases
import front_abi_cases
import front_half_abi_cases
import guard_abi_cases
import half_abi_cases
import train_abi_cases
from conftest import load_pkg


class Ctx:
    """what a case's call gets: the package, the library, the current stream and the models kept until close()"""

    def __init__(self):
        self.pkg = load_pkg()
        self.lib = self.pkg._lib.lib()          # raises if the .so is missing: no silent fallback
        self._models = {}

    def stream(self):
        return self.pkg._lib.current_stream()

    def model(self, key, factory):
        """factory() -> (a dcf_model handle, the bound weights: alive as long as the handle), of which the handle is returned and
        destroyed by close(); or a tuple that starts with a torch model, returned whole"""
        if key not in self._models:
            self._models[key] = factory()
        made = self._models[key]
        return made[0] if isinstance(made[0], ctypes.c_void_p) else made

    def close(self):
        torch.cuda.synchronize()
        for made in self._models.values():
            if isinstance(made[0], ctypes.c_void_p):
                self.lib.dcf_model_destroy(made[0])
        self._models.clear()


def run_case(ctx, case, after=None):
    """one case between poisoned borders: its debug options set around the three runs of arena.run_three_ways and reset to -1
    afterwards, every return code through _lib.check (non-zero raises with dcf_last_error()); then after(case, specs, plain, verify)
    on the outputs of the plain run, which are returned.  ``case.make()`` -> (specs, call[, fixup[, verify]])"""
    specs, call, fixup, verify = (tuple(case.make()) + (None, None))[:4]
    check = ctx.pkg._lib.check

    def run(v):
        rc = call(ctx, v)
        check(rc, case.export)
        return rc

    try:
        for name, value in case.options:
            check(ctx.lib.dcf_debug_set_option(name.encode(), value), 'dcf_debug_set_option')
        plain = arena.run_three_ways(specs, run, 'cuda', fixup)
    finally:
        for name, _ in case.options:
            check(ctx.lib.dcf_debug_set_option(name.encode(), -1), 'dcf_debug_set_option')
    if after is not None:
        after(case, specs, plain, verify)
    return plain


# ---------------------------------------------------------------------------------------------- what each extension adds to the bits
def _after_dist(case, specs, plain, verify):
    """the plain run's values against ``torch.mul`` and the poison between the destination slices"""
    C = dist_abi_cases
    assert verify(plain) == sum(C.SIZES) - C.SIZES[C.NO_GRAD] - C.SIZES[C.NULL_G]


def _moved(C, case, got):
    """p, both moments and the EMA copy of every row that has them, or nothing at all"""
    live = [i for i, n in enumerate(C.SIZES) if n]
    moved = 3 * sum(i != C.NO_GRAD for i in live) + sum(i != C.NO_EMA for i in live)
    assert got == (0 if 'skip' in case.tag else moved)


def _after_guard(case, specs, plain, verify):
    """the plain run's record against the restatement (tests/guard_ref.py); under the skip verdict every parameter, moment and EMA
    tensor against the bits that went in"""
    got = verify(plain)
    if case.export == 'dcf_guard_grad_norm':
        assert got == int('inf' in case.tag)
    else:
        _moved(guard_abi_cases, case, got)


def _after_clock(case, specs, plain, verify):
    """which tensors and which counts moved under verdict apply, and that none did under verdict skip"""
    roles = {name: role for name, _, role in specs}
    assert roles['steps'] == 'inout' and roles['bc0'] == roles['bc1'] == 'in'
    _moved(clock_abi_cases, case, verify(plain))


def _halves(specs):
    """the operands placed as the bytes of binary16 values: what surrounds them reads as half NaNs (fill 1) or zeros (fill 2)"""
    return [name for name, t, role, *rest in specs if rest and t.dtype == torch.uint8 and t.dim() == 2 and rest[0] == t.shape[-1]]


def _after_half(case, specs, plain, verify):
    assert _halves(specs), 'every case of this extension has a half operand'
    for name, t in plain.items():              # the plain run computed something: no sentinel left, nothing non-finite
        if t.is_floating_point():
            assert bool(torch.isfinite(t).all()), name


def _after_front_half(case, specs, plain, verify):
    halves = _halves(specs)
    assert 'vid' in halves and 'shallow' in halves, 'the features of every case of this extension are half operands'
    for name, t in plain.items():              # the plain run computed something: no sentinel left, nothing non-finite
        assert bool(torch.isfinite(t).all()), name


# key of _lib.EXTENSIONS -> its case module (CASES, EXCLUDED), the hook of run_case, and what the case table is pinned to: the names
# that may be excluded and, where a table pins them, its tags or the exports it covers (None: whatever the table holds).  The base
# table has the stricter rules of tests/test_gpu_borders.py.
Borders = namedtuple('Borders', 'cases after excluded tags covered', defaults=(None, None, None, None))


def _version(key):
    return {f'dcf_{key}_ext_version'}


TABLE = {
    'base': Borders(abi_cases),
    'train': Borders(train_abi_cases, None, _version('train')),
    'dist': Borders(dist_abi_cases, _after_dist, _version('dist')),
    'attn': Borders(attn_abi_cases, None, _version('attn')),
    'front': Borders(front_abi_cases, None, _version('front')),
    'guard': Borders(guard_abi_cases, _after_guard, _version('guard') | {'dcf_guard_arm', 'dcf_guard_disarm'}),
    'clock': Borders(clock_abi_cases, _after_clock, _version('clock'), tags={'nine-tensors-verdict-apply', 'nine-tensors-verdict-skip'}),
    'half': Borders(half_abi_cases, _after_half, _version('half'),
                    covered={'dcf_forward_eval_h', 'dcf_forward_eval_videos_h', 'dcf_op_linear_cm_split_h', 'dcf_op_linear_cm_split_ld_h',
                             'dcf_op_sidekick_h'}),
    'front_half': Borders(front_half_abi_cases, _after_front_half, _version('front_half'),
                          covered={'dcf_op_vidmap_shared_h', 'dcf_op_vidmap_shared_bwd_h'}),
}
NO_CASE_TABLE = {'embd': 'tests/test_gpu_embd_chain_borders.py builds its specs from parameters'}


# ---------------------------------------------------------------------------------------------- what a border test file is made of
@pytest.fixture(scope='module')
def ctx():
    c = Ctx()
    yield c
    c.close()


def export_test(key):
    """-> the test of every case of the key's table through run_case with the row's hook, ids ``<export>-<tag>``; the file that
    assigns it to a ``test_`` name imports the ``ctx`` fixture above"""
    row = TABLE[key]

    @pytest.mark.gpu
    @pytest.mark.parametrize('case', row.cases.CASES, ids=[f'{c.export}-{c.tag}' for c in row.cases.CASES])
    def test(ctx, case):
        run_case(ctx, case, row.after)
    return test


def completeness_test(key):
    """-> the test that every name of the extension's table has a poisoned-border case or a reason why it has none, and that the case
    table is what its row of TABLE pins it to"""
    @pytest.mark.gpu
    def test():
        ext = {e.key: e for e in load_pkg()._lib.EXTENSIONS}[key]
        row = TABLE[key]
        cases, excluded = row.cases.CASES, row.cases.EXCLUDED
        covered = {c.export for c in cases}
        assert set(excluded) == row.excluded
        assert all(isinstance(r, str) and r.strip() for r in excluded.values())
        missing = [n for n in ext.table if n not in covered and n not in excluded]
        assert not missing, f'{key} exports without a case: {missing}'
        stale = [n for n in list(covered) + list(excluded) if n not in ext.table]
        assert not stale, f'not in the {key} table: {stale}'
        assert row.tags is None or {c.tag for c in cases} == row.tags
        assert row.covered is None or covered == row.covered
        ids = [f'{c.export}-{c.tag}' for c in cases]
        assert len(set(ids)) == len(ids)
    return test
