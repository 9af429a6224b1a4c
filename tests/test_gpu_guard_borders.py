"""tests/test_gpu_borders.py for the step-guard extension: the two table exports of ``_lib.GUARD_SIGNATURES`` on operands between
poisoned borders (tests/arena.py) at the shapes of tests/guard_abi_cases.py -- a plain run, an arena run per fill; outputs bit-identical,
borders and inputs untouched; then the plain run's record against the restatement (tests/guard_ref.py) and, under the skip verdict,
every parameter, moment and EMA tensor against the bits that went in.  GPU only; no tolerance anywhere."""
import pytest

import arena
import guard_abi_cases
from conftest import load_pkg

pytestmark = pytest.mark.gpu


class Ctx:
    def __init__(self):
        self.pkg = load_pkg()
        self.lib = self.pkg._lib.lib()          # raises if the .so is missing: no silent fallback

    def stream(self):
        return self.pkg._lib.current_stream()


@pytest.fixture(scope='module')
def ctx():
    return Ctx()


@pytest.mark.parametrize('case', guard_abi_cases.CASES, ids=[f'{c.export}-{c.tag}' for c in guard_abi_cases.CASES])
def test_guard_export_between_poisoned_borders(ctx, case):
    specs, call, fixup, verify = case.make()

    def run(v):
        rc = call(ctx, v)
        ctx.pkg._lib.check(rc, case.export)    # a non-zero return code raises with dcf_last_error()
        return rc

    plain = arena.run_three_ways(specs, run, 'cuda', fixup)
    C = guard_abi_cases
    got = verify(plain)
    if case.export == 'dcf_guard_grad_norm':
        assert got == int('inf' in case.tag)
    else:                                       # p, both moments and the EMA copy of every row that has them, or nothing at all
        live = [i for i, n in enumerate(C.SIZES) if n]
        moved = 3 * sum(i != C.NO_GRAD for i in live) + sum(i != C.NO_EMA for i in live)
        assert got == (0 if 'skip' in case.tag else moved)


def test_every_guard_export_has_a_case():
    """every name of the extension's table has a poisoned-border case or a reason why it has none"""
    pkg = load_pkg()
    names = list(pkg._lib.GUARD_SIGNATURES)
    covered = {c.export for c in guard_abi_cases.CASES}
    assert set(guard_abi_cases.EXCLUDED) == {'dcf_guard_ext_version', 'dcf_guard_arm', 'dcf_guard_disarm'}
    missing = [n for n in names if n not in covered and n not in guard_abi_cases.EXCLUDED]
    assert not missing, f'guard exports without a case: {missing}'
    stale = [n for n in covered if n not in pkg._lib.GUARD_SIGNATURES]
    assert not stale, f'not in GUARD_SIGNATURES: {stale}'
