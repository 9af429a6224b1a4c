"""tests/test_gpu_borders.py for the step-count extension: the table export of ``_lib.CLOCK_SIGNATURES`` on operands between poisoned
borders (tests/arena.py) at the shapes of tests/clock_abi_cases.py -- a plain run, an arena run per fill; outputs bit-identical, borders
and inputs (the bias-correction tables among them) untouched; then, on the plain run, which tensors and which counts moved under
verdict apply, and that none did under verdict skip.  GPU only; no tolerance anywhere."""
import pytest

import arena
import clock_abi_cases
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


@pytest.mark.parametrize('case', clock_abi_cases.CASES, ids=[f'{c.export}-{c.tag}' for c in clock_abi_cases.CASES])
def test_clock_export_between_poisoned_borders(ctx, case):
    specs, call, fixup, verify = case.make()
    roles = {name: role for name, _, role in specs}
    assert roles['steps'] == 'inout' and roles['bc0'] == roles['bc1'] == 'in'

    def run(v):
        rc = call(ctx, v)
        ctx.pkg._lib.check(rc, case.export)    # a non-zero return code raises with dcf_last_error()
        return rc

    plain = arena.run_three_ways(specs, run, 'cuda', fixup)
    C = clock_abi_cases
    got = verify(plain)                         # p, both moments and the EMA copy of every row that has them, or nothing at all
    live = [i for i, n in enumerate(C.SIZES) if n]
    moved = 3 * sum(i != C.NO_GRAD for i in live) + sum(i != C.NO_EMA for i in live)
    assert got == (0 if 'skip' in case.tag else moved)


def test_every_clock_export_has_a_case():
    """every name of the extension's table has a poisoned-border case or a reason why it has none"""
    pkg = load_pkg()
    names = list(pkg._lib.CLOCK_SIGNATURES)
    covered = {c.export for c in clock_abi_cases.CASES}
    assert set(clock_abi_cases.EXCLUDED) == {'dcf_clock_ext_version'}
    assert {c.tag for c in clock_abi_cases.CASES} == {'nine-tensors-verdict-apply', 'nine-tensors-verdict-skip'}
    missing = [n for n in names if n not in covered and n not in clock_abi_cases.EXCLUDED]
    assert not missing, f'clock exports without a case: {missing}'
    stale = [n for n in covered if n not in pkg._lib.CLOCK_SIGNATURES]
    assert not stale, f'not in CLOCK_SIGNATURES: {stale}'
