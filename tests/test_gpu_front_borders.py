"""tests/test_gpu_borders.py for the training-front-end extension: both operators of ``_lib.FRONT_SIGNATURES`` on operands between
poisoned borders (tests/arena.py) at the shapes of tests/front_abi_cases.py -- a plain run, an arena run per fill; outputs bit-identical,
borders and inputs untouched.  GPU only; no tolerance anywhere."""
import pytest

import arena
import front_abi_cases
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


@pytest.mark.parametrize('case', front_abi_cases.CASES, ids=[f'{c.export}-{c.tag}' for c in front_abi_cases.CASES])
def test_front_export_between_poisoned_borders(ctx, case):
    specs, call = case.make()

    def run(v):
        rc = call(ctx, v)
        ctx.pkg._lib.check(rc, case.export)    # a non-zero return code raises with dcf_last_error()
        return rc

    arena.run_three_ways(specs, run, 'cuda')


def test_every_front_export_has_a_case():
    """every name of the extension's table has a poisoned-border case or is the version function"""
    pkg = load_pkg()
    names = list(pkg._lib.FRONT_SIGNATURES)
    covered = {c.export for c in front_abi_cases.CASES}
    assert set(front_abi_cases.EXCLUDED) == {'dcf_front_ext_version'}
    missing = [n for n in names if n not in covered and n not in front_abi_cases.EXCLUDED]
    assert not missing, f'front-end exports without a case: {missing}'
    stale = [n for n in covered if n not in pkg._lib.FRONT_SIGNATURES]
    assert not stale, f'not in FRONT_SIGNATURES: {stale}'
    ids = [f'{c.export}-{c.tag}' for c in front_abi_cases.CASES]
    assert len(set(ids)) == len(ids)
