"""tests/test_gpu_borders.py for the half-feature training-front-end extension: both operators of ``_lib.FRONT_HALF_SIGNATURES`` on
operands between poisoned borders (tests/arena.py) at the shapes of tests/front_half_abi_cases.py -- a plain run, an arena run per fill;
outputs bit-identical, borders and inputs untouched.  The half operands lie in the arena as the bytes of their binary16 values, so what
surrounds them reads as half NaNs (fill 1) or zeros (fill 2).  GPU only; no tolerance anywhere."""
import pytest
import torch

import arena
import front_half_abi_cases
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


@pytest.mark.parametrize('case', front_half_abi_cases.CASES, ids=[f'{c.export}-{c.tag}' for c in front_half_abi_cases.CASES])
def test_front_half_export_between_poisoned_borders(ctx, case):
    specs, call = case.make()
    check = ctx.pkg._lib.check
    halves = [name for name, t, role, *rest in specs if rest and t.dtype == torch.uint8 and t.dim() == 2 and rest[0] == t.shape[-1]]
    assert 'vid' in halves and 'shallow' in halves, 'the features of every case of this extension are half operands'

    def run(v):
        rc = call(ctx, v)
        check(rc, case.export)                 # a non-zero return code raises with dcf_last_error()
        return rc

    try:
        for name, value in case.options:
            check(ctx.lib.dcf_debug_set_option(name.encode(), value), 'dcf_debug_set_option')
        plain = arena.run_three_ways(specs, run, 'cuda')
    finally:
        for name, _ in case.options:
            check(ctx.lib.dcf_debug_set_option(name.encode(), -1), 'dcf_debug_set_option')
    for name, t in plain.items():              # the plain run computed something: no sentinel left, nothing non-finite
        assert bool(torch.isfinite(t).all()), name


def test_every_front_half_export_has_a_case():
    """every name of the extension's table has a poisoned-border case or is the version function"""
    pkg = load_pkg()
    names = list(pkg._lib.FRONT_HALF_SIGNATURES)
    covered = {c.export for c in front_half_abi_cases.CASES}
    assert set(front_half_abi_cases.EXCLUDED) == {'dcf_front_half_ext_version'}
    missing = [n for n in names if n not in covered and n not in front_half_abi_cases.EXCLUDED]
    assert not missing, f'half front-end exports without a case: {missing}'
    stale = [n for n in covered if n not in pkg._lib.FRONT_HALF_SIGNATURES]
    assert not stale, f'not in FRONT_HALF_SIGNATURES: {stale}'
    assert covered == {'dcf_op_vidmap_shared_h', 'dcf_op_vidmap_shared_bwd_h'}
    ids = [f'{c.export}-{c.tag}' for c in front_half_abi_cases.CASES]
    assert len(set(ids)) == len(ids)
