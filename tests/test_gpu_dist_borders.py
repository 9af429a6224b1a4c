"""tests/test_gpu_borders.py for the data-parallel extension: every operator of ``_lib.DIST_SIGNATURES`` on operands between poisoned
borders (tests/arena.py) at the shapes of tests/dist_abi_cases.py -- a plain run, an arena run per fill; outputs bit-identical, borders
and inputs untouched; then the plain run's values against ``torch.mul`` and the poison between the destination slices.  GPU only; no
tolerance anywhere."""
import pytest

import arena
import dist_abi_cases
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


@pytest.mark.parametrize('case', dist_abi_cases.CASES, ids=[f'{c.export}-{c.tag}' for c in dist_abi_cases.CASES])
def test_dist_export_between_poisoned_borders(ctx, case):
    specs, call, fixup, verify = case.make()

    def run(v):
        rc = call(ctx, v)
        ctx.pkg._lib.check(rc, case.export)    # a non-zero return code raises with dcf_last_error()
        return rc

    plain = arena.run_three_ways(specs, run, 'cuda', fixup)
    C = dist_abi_cases
    assert verify(plain) == sum(C.SIZES) - C.SIZES[C.NO_GRAD] - C.SIZES[C.NULL_G]


def test_argument_checks_and_the_empty_table(ctx):
    """check_table's pattern: -1 with a message for negative counts, a null table and chunks without tensors; no chunks is a no-op"""
    lib, st = ctx.lib, ctx.stream()
    assert lib.dcf_dist_pack_grads(None, None, 0, 0, 0.5, st) == 0
    assert lib.dcf_dist_pack_grads(None, None, 3, 0, 0.5, st) == 0
    for args, word in (((None, None, 1, 1), 'null table'), ((None, None, -1, 0), 'negative'), ((None, None, 1, -1), 'negative'),
                       ((None, None, 1, 1 << 31), 'exceed')):
        assert lib.dcf_dist_pack_grads(*args, 0.5, st) == -1
        msg = lib.dcf_last_error().decode()
        assert 'dcf_dist_pack_grads' in msg and word in msg, msg


def test_every_dist_export_has_a_case():
    """every name of the extension's table has a poisoned-border case or is the version function"""
    pkg = load_pkg()
    names = list(pkg._lib.DIST_SIGNATURES)
    covered = {c.export for c in dist_abi_cases.CASES}
    assert set(dist_abi_cases.EXCLUDED) == {'dcf_dist_ext_version'}
    missing = [n for n in names if n not in covered and n not in dist_abi_cases.EXCLUDED]
    assert not missing, f'data-parallel exports without a case: {missing}'
    stale = [n for n in covered if n not in pkg._lib.DIST_SIGNATURES]
    assert not stale, f'not in DIST_SIGNATURES: {stale}'
