"""tests/test_gpu_borders.py for the embedding-stage extension: both operators of ``_lib.EMBD_SIGNATURES`` on operands between
poisoned borders (tests/arena.py) -- a plain run, an arena run per fill; outputs bit-identical, every border byte and every input
untouched.  The one-kernel form reads two halo rows on each side of a 124-row window and stores only rows of [0, B * T); the shapes
put the first and the last window against the borders.  GPU only; no tolerance anywhere."""
import pytest
import torch

import arena
import embd_chain_cases as C
import embd_chain_ref as ER
from conftest import load_pkg

pytestmark = pytest.mark.gpu

EXPORTS = ['dcf_op_embd_chain', 'dcf_op_embd_launches']
EXCLUDED = {'dcf_embd_ext_version': 'no device operand: returns a constant'}


@pytest.fixture(scope='module')
def ctx():
    pkg, model, sd, handle = C.make_model()
    return dict(pkg=pkg, model=model, handle=handle, params=ER.params_of(sd, C.E))


@pytest.mark.parametrize('ln_in', [1, 0])
@pytest.mark.parametrize('with_pe', [1, 0])
@pytest.mark.parametrize('B,T', [(2, 125), (3, 100), (4, 1)])
@pytest.mark.parametrize('export', EXPORTS)
def test_embd_export_between_poisoned_borders(ctx, export, B, T, with_pe, ln_in):
    pkg, handle, p = ctx['pkg'], ctx['handle'], ctx['params']
    mask = C.masks_of(B, T, 100 + B * T)
    specs = [('X', C.rows_of(B, T, ln_in, 9, p), 'in', C.E * 4), ('mask', mask, 'in'),
             ('Y', torch.zeros(B, T, C.E), 'out', C.E * 4)]
    if with_pe:
        specs.append(('pe', torch.randn(T, C.E, generator=torch.Generator().manual_seed(2)), 'in', C.E * 4))

    def run(v):
        return C.call(pkg, handle, export, v['X'], v['mask'], ln_in, v.get('pe'), v['Y'])

    plain = arena.run_three_ways(specs, run, 'cuda')
    assert bool(torch.isfinite(plain['Y']).all())            # every row of [0, B * T) was stored: no sentinel left
    assert ctx['model'].numerics_status(reset=True) & 1 == 0


def test_every_embd_export_has_a_case():
    names = list(load_pkg()._lib.EMBD_SIGNATURES)
    assert set(EXCLUDED) == {'dcf_embd_ext_version'}
    assert sorted(n for n in names if n not in EXCLUDED) == sorted(EXPORTS)
