"""Every case of tests/attn_drop_abi_cases.py between poisoned borders through tests/borders.run_case (a plain run, an arena run per
fill; outputs bit-identical, borders and inputs untouched), and that every export of ``_lib.ATTN_DROP_TABLE`` has a case or a reason.
The record waits in ``_lib.ATTN_DROP`` like ``_lib.STEPLOG``, so the table is checked here and not through ``borders.TABLE``.  GPU only;
no tolerance anywhere."""
import pytest
import torch

import attn_drop_abi_cases as C
import borders
from borders import ctx  # noqa: F401  (the module-scoped fixture)
from conftest import load_pkg

pytestmark = pytest.mark.gpu
IDS = [f'{c.export}-{c.tag}' for c in C.CASES]


def test_case_table_covers_the_attn_drop_record():
    table = load_pkg()._lib.ATTN_DROP[0].table
    assert {c.export for c in C.CASES} | set(C.EXCLUDED) == set(table) and len(set(IDS)) == len(IDS)
    assert not {c.export for c in C.CASES} & set(C.EXCLUDED) and set(C.EXCLUDED) == {'dcf_attn_drop_ext_version'}
    assert all(isinstance(r, str) and r.strip() for r in C.EXCLUDED.values())


def _after(case, specs, plain, verify):
    """the plain run computed something: no sentinel left, nothing non-finite, and the dropout both dropped and kept"""
    for name, t in plain.items():
        assert bool(torch.isfinite(t).all()), name
        if case.export == 'dcf_op_channel_dropout':
            assert bool((t == 0).any()) and bool((t != 0).any()), name


@pytest.mark.parametrize('case', C.CASES, ids=IDS)
def test_poisoned_borders(ctx, case):
    borders.run_case(ctx, case, _after)
