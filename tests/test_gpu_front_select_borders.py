"""Every case of tests/front_select_abi_cases.py between poisoned borders through tests/borders.run_case (a plain run, an arena run
per fill; outputs bit-identical, borders and inputs untouched), and that every export of ``_lib.FRONT_SELECT_TABLE`` has a case or a
reason.  The record waits in ``_lib.FRONT_SELECT`` like ``_lib.SELECT_VIDEOS``, so the table is checked here and not through
``borders.TABLE``.  GPU only; no tolerance anywhere."""
import pytest
import torch

import borders
import front_select_abi_cases as C
from borders import ctx  # noqa: F401  (the module-scoped fixture)
from conftest import load_pkg

pytestmark = pytest.mark.gpu
IDS = [f'{c.export}-{c.tag}' for c in C.CASES]


def test_case_table_covers_the_front_select_record():
    table = load_pkg()._lib.FRONT_SELECT[0].table
    assert {c.export for c in C.CASES} | set(C.EXCLUDED) == set(table) and len(set(IDS)) == len(IDS)
    assert not {c.export for c in C.CASES} & set(C.EXCLUDED) and set(C.EXCLUDED) == {'dcf_front_select_ext_version'}
    assert all(isinstance(r, str) and r.strip() for r in C.EXCLUDED.values())
    for export in set(table) - set(C.EXCLUDED):                      # every export with and without msf, with and without scat
        tags = [c.tag for c in C.CASES if c.export == export]
        assert any('-msf' in t for t in tags) and any('-nomsf' in t for t in tags)
        assert any('-scat' in t for t in tags) and any('-scat' not in t for t in tags)


def _after(case, specs, plain, verify):
    """the plain run computed something finite and not all zero"""
    for name, t in plain.items():
        assert bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0, (case.export, case.tag, name)


@pytest.mark.parametrize('case', C.CASES, ids=IDS)
def test_poisoned_borders(ctx, case):
    borders.run_case(ctx, case, _after)
