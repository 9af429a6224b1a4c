"""Every case of tests/select_abi_cases.py between poisoned borders through tests/borders.run_case (a plain run, an arena run per
fill; outputs bit-identical, borders and inputs untouched), and that every export of ``_lib.SELECT_TABLE`` has a case or a reason.
The record waits in ``_lib.SELECT`` like ``_lib.ATTN_DROP``, so the table is checked here and not through ``borders.TABLE``.  GPU only;
no tolerance anywhere."""
import pytest
import torch

import borders
import select_abi_cases as C
import select_ref
from borders import ctx  # noqa: F401  (the module-scoped fixture)
from conftest import load_pkg

pytestmark = pytest.mark.gpu
IDS = [f'{c.export}-{c.tag}' for c in C.CASES]


def test_case_table_covers_the_select_record():
    table = load_pkg()._lib.SELECT[0].table
    assert {c.export for c in C.CASES} | set(C.EXCLUDED) == set(table) and len(set(IDS)) == len(IDS)
    assert not {c.export for c in C.CASES} & set(C.EXCLUDED) and set(C.EXCLUDED) == {'dcf_select_ext_version'}
    assert all(isinstance(r, str) and r.strip() for r in C.EXCLUDED.values())


def _after(case, specs, plain, verify):
    """the plain run computed something: the list is the restatement's and its tail kept the sentinel; the gathered rows are the
    indexed columns; a forward left no sentinel and nothing non-finite"""
    ops = {name: t for name, t, *_ in specs}
    if case.export == 'dcf_op_select_clips':
        clips, pos, n = select_ref.select_clips(ops['gate'], ops['mask'])
        got = plain['clips'].cpu()
        assert int(plain['count'].cpu()) == n and torch.equal(got[:n], clips) and torch.equal(plain['pos'].cpu(), pos)
        assert bool((got[n:] == 0x5A5A5A5A).all()), 'an entry at or beyond count was written'
    elif case.export.startswith('dcf_op_gather_clip_rows'):
        x, rows = ops['X'], plain['rows'].cpu()
        if case.export.endswith('_h'):
            x, rows = x.view(torch.int16), rows.view(torch.int16)
        assert torch.equal(rows, select_ref.gather_clip_rows(x, ops['clips']))
    else:
        assert bool(torch.isfinite(plain['logits']).all()) and bool(torch.isfinite(plain['offsets']).all())


@pytest.mark.parametrize('case', C.CASES, ids=IDS)
def test_poisoned_borders(ctx, case):
    borders.run_case(ctx, case, _after)
