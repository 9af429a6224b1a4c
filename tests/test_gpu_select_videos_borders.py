"""Every case of tests/select_videos_abi_cases.py between poisoned borders through tests/borders.run_case (a plain run, an arena run
per fill; outputs bit-identical, borders and inputs untouched), and that every export of ``_lib.SELECT_VIDEOS_TABLE`` has a case or a
reason.  The record waits in ``_lib.SELECT_VIDEOS`` like ``_lib.SELECT``, so the table is checked here and not through
``borders.TABLE``.  GPU only; no tolerance anywhere."""
import pytest
import torch

import borders
import select_videos_abi_cases as C
import select_videos_ref as V
from borders import ctx  # noqa: F401  (the module-scoped fixture)
from conftest import load_pkg

pytestmark = pytest.mark.gpu
IDS = [f'{c.export}-{c.tag}' for c in C.CASES]
SENTINEL = 0x5A5A5A5A


def test_case_table_covers_the_select_videos_record():
    table = load_pkg()._lib.SELECT_VIDEOS[0].table
    assert {c.export for c in C.CASES} | set(C.EXCLUDED) == set(table) and len(set(IDS)) == len(IDS)
    assert not {c.export for c in C.CASES} & set(C.EXCLUDED) and set(C.EXCLUDED) == {'dcf_select_videos_ext_version'}
    assert all(isinstance(r, str) and r.strip() for r in C.EXCLUDED.values())


def _lists_are_consistent(clips, pos, counts, masks):
    """every list ascending, inside its video's valid clips, the inverse of pos, and its tail kept the sentinel"""
    for v, n in enumerate(counts.tolist()):
        c = clips[v, :n].long()
        assert 0 < n <= int(masks[v].sum()) and bool((c[1:] > c[:-1]).all()) and bool(masks[v][c].all())
        assert bool((clips[v, n:] == SENTINEL).all()), 'an entry at or beyond a count was written'
        want = torch.full_like(pos[v], -1)
        want[c] = torch.arange(n, dtype=pos.dtype)
        assert torch.equal(pos[v], want)


def _after(case, specs, plain, verify):
    """the plain run computed something: the lists are the restatement's and their tails kept the sentinel; the gathered rows are the
    indexed columns; dcf_select_videos left consistent lists of its own gates; a forward left no sentinel and nothing non-finite"""
    ops = {name: t for name, t, *_ in specs}
    if case.export == 'dcf_op_select_clips_videos':
        T, lens, nqs, _, _ = next(s for s in C.SELECT_SHAPES if f'T{s[0]}-' in case.tag)
        clips, pos, counts, _ = V.select_clips_videos(ops['gate'], ops['masks'], nqs, fill=SENTINEL)
        assert plain['counts'].cpu().tolist() == counts and torch.equal(plain['clips'].cpu(), clips) and torch.equal(plain['pos'].cpu(), pos)
    elif case.export.startswith('dcf_op_gather_clip_rows_videos'):
        counts = [int(n) for n in case.tag.split('-n')[1].split('_')]
        xs, rows = [ops[f'X{v}'] for v in range(len(counts))], plain['rows'].cpu()
        if case.export.endswith('_h'):
            xs, rows = [x.view(torch.int16) for x in xs], rows.view(torch.int16)
        assert torch.equal(rows, V.gather_clip_rows_videos(xs, ops['clips'], counts))
    elif case.export.startswith('dcf_select_videos'):
        nv = plain['counts'].numel()
        gate = plain['gate'].cpu()
        assert bool(((gate == 0) | (gate == 1)).all())
        masks = torch.stack([ops[f'mask{v}'] for v in range(nv)]).bool()
        clips, pos, counts = plain['clips'].cpu(), plain['pos'].cpu(), plain['counts'].cpu()
        _lists_are_consistent(clips, pos, counts, masks)
        nqs = [ops[f'cls{v}'].shape[0] for v in range(nv)]
        want = V.select_clips_videos(gate, masks, nqs, fill=SENTINEL)
        assert torch.equal(clips, want[0]) and torch.equal(pos, want[1]) and counts.tolist() == want[2]
        if 'correl' in plain:
            assert bool(torch.isfinite(plain['correl']).all())
    else:
        assert bool(torch.isfinite(plain['logits']).all()) and bool(torch.isfinite(plain['offsets']).all())


@pytest.mark.parametrize('case', C.CASES, ids=IDS)
def test_poisoned_borders(ctx, case):
    borders.run_case(ctx, case, _after)
