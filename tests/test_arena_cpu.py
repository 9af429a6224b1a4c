"""The poisoned-border harness (tests/arena.py) sees what it is for: plain Python "operators" on CPU views that misbehave in a known
way, each caught by exactly the check meant for it, and a well-behaved control that passes both runs.  No GPU, and no call into the
library."""
import pytest
import torch

import arena
from arena import Arena, BorderError, InputError, OutputMismatch, run_three_ways

ROWS, C = 5, 6


def specs():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(ROWS, C, generator=g)
    mask = torch.tensor([1, 1, 0, 1, 1], dtype=torch.uint8)
    return [('x', x, 'in'), ('mask', mask, 'in'), ('y', torch.empty(ROWS, C), 'out')]


def shifted(t, elements, size=None):
    """the view a faulty index computes: ``t`` moved by ``elements`` inside its storage"""
    return t.as_strided(size or t.shape, t.stride(), t.storage_offset() + elements)


def op_good(v):
    v['y'].copy_(v['x'] * v['mask'][:, None])


def op_store_one_past(v):
    op_good(v)
    shifted(v['y'].view(-1), ROWS * C, (1,)).fill_(1.0)


def op_store_row_before(v):
    op_good(v)
    shifted(v['y'], -C, (1, C)).fill_(0.0)


def op_zero_times_row_before(v):
    """a tap at row -1 behind a zero flag"""
    op_good(v)
    v['y'][0] += 0.0 * shifted(v['x'], -C, (1, C))[0]


def op_max_with_element_after(v):
    """a running maximum whose loop runs one element too far (a comparison, as v_cmp / v_max do: a NaN loses it)"""
    op_good(v)
    nb = shifted(v['x'].view(-1), ROWS * C, (1,))[0]
    last = v['y'].view(-1)[-1:]
    last.copy_(torch.where(nb > last, nb, last))


def op_gate_on_mask_byte_past_end(v):
    """row t is gated by the mask of row t + 1 as well; the last row looks one byte past the mask"""
    nxt = shifted(v['mask'], 1)
    v['y'].copy_(v['x'] * v['mask'][:, None] * (nxt != 0)[:, None])


def op_modifies_input(v):
    op_good(v)
    v['x'][1, 2] = 0.0


def test_layout():
    """operands at 512-byte offsets, borders of at least 64 KiB and 256 rows on both sides, fills and sentinels as documented"""
    wide = torch.zeros(3, 1000)                                      # 256 rows of 4000 bytes > 64 KiB
    cm = torch.zeros(4, 10)
    for fill in arena.FILLS:
        ar = Arena('cpu', fill)
        ar.place('a', torch.arange(7, dtype=torch.float32), 'in').place('w', wide, 'inout').place('m', torch.ones(5, dtype=torch.bool), 'in')
        ar.place('i', torch.arange(3, dtype=torch.int32), 'out').place('l', torch.arange(3), 'in').place('cm', cm, 'in', row_bytes=40000)
        v = ar.build()
        assert ar.buf.dtype == torch.uint8
        prev_hi = 0
        for o in ar._ops:
            need = max(64 * 1024, 256 * o['pitch'])
            assert o['off'] % 512 == 0 and o['lo'] == prev_hi
            assert o['off'] - o['lo'] >= need and o['hi'] - (o['off'] + o['nbytes']) >= need
            assert v[o['name']].data_ptr() == ar.buf.data_ptr() + o['off'] and v[o['name']].is_contiguous()
            prev_hi = o['hi']
        assert prev_hi == ar.buf.numel()
        assert [o['pitch'] for o in ar._ops] == [4, 4000, 1, 4, 8, 40000]
        f32 = ar.buf[:ar._ops[0]['off']].view(torch.int32)
        assert bool((f32 == (0x7fc00000, 0x7f7fffff)[fill - 1]).all())
        after_a = ar.buf[ar._ops[0]['off'] + 28:ar._ops[0]['hi']].view(torch.int32)          # the border starts at the operand's last byte
        assert bool((after_a == (0x7fc00000, 0x7f7fffff)[fill - 1]).all())
        m = ar._ops[2]
        assert bool((ar.buf[m['lo']:m['off']] == (0xFF, 0)[fill - 1]).all()) and bool((ar.buf[m['off'] + 5:m['hi']] == (0xFF, 0)[fill - 1]).all())
        i = ar._ops[3]
        assert bool((ar.buf[i['lo']:i['off']].view(torch.int32) == (0x7fffffff, 0)[fill - 1]).all())
        ln = ar._ops[4]
        assert bool((ar.buf[ln['lo']:ln['off']].view(torch.int64) == (0x7fffffffffffffff, 0)[fill - 1]).all())
        assert torch.equal(v['a'], torch.arange(7, dtype=torch.float32)) and torch.equal(v['l'], torch.arange(3))
        assert bool((v['i'] == 0x5A5A5A5A).all())                      # an output starts as its sentinel
        ar.verify()
        v['w'].add_(1.0)                                               # an inout operand may change, an output too
        v['i'].zero_()
        ar.verify()


def test_control_passes_both_runs():
    out = run_three_ways(specs(), op_good, 'cpu')
    x, mask = specs()[0][1], specs()[1][1]
    assert torch.equal(out['y'], x * mask[:, None])


@pytest.mark.parametrize('op', [op_store_one_past, op_store_row_before])
def test_store_outside_the_output_is_caught_by_the_border_check(op):
    with pytest.raises(BorderError, match="'y'"):
        run_three_ways(specs(), op, 'cpu')
    # ... in both fills, and by nothing else: the outputs themselves are those of the plain run
    for fill in arena.FILLS:
        ar = Arena('cpu', fill)
        for s in specs():
            ar.place(*s)
        v = ar.build()
        op(v)
        assert torch.equal(v['y'], specs()[0][1] * specs()[1][1][:, None])
        with pytest.raises(BorderError, match='before' if op is op_store_row_before else 'after'):
            ar.verify()


def _arena_run(op, fill):
    ar = Arena('cpu', fill)
    for s in specs():
        ar.place(*s)
    v = ar.build()
    op(v)
    ar.verify()
    return v['y'].clone()


def _plain_run(op):
    v, _ = arena.plain_operands(specs(), 'cpu')
    op(v)
    return v['y'].clone()


def test_zero_times_neighbour_is_caught_by_the_nan_run_only():
    with pytest.raises(OutputMismatch) as e:
        run_three_ways(specs(), op_zero_times_row_before, 'cpu')
    assert e.value.fill == 1
    plain = _plain_run(op_zero_times_row_before)
    assert torch.isnan(_arena_run(op_zero_times_row_before, 1)[0]).all()
    assert torch.equal(_arena_run(op_zero_times_row_before, 2), plain), '0 * the largest finite float is 0: the finite run cannot see it'


def test_max_with_neighbour_is_caught_by_the_finite_run_only():
    with pytest.raises(OutputMismatch) as e:
        run_three_ways(specs(), op_max_with_element_after, 'cpu')
    assert e.value.fill == 2
    plain = _plain_run(op_max_with_element_after)
    assert torch.equal(_arena_run(op_max_with_element_after, 1), plain), 'a NaN loses the comparison: the NaN run cannot see it'
    assert float(_arena_run(op_max_with_element_after, 2).view(-1)[-1]) == torch.finfo(torch.float32).max


def test_mask_byte_past_the_end_is_caught_by_the_mask_fill():
    """next to zeroed memory (the plain run) and next to fill 2 (0x00) the stray byte closes the gate of the last row; fill 1 (0xFF, a
    valid mask byte) opens it"""
    with pytest.raises(OutputMismatch) as e:
        run_three_ways(specs(), op_gate_on_mask_byte_past_end, 'cpu')
    assert e.value.fill == 1
    plain = _plain_run(op_gate_on_mask_byte_past_end)
    assert torch.equal(_arena_run(op_gate_on_mask_byte_past_end, 2), plain)
    got = _arena_run(op_gate_on_mask_byte_past_end, 1)
    assert torch.equal(got[:-1], plain[:-1]) and bool((plain[-1] == 0).all()) and torch.equal(got[-1], specs()[0][1][-1])


def test_modified_input_is_caught_by_the_input_check():
    with pytest.raises(InputError, match="'x'"):
        run_three_ways(specs(), op_modifies_input, 'cpu')


def test_update_rewrites_an_input_and_its_snapshot():
    ar = Arena('cpu', 1)
    ar.place('table', torch.zeros(2, 8, dtype=torch.int64), 'in').place('p', torch.zeros(4), 'inout')
    v = ar.build()
    tab = torch.zeros(2, 8, dtype=torch.int64)
    tab[0, 0] = v['p'].data_ptr()
    ar.update('table', tab)
    assert int(v['table'][0, 0]) == v['p'].data_ptr()
    ar.verify()
    v['table'][1, 1] = 5
    with pytest.raises(InputError, match="'table'"):
        ar.verify()


def test_case_table_is_well_formed():
    """tests/abi_cases.py without a GPU: every builder yields operands the arena can place, ids are unique, and every name of the
    signature table is either a case or excluded with a reason (tests/test_gpu_borders.py asserts the same before it runs them)"""
    import abi_cases
    from conftest import load_pkg
    seen = set()
    for c in abi_cases.CASES:
        assert (c.export, c.tag) not in seen, (c.export, c.tag)
        seen.add((c.export, c.tag))
        made = c.make()
        assert len(made) in (2, 3) and callable(made[1])
        ar = Arena('cpu', 1)
        for s in made[0]:
            assert s[2] in arena.ROLES and s[1].device.type == 'cpu', (c.export, c.tag, s[0])
            ar.place(*s)
        assert any(s[2] != 'in' for s in made[0]), (c.export, c.tag, 'no output operand')
        ar.build()
        ar.verify()
    signatures = load_pkg()._lib.SIGNATURES
    covered = {c.export for c in abi_cases.CASES}
    assert not [n for n in signatures if n not in covered and n not in abi_cases.EXCLUDED]
    assert not [n for n in list(covered) + list(abi_cases.EXCLUDED) if n not in signatures]
