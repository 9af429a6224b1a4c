"""CPU checks that go with the data-parallel extension (include/decafnet_hip_dist.h; its header and table:
tests/test_abi_headers.py): the names of ``_lib.DIST_SIGNATURES``, and the pure-Python parts of the bucketed gradient all-reduce,
``dist.grad_bucket_plan`` and ``dist._BucketSchedule``.  No GPU, no compute calls."""
import random

import pytest

from conftest import load_pkg

KIB = 1024


def test_dist_table_names():
    assert sorted(load_pkg()._lib.DIST_SIGNATURES) == ['dcf_dist_ext_version', 'dcf_dist_pack_grads']


# ---------------------------------------------------------------------------------------------- the plan
def check_plan(sizes, plan, bucket_bytes, align=64):
    """the rules of grad_bucket_plan, whatever the sizes"""
    order = [i for b in plan['buckets'] for i in b['params']]
    assert order == list(reversed(range(len(sizes)))), 'every index once, in reverse order'
    slices, end = [], 0
    for b in plan['buckets']:
        assert b['start'] == end and b['start'] % align == 0 and b['end'] % align == 0 and len(b['params']) == len(b['offsets']) >= 1
        for i, off in zip(b['params'], b['offsets']):
            assert off % align == 0 and b['start'] <= off and off + sizes[i] <= b['end'], (i, off)
            slices.append((off, off + sizes[i]))
        nbytes = 4 * (b['end'] - b['start'])
        assert nbytes <= bucket_bytes or len(b['params']) == 1, f'{nbytes} bytes in a bucket of {len(b["params"])} tensors'
        end = b['end']
    assert plan['length'] == end and plan['align'] == align
    slices.sort()
    assert all(a[1] <= b[0] for a, b in zip(slices, slices[1:])), 'slices are disjoint'


def test_plan_of_the_stated_sizes():
    D = load_pkg().dist
    sizes = [1, 63, 64, 65, 5000, 1]
    plan = D.grad_bucket_plan(sizes, 4 * KIB)
    check_plan(sizes, plan, 4 * KIB)
    # in reverse order: the last tensor (1 -> one slot of 64) is closed by the oversize 5000, which stays alone; 65 takes two slots,
    # 64, 63 and 1 one each: 320 floats of the 1024 a bucket holds
    assert [b['params'] for b in plan['buckets']] == [[5], [4], [3, 2, 1, 0]]
    assert [b['offsets'] for b in plan['buckets']] == [[0], [64], [5120, 5248, 5312, 5376]]
    assert [(b['start'], b['end']) for b in plan['buckets']] == [(0, 64), (64, 5120), (5120, 5440)] and plan['length'] == 5440
    assert D.grad_bucket_plan(sizes, 4 * KIB) == plan and D.grad_bucket_plan(tuple(sizes), 4 * KIB) == plan      # equal inputs, equal plans


def test_plan_rules_for_seeded_sizes():
    D = load_pkg().dist
    rs = random.Random(7)
    for trial in range(20):
        sizes = [rs.choice([0, 1, 63, 64, 65, 1000, 1024, 1025, rs.randint(1, 5000)]) for _ in range(rs.randint(1, 40))]
        for bucket_bytes, align in ((4 * KIB, 64), (64 * KIB, 64), (D.DEFAULT_BUCKET_BYTES, 64), (4 * KIB, 16), (256, 64)):
            plan = D.grad_bucket_plan(sizes, bucket_bytes, align)
            check_plan(sizes, plan, bucket_bytes, align)
    one = D.grad_bucket_plan([10, 20, 30], D.DEFAULT_BUCKET_BYTES)
    assert len(one['buckets']) == 1 and one['length'] == 192
    assert D.grad_bucket_plan([], 4 * KIB) == {'buckets': [], 'length': 0, 'align': 64}
    over = D.grad_bucket_plan([512, 512, 64], 4 * KIB)                    # 64 + 512 fit, the second 512 would pass the 1024 floats
    assert [b['params'] for b in over['buckets']] == [[2, 1], [0]]
    exact = D.grad_bucket_plan([512, 512], 4 * KIB)                       # exactly 4 KiB is not more than 4 KiB
    assert [b['params'] for b in exact['buckets']] == [[1, 0]]
    with pytest.raises(ValueError):
        D.grad_bucket_plan([4], 0)
    assert D.DEFAULT_BUCKET_BYTES == 25 * KIB * KIB


# ---------------------------------------------------------------------------------------------- the schedule
def test_schedule_launches_in_index_order_whatever_the_ready_order():
    D = load_pkg().dist
    sizes = [1, 63, 64, 65, 5000, 1, 700, 700, 700, 3, 3, 2000]
    plan = D.grad_bucket_plan(sizes, 4 * KIB)
    K = len(plan['buckets'])
    assert K >= 5
    bucket_of = {i: k for k, b in enumerate(plan['buckets']) for i in b['params']}
    sched = D._BucketSchedule(plan)
    for seed in range(12):
        order = list(range(len(sizes)))
        random.Random(seed).shuffle(order)
        if seed % 3 == 2:
            order = order[:len(order) // 2]                  # some parameters never get a gradient: finish() hands their buckets out
        sched.reset()                                         # ... and re-arms after the previous round
        reported, by_ready = set(), []
        for i in order:
            reported.add(i)
            got = sched.ready(i)
            for k in got:
                assert set(plan['buckets'][k]['params']) <= reported, f'bucket {k} before all its parameters (seed {seed})'
            by_ready += got
            assert sched.ready(i) == [], 'a parameter reported twice counts once'
        rest = sched.finish()
        assert by_ready + rest == list(range(K)), (seed, by_ready, rest)
        assert sched.finish() == [] and all(sched.ready(i) == [] for i in range(len(sizes)))
        if seed % 3 != 2:
            assert rest == []
        else:
            assert rest and not set(plan['buckets'][rest[0]]['params']) <= reported
    # in reverse parameter order (the order the plan assumes) every bucket goes out with its last parameter
    sched.reset()
    for i in reversed(range(len(sizes))):
        last = plan['buckets'][bucket_of[i]]['params'][-1] == i
        assert sched.ready(i) == ([bucket_of[i]] if last else [])
    assert sched.finish() == []
