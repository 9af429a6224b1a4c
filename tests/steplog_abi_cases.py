"""The cases of dcf_op_steplog_add and dcf_op_steplog_flush (include/decafnet_hip_steplog.h, ``_lib.STEPLOG_TABLE``) for
tests/test_gpu_steplog.py, in the format of tests/abi_cases.py: ``Case(export, tag, make, options)`` with ``make()`` -> ``(specs, call,
None, verify)``; ``verify(outputs)`` compares ``stats``, ``counts`` and ``out`` bit for bit with the restatement of tests/steplog_ref.py.

``stats`` and ``out`` are placed as the int64 bits of their float64 values (the arena has no float64 fill), and every value of an add
is an operand of its own -- one fp32 between its own borders -- as the losses of a step are allocations of their own.

Shapes: K = 1, 3 and 16 (the one-key table, the Trainer's three losses, the most the extension takes).  The tables are those the
restatement leaves after 0, 1 and 5 earlier steps (plain and special vectors in turn), with a recognisable value in the reserved
column.  An add puts one plain vector or one of the special values of ``steplog_ref.SPECIAL`` (NaN, both infinities, both zeros,
denormals, 3.4e38) on top; a flush reads each of the tables out, the empty one included."""
import ctypes

import numpy as np
import torch

import steplog_ref as R
from abi_cases import Case, p

CASES = []
KS = (1, 3, 16)
EARLIER = (0, 1, 5)
RESERVED = 7.0


def _tables(K, n):
    stats, counts = R.tables_after(K, n, 100 * K + n)
    stats[:, R.RESERVED] = RESERVED
    return stats, counts


def _as_words(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy())


def _same(got, want, what):
    got = got.cpu().numpy().view(np.uint64).reshape(-1)
    want = np.ascontiguousarray(want).view(np.uint64).reshape(-1)
    bad = np.nonzero(got != want)[0]
    assert not len(bad), f'{what}: {len(bad)} of {len(want)} words differ, the first at {int(bad[0])}: {int(got[bad[0]]):#x} want {int(want[bad[0]]):#x}'


def add(K, n, special):
    def make():
        stats, counts = _tables(K, n)
        vals = R.special_vals(K, n + K) if special else R.random_vals(K, 7 * K + n)
        specs = [(f'v{k}', torch.from_numpy(vals[k:k + 1].copy()), 'in') for k in range(K)]
        specs += [('stats', _as_words(stats), 'inout'), ('counts', torch.from_numpy(counts.copy()), 'inout')]
        R.add(stats, counts, vals)                                             # what the call has to leave

        def call(c, v):
            ptrs = (ctypes.c_void_p * K)(*[v[f'v{k}'].data_ptr() for k in range(K)])
            return c.lib.dcf_op_steplog_add(ptrs, K, p(v['stats']), p(v['counts']), c.stream())

        def verify(got):
            _same(got['stats'], stats, 'stats')
            _same(got['counts'], counts, 'counts')
            assert counts[K] == n + 1 and (stats[:, R.RESERVED] == RESERVED).all()
        return specs, call, None, verify
    return make


def flush(K, n):
    def make():
        stats, counts = _tables(K, n)
        specs = [('stats', _as_words(stats), 'inout'), ('counts', torch.from_numpy(counts.copy()), 'inout'),
                 ('out', torch.zeros(K + 1, R.COLS, dtype=torch.int64), 'out')]
        want = R.flush(stats, counts)

        def call(c, v):
            return c.lib.dcf_op_steplog_flush(p(v['stats']), p(v['counts']), K, p(v['out']), c.stream())

        def verify(got):
            _same(got['out'], want, 'out')
            _same(got['stats'], stats, 'stats')
            _same(got['counts'], counts, 'counts')
            assert want[K, 0] == n and not counts.any() and not stats[:, :R.RESERVED].any() and (stats[:, R.RESERVED] == RESERVED).all()
        return specs, call, None, verify
    return make


for K in KS:
    for n in EARLIER:
        CASES.append(Case('dcf_op_steplog_add', f'k{K}-after{n}-plain', add(K, n, False), ()))
        CASES.append(Case('dcf_op_steplog_add', f'k{K}-after{n}-special', add(K, n, True), ()))
        CASES.append(Case('dcf_op_steplog_flush', f'k{K}-after{n}', flush(K, n), ()))

EXCLUDED = {'dcf_steplog_ext_version': 'no device operand: returns a constant'}
