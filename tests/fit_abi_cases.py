"""The cases of dcf_op_loss_table_mean (include/decafnet_hip_fit.h, ``_lib.FIT_TABLE``) for tests/test_gpu_loss_table.py, in the format
of tests/abi_cases.py: ``Case(export, tag, make, options)`` with ``make()`` -> ``(specs, call, None, verify)``; ``verify(outputs)``
compares ``per_video`` and ``out2`` bit for bit with the restatement of tests/eval_loss_ref.py and, on the tables without NaN or inf,
``out2`` with ``np.mean`` of ``np.mean``s within (N + V) * 2^-52 relative -- the bound for sums of non-negative doubles taken in two
orders.

``per_video`` and ``out2`` are placed as the int64 bits of their float64 values (the arena has no float64 fill).

Shapes: V = 1 with one query (a plain row, n_pos = 0, a NaN row, an inf row, a NaN n_pos), V = 3 with 1, 2 and 7 queries, V = 257 and
V = 600 with 1 to 5 queries each -- across a 256-lane workgroup of the first launch and across the lane stride of the final pass.
Every size once with the special rows of ``eval_loss_ref.table`` and once clean; ``nopv`` passes ``per_video = NULL``."""
import numpy as np
import torch

import eval_loss_ref as R
from abi_cases import Case, p

CASES = []
SIZES = {'v1': [1], 'v3': [1, 2, 7], 'v257': R.counts_for(257, 1), 'v600': R.counts_for(600, 2)}


def loss_mean(size, seed, special, with_pv=True):
    def make():
        counts = SIZES[size]
        rows, offsets = R.table(counts, seed, special)
        V, N = len(counts), len(rows)
        want_pv, want = R.loss_table_mean(rows, offsets)
        specs = [('rows', torch.from_numpy(rows), 'in'), ('offsets', torch.from_numpy(offsets), 'in'),
                 ('out2', torch.zeros(2, dtype=torch.int64), 'out')]
        if with_pv:
            specs.append(('per_video', torch.zeros(V, 2, dtype=torch.int64), 'out'))

        def call(c, v):
            return c.lib.dcf_op_loss_table_mean(p(v['rows']), p(v['offsets']), V, p(v.get('per_video')), p(v['out2']), c.stream())

        def verify(got):
            out = got['out2'].cpu().numpy().view(np.float64)
            print(f'LOSSTABLE {size} seed {seed} special {special}: out2 {out.tolist()} want {want.tolist()}')
            if with_pv:
                pv = got['per_video'].cpu().numpy().view(np.float64)
                assert np.array_equal(R.bits(pv), R.bits(want_pv)), f'per_video differs in {int((R.bits(pv) != R.bits(want_pv)).sum())} values'
            assert np.array_equal(R.bits(out), R.bits(want)), f'out2 {out.tolist()} want {want.tolist()}'
            if special:
                assert N == 1 or (np.isnan(want_pv).any() and np.isnan(want).all())     # the all-NaN video propagates
            else:
                ref = R.numpy_mean_of_means(rows, offsets)
                err = np.abs(out - ref) / ref
                print(f'LOSSTABLE {size}: relative distance to np.mean of np.means {err.tolist()}, bound {(N + V) * 2.0 ** -52}')
                assert np.isfinite(ref).all() and (err <= (N + V) * 2.0 ** -52).all()
        return specs, call, None, verify
    return make


for size in SIZES:
    seeds = (0, 1, 2, 3) if size == 'v1' else (4,)
    for seed in seeds:
        CASES.append(Case('dcf_op_loss_table_mean', f'{size}-special{seed}', loss_mean(size, seed, True), ()))
    CASES.append(Case('dcf_op_loss_table_mean', f'{size}-clean', loss_mean(size, 9, False), ()))
for size in ('v3', 'v600'):
    CASES.append(Case('dcf_op_loss_table_mean', f'{size}-special-nopv', loss_mean(size, 4, True, with_pv=False), ()))

EXCLUDED = {'dcf_fit_ext_version': 'no device operand: returns a constant',
            'dcf_guard_word_publish': 'reads the process-wide word of the armed guard, which no arena holds: tests/test_gpu_guard_agree.py',
            'dcf_guard_word_merge': 'writes the process-wide word of the armed guard, which no arena holds: tests/test_gpu_guard_agree.py'}
