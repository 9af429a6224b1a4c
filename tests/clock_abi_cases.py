"""One entry per table export of the step-count extension (include/decafnet_hip_clock.h, ``_lib.CLOCK_SIGNATURES``) for
tests/test_gpu_clock_borders.py, in the format of tests/guard_abi_cases.py: ``Case(export, tag, make, options)`` with ``make()`` ->
``(specs, call, fixup, verify)``; ``verify(outputs)`` checks the values of the plain run, which the arena runs must equal bit for bit.

The table is the nine rows of tests/guard_abi_cases.py (n = 1, 3, 5, 257, 0, CHUNK-1, CHUNK+1, 2 CHUNK+7 and 77; two rows at an address
of 4 mod 16, one with DCF_OPTIM_NO_GRAD and a NaN in its gradient, one without an EMA copy).  Further operands: ``steps`` (nine int64,
``inout``; the start counts 0, 1, 2, 3, 4, 5, 6, 2000, 40 put the row of 2 CHUNK+7 elements past the end of its group's table and give
every row a count of its own), the two bias-correction tables (``in``; group 0 betas (0.9, 0.999), group 1 betas (0.8, 0.99), built
by ``optim.bias_correction_table``), the coefficient and the dcf_guard_state record (``in``).

dcf_clock_adam_step: under verdict apply -- every tensor that has to move moved, the counts are + 1 except on the NO_GRAD row -- and
under verdict skip, where every parameter, moment, EMA tensor and count -- all ``inout`` -- must come back with the bits that went in."""
import ctypes

import numpy as np
import torch

from abi_cases import _ROW, Case, gen, p, rn
from guard_abi_cases import CHUNK, COLS, MISALIGNED, NO_EMA, NO_GRAD, SIZES, START, state_words

CASES = []
BETAS = ((0.9, 0.999), (0.8, 0.99))
COUNTS = [0, 1, 2, 3, 4, 5, 6, 2000, 40]


def case(export, tag, make):
    CASES.append(Case(export, tag, make, ()))


def _clock(verdict):
    def make():
        from conftest import load_pkg
        g = gen(67, len(SIZES), sum(SIZES))
        n_t, tensors = len(SIZES), {}
        roles = dict(p='inout', g='in', m='inout', v='inout', e='inout')
        specs = []
        for i, n in enumerate(SIZES):
            pad = 1 if i in MISALIGNED else 0
            for col, _, scale in COLS:
                t = torch.rand(n + pad, generator=g) * 1e-3 if scale is None else rn(g, n + pad, scale=scale)
                if col == 'g' and i == NO_GRAD:
                    t[pad + 1] = float('nan')
                tensors[f'{col}{i}'] = t[pad:]
                specs.append((f'{col}{i}', t, roles[col]))
        counts = [-(-n // CHUNK) for n in SIZES]
        cmap = np.repeat(np.arange(n_t, dtype=np.int32), counts)
        tables = [load_pkg().optim.bias_correction_table(*b) for b in BETAS]
        assert len(tables[1]) < COUNTS[7] and n_t == len(COUNTS)
        specs += [('table', torch.zeros(n_t, 8, dtype=torch.int64), 'in'), ('cmap', torch.from_numpy(cmap.copy()), 'in'),
                  ('state', state_words(dict(START, verdict=verdict)), 'in'), ('coef', torch.tensor([0.37]), 'in'),
                  ('steps', torch.tensor(COUNTS, dtype=torch.int64), 'inout'),
                  ('bc0', torch.from_numpy(tables[0].reshape(-1).copy()), 'in'), ('bc1', torch.from_numpy(tables[1].reshape(-1).copy()), 'in')]

        def fixup(v, update):
            rec = np.zeros(n_t, dtype=_ROW)
            for i, n in enumerate(SIZES):
                off = 4 if i in MISALIGNED else 0
                for col, f, _ in COLS:
                    rec[f][i] = v[f'{col}{i}'].data_ptr() + off
                    assert rec[f][i] % 16 == off
                if i == NO_EMA:
                    rec['ema'][i] = 0
                rec['n'][i], rec['group'][i], rec['flags'][i] = n, i % 2, int(i == NO_GRAD)
            rec['chunk0'] = np.cumsum(counts) - np.array(counts)
            update('table', torch.from_numpy(rec.view(np.int64).reshape(n_t, 8).copy()))

        def call(c, v):
            groups = (c.pkg._lib.DcfOptimGroup * 2)()
            for k, (wd, mode) in enumerate(((0.05, 0), (0.01, 1))):
                h = groups[k]
                h.lr, h.weight_decay, h.b1, h.b2, h.eps = 1e-3, wd, BETAS[k][0], BETAS[k][1], 1e-8
                h.one_minus_b1, h.one_minus_b2 = 1.0 - BETAS[k][0], 1.0 - BETAS[k][1]
                h.bc1 = h.sqrt_bc2 = float('nan')                   # ignored by this export
                h.mode = mode
            bc = (ctypes.c_void_p * 2)(v['bc0'].data_ptr(), v['bc1'].data_ptr())
            lens = (ctypes.c_int32 * 2)(len(tables[0]), len(tables[1]))
            return c.lib.dcf_clock_adam_step(p(v['table']), p(v['cmap']), n_t, len(cmap), ctypes.cast(groups, ctypes.c_void_p), 2,
                                             ctypes.cast(bc, ctypes.c_void_p), ctypes.cast(lens, ctypes.c_void_p), p(v['steps']), p(v['coef']),
                                             p(v['state']), 1, 0.999, c.stream())

        def verify(outputs):
            moved = 0
            for i, n in enumerate(SIZES):
                for col in 'pmve':
                    same = torch.equal(outputs[f'{col}{i}'][-n:].cpu().view(torch.int32), tensors[f'{col}{i}'].view(torch.int32)) if n else True
                    written = i != NO_GRAD if col != 'e' else i != NO_EMA
                    if verdict or not written or not n:
                        assert same, f'{col}{i} changed under verdict {verdict}'
                    else:
                        assert not same and bool(torch.isfinite(outputs[f'{col}{i}'][-n:]).all()), f'{col}{i} did not move under verdict apply'
                        moved += 1
            steps = outputs['steps'].cpu().tolist()
            assert steps == [c + int(not verdict and i != NO_GRAD) for i, c in enumerate(COUNTS)], steps
            print(f'CLOCKADAM verdict {verdict}: {moved} tensors moved, counts {steps}')
            return moved
        return specs, call, fixup, verify
    return make


case('dcf_clock_adam_step', 'nine-tensors-verdict-apply', _clock(0))
case('dcf_clock_adam_step', 'nine-tensors-verdict-skip', _clock(1))

EXCLUDED = {'dcf_clock_ext_version': 'no device operand: returns a constant'}
