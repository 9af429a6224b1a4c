"""One entry per table export of the step-guard extension (include/decafnet_hip_guard.h, ``_lib.GUARD_SIGNATURES``) for
tests/test_gpu_guard_borders.py, in the format of tests/abi_cases.py: ``Case(export, tag, make, options)`` with ``make()`` ->
``(specs, call, fixup, verify)``; ``verify(outputs)`` checks the values of the plain run, which the arena runs must equal bit for bit.

ONE table of nine rows, n = 1, 3, 5, 257, 0, CHUNK-1, CHUNK+1, 2 CHUNK+7 and 77: parameter, gradient, both moments and the EMA copy of
every row are operands of their own, two rows start one element into them (address = 4 mod 16: the element-at-a-time path), one row
carries DCF_OPTIM_NO_GRAD and a NaN in its gradient that must not count, one has no EMA copy.  The dcf_guard_state record is an operand
too (six int64): ``inout`` for the norm, which must leave the restatement's record (tests/guard_ref.py) in it, ``in`` for the update.

dcf_guard_grad_norm: finite gradients (verdict apply) and one with an inf in the last element of the longest row (verdict skip, the
coefficient +0).  dcf_guard_adam_step: under verdict apply, and under verdict skip, where every parameter, moment and EMA tensor -- all
``inout`` -- must come back with the bits that went in."""
import ctypes
import math

import numpy as np
import torch

from abi_cases import _ROW, Case, gen, out, p, rn
import guard_ref as G

CASES = []
CHUNK = 4096
SIZES = [1, 3, 5, 257, 0, CHUNK - 1, CHUNK + 1, 2 * CHUNK + 7, 77]
MISALIGNED, NO_GRAD, NO_EMA = (3, 7), 2, 5
COLS = (('p', 'p', 1.0), ('g', 'g', 0.1), ('m', 'exp_avg', 0.01), ('v', 'exp_avg_sq', None), ('e', 'ema', 1.0))
_STATE = np.dtype([('verdict', '<i4'), ('first_bad_row', '<i4'), ('n_bad_rows', '<i4'), ('reserved0', '<i4'), ('applied', '<i8'),
                   ('skipped', '<i8'), ('last_skipped_attempt', '<i8'), ('conv_flag', '<i4'), ('reserved1', '<i4')])
START = dict(G.fresh_state(applied=5, skipped=2))


def case(export, tag, make):
    CASES.append(Case(export, tag, make, ()))


def state_words(state):
    rec = np.zeros(1, dtype=_STATE)
    for k in G.FIELDS:
        rec[k] = state[k]
    return torch.from_numpy(rec.view(np.int64).reshape(-1).copy())


def state_of(words):
    rec = words.cpu().numpy().view(_STATE)[0]
    return {k: int(rec[k]) for k in G.FIELDS}


def _guard(kind, poison=False, verdict=0):
    def make():
        g = gen(61, len(SIZES), sum(SIZES))
        n_t, tensors = len(SIZES), {}
        roles = dict(p='in', g='in', m='in', v='in', e='in') if kind == 'norm' else dict(p='inout', g='in', m='inout', v='inout', e='inout')
        specs = []
        for i, n in enumerate(SIZES):
            pad = 1 if i in MISALIGNED else 0
            for col, _, scale in COLS:
                t = torch.rand(n + pad, generator=g) * 1e-3 if scale is None else rn(g, n + pad, scale=scale)
                if col == 'g' and i == NO_GRAD:
                    t[pad + 1] = float('nan')
                if col == 'g' and i == 7 and poison:
                    t[pad + n - 1] = float('inf')
                tensors[f'{col}{i}'] = t[pad:]
                specs.append((f'{col}{i}', t, roles[col]))
        counts = [-(-n // CHUNK) for n in SIZES]
        cmap = np.repeat(np.arange(n_t, dtype=np.int32), counts)
        start = dict(START, verdict=verdict)
        specs += [('table', torch.zeros(n_t, 8, dtype=torch.int64), 'in'), ('cmap', torch.from_numpy(cmap.copy()), 'in'),
                  ('state', state_words(start), 'inout' if kind == 'norm' else 'in')]
        if kind == 'norm':
            specs += [('norm', out(1), 'out'), ('coef', out(1), 'out')]
        else:
            specs.append(('coef', torch.tensor([0.37]), 'in'))

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
            args = (p(v['table']), p(v['cmap']), n_t, len(cmap))
            if kind == 'norm':
                return c.lib.dcf_guard_grad_norm(*args, 1.0, p(v['norm']), p(v['coef']), p(v['state']), c.stream())
            groups = (c.pkg._lib.DcfOptimGroup * 2)()
            for k, (wd, mode) in enumerate(((0.05, 0), (0.01, 1))):
                h = groups[k]
                h.lr, h.weight_decay, h.b1, h.b2, h.eps = 1e-3, wd, 0.9, 0.999, 1e-8
                h.one_minus_b1, h.one_minus_b2 = 1.0 - 0.9, 1.0 - 0.999
                h.bc1, h.sqrt_bc2 = 1.0 - 0.9 ** 3, math.sqrt(1.0 - 0.999 ** 3)
                h.mode = mode
            return c.lib.dcf_guard_adam_step(*args, ctypes.cast(groups, ctypes.c_void_p), 2, p(v['coef']), p(v['state']), 1, 0.999, c.stream())

        def verify(outputs):
            if kind == 'norm':
                table = [(tensors[f'g{i}'].numpy(), int(i == NO_GRAD)) for i in range(n_t)]
                want = G.judge(table, start)
                got = state_of(outputs['state'])
                norm, coef = float(outputs['norm']), outputs['coef'].cpu().view(torch.int32).item()
                print(f'GUARDNORM poison {poison}: record {got}, norm {norm!r}, coef bits {coef:#x}')
                assert got == want and want['verdict'] == int(poison), (got, want)
                assert (coef == 0 and math.isinf(norm)) if poison else (0 < outputs['coef'].item() <= 1 and math.isfinite(norm))
                return want['verdict']
            moved = 0
            for i, n in enumerate(SIZES):
                for col in 'pmve':
                    same = torch.equal(outputs[f'{col}{i}'][-n:].cpu().view(torch.int32), tensors[f'{col}{i}'].view(torch.int32)) if n else True
                    written = i != NO_GRAD if col != 'e' else i != NO_EMA
                    if verdict or not written or not n:
                        assert same, f'{col}{i} changed under verdict {verdict}'
                    else:
                        assert not same, f'{col}{i} did not move under verdict apply'
                        moved += 1
            print(f'GUARDADAM verdict {verdict}: {moved} tensors moved')
            return moved
        return specs, call, fixup, verify
    return make


case('dcf_guard_grad_norm', 'nine-tensors-finite', _guard('norm'))
case('dcf_guard_grad_norm', 'nine-tensors-inf-in-the-last-element', _guard('norm', poison=True))
case('dcf_guard_adam_step', 'nine-tensors-verdict-apply', _guard('adam', verdict=0))
case('dcf_guard_adam_step', 'nine-tensors-verdict-skip', _guard('adam', verdict=1))

EXCLUDED = {'dcf_guard_ext_version': 'no device operand: returns a constant',
            'dcf_guard_arm': 'no device operand is read or written: it names the state to the conv-gradient word (tests/test_gpu_guard.py)',
            'dcf_guard_disarm': 'no device operand (tests/test_gpu_guard.py)'}
