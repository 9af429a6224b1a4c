"""One entry per operator of the data-parallel extension (include/decafnet_hip_dist.h, ``_lib.DIST_SIGNATURES``) for
tests/test_gpu_dist_borders.py, in the format of tests/abi_cases.py: ``Case(export, tag, make, options)`` with ``make()`` ->
``(specs, call, fixup, verify)``; ``verify(outputs)`` checks the values of the plain run, which the arena runs must equal bit for bit.

dcf_dist_pack_grads: ONE table of twelve rows, n = 1, 3, 4, 5, 1023, 1024, 1025, CHUNK-1, CHUNK, CHUNK+1, 2 CHUNK+7 and one more of 5.
Every source is an operand of its own; two of them start one element into it (address = 4 mod 16: the element-at-a-time path, one
tensor below and one above a chunk), one row carries DCF_OPTIM_NO_GRAD (its source holds values that must not arrive), the extra
row has g == NULL without the flag.  The destinations are slices of one ``bucket`` operand, each at a multiple of 64 floats with at
least 64 floats of poison between two of them; in the ``dst-4mod16`` cases every slice starts one float later.  Scales 1, 0.5 and 1/3.
Expected: ``torch.mul(src, scale)`` bit for bit, +0 for the two rows without a gradient, the poison between the slices untouched.
The sources hold normal values of both signs, +-0, +-inf, the largest finite value and values whose products are subnormal."""
import numpy as np
import torch

from abi_cases import _ROW, Case, gen, p, rn

CASES = []
CHUNK = 4096
SIZES = [1, 3, 4, 5, 1023, 1024, 1025, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 7, 5]
MISALIGNED, NO_GRAD, NULL_G = (4, 9), 2, 11
ALIGN, GAP = 64, 64
POISON = 0x7fc0dead                             # a quiet NaN with a payload, as int32: neither fill of the arena
SPECIAL = [0.0, -0.0, float('inf'), -float('inf'), 3.4028234663852886e38, 1.1754943508222875e-38, -1.1754943508222875e-38, 2.8e-45,
           4.2e-45, 1.0, -3.0, 1.1754942106924411e-38]


def case(export, tag, make):
    CASES.append(Case(export, tag, make, ()))


def layout(shift):
    """-> (offsets in floats, length): slice i at a multiple of ALIGN (+ shift), GAP floats of poison at least after every slice"""
    offs, end = [], ALIGN
    for n in SIZES:
        offs.append(end + shift)
        end = -(-(end + shift + n) // ALIGN) * ALIGN + GAP
    return offs, end


def _pack(scale, shift):
    def make():
        g = gen(41, len(SIZES), shift)
        n_t = len(SIZES)
        specs, srcs = [], []
        for i, n in enumerate(SIZES):
            pad = 1 if i in MISALIGNED else 0
            t = rn(g, n + pad, scale=10.0 ** (i % 5 - 2))
            k = min(n, len(SPECIAL))
            t[pad:pad + k] = torch.tensor(SPECIAL[:k]) if i % 2 == 0 else torch.tensor(SPECIAL[-k:])
            specs.append((f'g{i}', t, 'in'))
            srcs.append(t[pad:])
        offs, length = layout(shift)
        bucket = torch.full((length,), POISON, dtype=torch.int32).view(torch.float32)
        counts = [-(-n // CHUNK) for n in SIZES]
        cmap = np.repeat(np.arange(n_t, dtype=np.int32), counts)
        specs += [('bucket', bucket, 'inout'), ('table', torch.zeros(n_t, 8, dtype=torch.int64), 'in'), ('cmap', torch.from_numpy(cmap.copy()), 'in')]

        def fixup(v, update):
            rec = np.zeros(n_t, dtype=_ROW)
            for i, n in enumerate(SIZES):
                rec['p'][i] = v['bucket'].data_ptr() + 4 * offs[i]
                rec['g'][i] = 0 if i == NULL_G else v[f'g{i}'].data_ptr() + (4 if i in MISALIGNED else 0)
                rec['n'][i], rec['flags'][i] = n, int(i == NO_GRAD)
                assert rec['p'][i] % 16 == 4 * shift and (i == NULL_G or rec['g'][i] % 16 == (4 if i in MISALIGNED else 0))
            rec['chunk0'] = np.cumsum(counts) - np.array(counts)
            update('table', torch.from_numpy(rec.view(np.int64).reshape(n_t, 8).copy()))

        def call(c, v):
            return c.lib.dcf_dist_pack_grads(p(v['table']), p(v['cmap']), n_t, len(cmap), scale, c.stream())

        def verify(outputs):
            got = outputs['bucket'].view(torch.int32)
            want = torch.full((length,), POISON, dtype=torch.int32, device=got.device)
            for i, n in enumerate(SIZES):
                if i in (NO_GRAD, NULL_G):
                    want[offs[i]:offs[i] + n] = 0                                  # +0
                else:
                    want[offs[i]:offs[i] + n] = torch.mul(srcs[i].to(got.device), scale).view(torch.int32)
            bad = (got != want).nonzero()
            moved = sum(n for i, n in enumerate(SIZES) if i not in (NO_GRAD, NULL_G))
            print(f'DISTPACK scale {scale!r} dst {4 * shift} mod 16: {moved} elements against torch.mul and {length - sum(SIZES)} poisoned '
                  f'floats between {n_t} slices, {bad.numel()} differ')
            assert not bad.numel(), f'element {int(bad[0])} of the bucket: {int(got[int(bad[0])]):#x}, expected {int(want[int(bad[0])]):#x}'
            return moved
        return specs, call, fixup, verify
    return make


for scale, name in ((1.0, '1'), (0.5, '0.5'), (1.0 / 3.0, 'third')):
    case('dcf_dist_pack_grads', f'twelve-rows-scale-{name}', _pack(scale, 0))
case('dcf_dist_pack_grads', 'twelve-rows-scale-third-dst-4mod16', _pack(1.0 / 3.0, 1))
case('dcf_dist_pack_grads', 'twelve-rows-scale-1-dst-4mod16', _pack(1.0, 1))

EXCLUDED = {'dcf_dist_ext_version': 'no device operand: returns a constant'}
