"""One entry per operator of the attention-gradient extension (include/decafnet_hip_attn.h, ``_lib.ATTN_SIGNATURES``) for
tests/test_gpu_attn_ext_borders.py, in the format of tests/abi_cases.py: ``Case(export, tag, make, options)`` with ``make()`` ->
``(specs, call)``.

dcf_op_global_attn_bwd: T = 65 (one row past a tile: the second tile holds one row and 63 that must not be read) and T = 130 (two tiles
and a tail of two), masked (``abi_cases.row_mask``: a padded tail and a hole) and with a NULL mask, all three outputs and each of them
NULL in turn.  q, k, v ~ N(0, 1), dO ~ N(0, 1) on every row; head dimension 32 and 64."""
from abi_cases import Case, gen, out, p, rn, row_mask

CASES = []


def case(export, tag, make):
    CASES.append(Case(export, tag, make, ()))


def _global_bwd(B, T, C, heads, masked, skip=None):
    def make():
        g = gen(51, B, T, C, heads)
        specs = [(n, rn(g, B * T, C), 'in') for n in ('Q', 'K', 'V', 'dO')]
        if masked:
            specs.append(('mask', row_mask(g, B, T), 'in'))
        specs += [(n, out(B * T, C), 'out') for n in ('dQ', 'dK', 'dV') if n != skip]

        def call(c, v):
            o = [p(v[n]) if n in v else None for n in ('dQ', 'dK', 'dV')]
            return c.lib.dcf_op_global_attn_bwd(p(v['Q']), p(v['K']), p(v['V']), p(v['mask']) if masked else None, p(v['dO']), o[0], o[1], o[2],
                                                B, T, C, heads, c.stream())
        return specs, call
    return make


for T in (65, 130):
    case('dcf_op_global_attn_bwd', f'T{T}-d32-masked', _global_bwd(2, T, 64, 2, True))
    case('dcf_op_global_attn_bwd', f'T{T}-d64-unmasked', _global_bwd(1, T, 128, 2, False))
case('dcf_op_global_attn_bwd', 'T65-d64-masked-no-dQ', _global_bwd(2, 65, 64, 1, True, 'dQ'))
case('dcf_op_global_attn_bwd', 'T130-d32-masked-no-dK', _global_bwd(2, 130, 64, 2, True, 'dK'))
case('dcf_op_global_attn_bwd', 'T130-d32-unmasked-no-dV', _global_bwd(1, 130, 64, 2, False, 'dV'))

EXCLUDED = {'dcf_attn_ext_version': 'no device operand: returns a constant'}
