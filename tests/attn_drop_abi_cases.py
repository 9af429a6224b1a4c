"""One entry per operator of the attention-map-dropout extension (include/decafnet_hip_attn_drop.h, ``_lib.ATTN_DROP_TABLE``) for
tests/test_gpu_attn_drop_borders.py, in the format of tests/abi_cases.py: ``Case(export, tag, make, options)`` with ``make()`` ->
``(specs, call)``.

dcf_op_local_attn_drop(window = 0) / dcf_op_global_attn_drop_bwd and dcf_op_xattn_drop / _bwd: sequences of one, two and three blocks
of 32 keys and of a single key, heads of 16 to 128 channels, one and two channel chunks, masked and with a NULL mask (backward), each
output NULL in turn.  dcf_op_local_attn_drop / _bwd: the windows of the three kernel variants (5: unrolled to 9; 19; 31: the loop with packed keep bits; 35:
keep bits drawn per element), an odd T so that the last wave of the forward holds one query, C = 64 (one chunk, partly filled) and
C = 512 (two chunks), masked (``abi_cases.row_mask``: a padded tail and a hole); the backward with all three outputs, with each of them
NULL in turn and with a NULL mask.  dcf_op_channel_dropout: T = 1, a T that is no multiple of the rows a thread walks, out of place
and in place.  q, k, v ~ N(0, 1), dO ~ N(0, 1) on every row; p = 0.5, b0 = 3."""
from abi_cases import Case, gen, out, p, rn, row_mask

CASES = []
SEED, SITE, P_DROP, B0 = 0x1234567887654321, 2 << 16 | 1 << 4 | 6, 0.5, 3


def case(export, tag, make):
    CASES.append(Case(export, tag, make, ()))


def _fwd(B, T, C, heads, window):
    def make():
        g = gen(61, B, T, C, heads, window)
        specs = [(n, rn(g, B * T, C), 'in') for n in ('Q', 'K', 'V')] + [('mask', row_mask(g, B, T), 'in'), ('O', out(B * T, C), 'out')]

        def call(c, v):
            return c.lib.dcf_op_local_attn_drop(p(v['Q']), p(v['K']), p(v['V']), p(v['mask']), p(v['O']), B, T, C, heads, window, B0, SEED, SITE,
                                                P_DROP, c.stream())
        return specs, call
    return make


def _bwd(B, T, C, heads, window, masked=True, skip=None):
    def make():
        g = gen(62, B, T, C, heads, window)
        specs = [(n, rn(g, B * T, C), 'in') for n in ('Q', 'K', 'V', 'dO')]
        if masked:
            specs.append(('mask', row_mask(g, B, T), 'in'))
        specs += [(n, out(B * T, C), 'out') for n in ('dQ', 'dK', 'dV') if n != skip]

        def call(c, v):
            o = [p(v[n]) if n in v else None for n in ('dQ', 'dK', 'dV')]
            return c.lib.dcf_op_local_attn_drop_bwd(p(v['Q']), p(v['K']), p(v['V']), p(v['mask']) if masked else None, p(v['dO']), o[0], o[1], o[2],
                                                    B, T, C, heads, window, B0, SEED, SITE, P_DROP, c.stream())
        return specs, call
    return make


def _channel(B, T, C, in_place):
    def make():
        g = gen(63, B, T, C)
        specs = [('X', rn(g, B * T, C), 'inout')] if in_place else [('X', rn(g, B * T, C), 'in'), ('Y', out(B * T, C), 'out')]

        def call(c, v):
            return c.lib.dcf_op_channel_dropout(p(v['X']), p(v['X' if in_place else 'Y']), B, T, C, B0, SEED, 7 << 16 | 7, P_DROP, c.stream())
        return specs, call
    return make


def _dense(kind, B, T, Lk, C, heads, bwd, masked=True, skip=None):
    """global self attention (Lk = T, through window = 0 of the local export / dcf_op_global_attn_drop_bwd) or cross attention"""
    def make():
        g = gen(64, B, T, Lk, C, heads, bwd)
        specs = [('Q', rn(g, B * T, C), 'in'), ('K', rn(g, B * Lk, C), 'in'), ('V', rn(g, B * Lk, C), 'in')]
        if bwd:
            specs.append(('dO', rn(g, B * T, C), 'in'))
        if masked:
            specs.append(('mask', row_mask(g, B, Lk), 'in'))
        if bwd:
            specs += [(n, out(B * (T if n == 'dQ' else Lk), C), 'out') for n in ('dQ', 'dK', 'dV') if n != skip]
        else:
            specs.append(('O', out(B * T, C), 'out'))

        def call(c, v):
            tail = (B0, SEED, SITE, P_DROP, c.stream())
            m = p(v['mask']) if masked else None
            if not bwd:
                if kind == 'global':
                    return c.lib.dcf_op_local_attn_drop(p(v['Q']), p(v['K']), p(v['V']), m, p(v['O']), B, T, C, heads, 0, *tail)
                return c.lib.dcf_op_xattn_drop(p(v['Q']), p(v['K']), p(v['V']), m, p(v['O']), B, T, Lk, C, heads, *tail)
            o = [p(v[n]) if n in v else None for n in ('dQ', 'dK', 'dV')]
            if kind == 'global':
                return c.lib.dcf_op_global_attn_drop_bwd(p(v['Q']), p(v['K']), p(v['V']), m, p(v['dO']), o[0], o[1], o[2], B, T, C, heads, *tail)
            return c.lib.dcf_op_xattn_drop_bwd(p(v['Q']), p(v['K']), p(v['V']), m, p(v['dO']), o[0], o[1], o[2], B, T, Lk, C, heads, *tail)
        return specs, call
    return make


case('dcf_op_local_attn_drop', 'global-T65-d32', _dense('global', 2, 65, 65, 64, 2, False))
case('dcf_op_local_attn_drop', 'global-T33-d64-C512', _dense('global', 2, 33, 33, 512, 8, False))
case('dcf_op_global_attn_drop_bwd', 'T65-d32-masked', _dense('global', 2, 65, 65, 64, 2, True))
case('dcf_op_global_attn_drop_bwd', 'T33-d64-C512-unmasked', _dense('global', 1, 33, 33, 512, 8, True, masked=False))
case('dcf_op_global_attn_drop_bwd', 'T65-d32-no-dQ', _dense('global', 2, 65, 65, 64, 2, True, skip='dQ'))
case('dcf_op_global_attn_drop_bwd', 'T65-d32-no-dK', _dense('global', 2, 65, 65, 64, 2, True, skip='dK'))
case('dcf_op_global_attn_drop_bwd', 'T65-d32-no-dV', _dense('global', 2, 65, 65, 64, 2, True, skip='dV'))
case('dcf_op_xattn_drop', 'T37-Lk24-d32', _dense('cross', 2, 37, 24, 128, 4, False))
case('dcf_op_xattn_drop', 'T5-Lk1-d16', _dense('cross', 2, 5, 1, 64, 4, False))
case('dcf_op_xattn_drop', 'T37-Lk64-d128', _dense('cross', 2, 37, 64, 256, 2, False))
case('dcf_op_xattn_drop_bwd', 'T37-Lk24-d32', _dense('cross', 2, 37, 24, 128, 4, True))
case('dcf_op_xattn_drop_bwd', 'T37-Lk33-d64-unmasked', _dense('cross', 2, 37, 33, 128, 2, True, masked=False))
case('dcf_op_xattn_drop_bwd', 'T37-Lk64-d128-no-dQ', _dense('cross', 2, 37, 64, 256, 2, True, skip='dQ'))
case('dcf_op_xattn_drop_bwd', 'T37-Lk5-d16-no-dK', _dense('cross', 2, 37, 5, 64, 4, True, skip='dK'))
case('dcf_op_xattn_drop_bwd', 'T37-Lk5-d16-no-dV', _dense('cross', 2, 37, 5, 64, 4, True, skip='dV'))

for W in (5, 19, 31, 35):
    case('dcf_op_local_attn_drop', f'T37-C64-w{W}', _fwd(2, 37, 64, 2, W))
    case('dcf_op_local_attn_drop_bwd', f'T37-C64-w{W}', _bwd(2, 37, 64, 2, W))
case('dcf_op_local_attn_drop', 'T21-C512-w9', _fwd(2, 21, 512, 8, 9))
case('dcf_op_local_attn_drop', 'T1-C64-w9', _fwd(2, 1, 64, 2, 9))
case('dcf_op_local_attn_drop_bwd', 'T21-C512-w9', _bwd(2, 21, 512, 8, 9))
case('dcf_op_local_attn_drop_bwd', 'T37-C64-w9-unmasked', _bwd(1, 37, 64, 2, 9, masked=False))
case('dcf_op_local_attn_drop_bwd', 'T37-C64-w19-no-dQ', _bwd(2, 37, 64, 2, 19, skip='dQ'))
case('dcf_op_local_attn_drop_bwd', 'T37-C64-w35-no-dK', _bwd(2, 37, 64, 2, 35, skip='dK'))
case('dcf_op_local_attn_drop_bwd', 'T37-C64-w5-no-dV', _bwd(2, 37, 64, 2, 5, skip='dV'))
case('dcf_op_channel_dropout', 'T1-C4', _channel(3, 1, 4, False))
case('dcf_op_channel_dropout', 'T37-C68', _channel(2, 37, 68, False))
case('dcf_op_channel_dropout', 'T37-C68-in-place', _channel(2, 37, 68, True))

EXCLUDED = {'dcf_attn_drop_ext_version': 'no device operand: returns a constant'}
