"""One entry per operator of the training extension (include/decafnet_hip_train.h, ``_lib.TRAIN_SIGNATURES``) for
tests/test_gpu_train_borders.py, in the format of tests/abi_cases.py: ``Case(export, tag, make, options)`` with ``make()`` ->
``(specs, call)``.

Shapes (B, T, C, b0): (2, 8, 8, 0) -- T % 4 == 0, one Philox block per four positions; (3, 10, 36, 5) -- T % 4 != 0, every element
draws its own, C no multiple of the 256-channel chunk, an interior seam; a tiny one, (1, 3, 4, 2), where the thread's 4 x 4 block
is larger than the operand.  Masks have a padded tail.  For the residual's backward each of dR / dH / dls is absent in turn,
``accumulate`` is 0 and 1, the masks are present and absent."""
import torch

from abi_cases import Case, gen, opt, out, p, rn, row_mask

CASES = []
SHAPES = [(2, 8, 8, 0), (3, 10, 36, 5), (1, 3, 4, 2)]
SEED = 0x5DEECE66D1234567 - (1 << 64)          # a key with both halves set, as the int64 the ABI takes
SITE_DROP, SITE_PATH = 3 << 16 | 1 << 4 | 2, 3 << 16 | 1 << 4 | 4


def case(export, tag, make):
    CASES.append(Case(export, tag, make, ()))


def _dropout(B, T, C, b0, pr, inplace):
    def make():
        g = gen(31, B, T, C, b0, pr)
        if inplace:
            return [('X', rn(g, B * T, C), 'inout')], \
                lambda c, v: c.lib.dcf_op_dropout(p(v['X']), p(v['X']), B, T, C, b0, SEED, SITE_DROP, pr, c.stream())
        return [('X', rn(g, B * T, C), 'in'), ('Y', out(B * T, C), 'out')], \
            lambda c, v: c.lib.dcf_op_dropout(p(v['X']), p(v['Y']), B, T, C, b0, SEED, SITE_DROP, pr, c.stream())
    return make


def _gelu_dropout(B, T, C, b0, pr, bwd):
    def make():
        g = gen(32, B, T, C, b0, pr)
        specs = [('X', rn(g, B * T, C, scale=2.0), 'in')]
        if not bwd:
            return specs + [('Y', out(B * T, C), 'out')], \
                lambda c, v: c.lib.dcf_op_gelu_dropout(p(v['X']), p(v['Y']), B, T, C, b0, SEED, SITE_DROP, pr, c.stream())
        return specs + [('dY', rn(g, B * T, C), 'in'), ('dX', out(B * T, C), 'out')], \
            lambda c, v: c.lib.dcf_op_gelu_dropout_bwd(p(v['X']), p(v['dY']), p(v['dX']), B, T, C, b0, SEED, SITE_DROP, pr, c.stream())
    return make


def _residual(B, T, C, b0, pd, pp, mR, mH):
    def make():
        g = gen(33, B, T, C, b0, pd, pp)
        specs = [('R', rn(g, B * T, C), 'in'), ('H', rn(g, B * T, C), 'in'), ('ls', rn(g, C), 'in'), ('Y', out(B * T, C), 'out')]
        if mR or mH:
            specs.append(('m', row_mask(g, B, T), 'in'))           # a block has one mask
        return specs, lambda c, v: c.lib.dcf_op_drop_residual(p(v['R']), opt(v, 'm') if mR else None, p(v['H']), opt(v, 'm') if mH else None,
                                                              p(v['ls']), p(v['Y']), B, T, C, b0, SEED, SITE_DROP, pd, SITE_PATH, pp, c.stream())
    return make


def _residual_bwd(B, T, C, b0, pd, pp, mR, mH, which, acc):
    def make():
        g = gen(34, B, T, C, b0, pd, pp)
        specs = [('dY', rn(g, B * T, C), 'in'), ('H', rn(g, B * T, C), 'in'), ('ls', rn(g, C), 'in')]
        if mR:
            specs.append(('mR', row_mask(g, B, T), 'in'))
        if mH:
            specs.append(('mH', row_mask(g, B, T, holes=False), 'in'))
        if 'r' in which:
            specs.append(('dR', out(B * T, C), 'out'))
        if 'h' in which:
            specs.append(('dH', out(B * T, C), 'out'))
        if 's' in which:
            specs.append(('dls', rn(g, C) if acc else out(C), 'inout' if acc else 'out'))
        return specs, lambda c, v: c.lib.dcf_op_drop_residual_bwd(p(v['dY']), p(v['H']), opt(v, 'mR'), opt(v, 'mH'), p(v['ls']), opt(v, 'dR'),
                                                                  opt(v, 'dH'), opt(v, 'dls'), B, T, C, b0, SEED, SITE_DROP, pd, SITE_PATH, pp, acc,
                                                                  c.stream())
    return make


for i, (B, T, C, b0) in enumerate(SHAPES):
    pr = (0.1, 0.5, 0.5)[i]
    tag = f'{B}x{T}x{C}-b{b0}-p{pr}'
    case('dcf_op_dropout', tag, _dropout(B, T, C, b0, pr, False))
    case('dcf_op_dropout', tag + '-inplace', _dropout(B, T, C, b0, pr, True))
    case('dcf_op_gelu_dropout', tag, _gelu_dropout(B, T, C, b0, pr, False))
    case('dcf_op_gelu_dropout_bwd', tag, _gelu_dropout(B, T, C, b0, pr, True))
    # the two residuals of a block: `skip * mask + ...` (:586, m_R) and `x + ... (h * mask)` (:589-590, m_H); then both, then none
    for mR, mH in [(1, 0), (0, 1), (1, 1), (0, 0)]:
        case('dcf_op_drop_residual', f'{tag}-path0.5-mR{mR}-mH{mH}', _residual(B, T, C, b0, pr, 0.5, mR, mH))
    case('dcf_op_drop_residual', f'{tag}-p0-mR0-mH1', _residual(B, T, C, b0, 0.0, 0.0, 0, 1))       # the layerscale_residual branch
    for which, acc, mR, mH in [('rhs', 0, 1, 1), ('hs', 1, 0, 1), ('rs', 0, 1, 0), ('rh', 0, 0, 1), ('s', 1, 1, 1), ('rhs', 1, 0, 0)]:
        case('dcf_op_drop_residual_bwd', f'{tag}-path0.5-{which}-acc{acc}-mR{mR}-mH{mH}', _residual_bwd(B, T, C, b0, pr, 0.5, mR, mH, which, acc))
    case('dcf_op_drop_residual_bwd', f'{tag}-p0-rhs-acc0-mR1-mH1', _residual_bwd(B, T, C, b0, 0.0, 0.0, 1, 1, 'rhs', 0))

EXCLUDED = {'dcf_train_ext_version': 'no device operand: returns a constant'}
