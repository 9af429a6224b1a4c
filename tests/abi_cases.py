"""One entry per operator export of the C ABI for tests/test_gpu_borders.py: a builder of the CPU operands with their roles and a call
through ``_lib`` on the placed device views.  Argument orders are those of include/decafnet_hip.h and of the ``Lib`` uses in the
tests/test_gpu_*.py files.

A case is ``Case(export, tag, make, options)``: ``make()`` -> ``(specs, call)`` or ``(specs, call, fixup)`` with

  specs : [(name, cpu_tensor, role[, row_bytes])], role in 'in' / 'out' / 'inout'   (tests/arena.py)
  call  : call(ctx, v) -> return code; v maps the names to device tensors, ctx has .pkg, .lib, .stream() and .model(key, factory)
  fixup : fixup(v, update) for operands that hold device addresses of other operands (the optimizer's row table)

``options`` are dcf_debug_set_option (name, value) pairs set around all three runs and reset to -1 afterwards.

Shapes: the smallest at which the addressing can still go wrong -- row counts that are no multiple of 64 / 128, B >= 2 (an interior
seam), odd T, T % 4 != 0 for the channel-major and scoring kernels, masks with a padded tail; a tiny one (one row, T of 1 to 3) where
the tile is far larger than the operand; and one shape per dispatch branch of the launch code.  Channel widths are the smallest the
export accepts for the branch."""
import ctypes
import math
from collections import namedtuple

import numpy as np
import torch

from conftest import Golden

Case = namedtuple('Case', 'export tag make options')
CASES = []

f32 = torch.float32


def case(export, tag, make, options=()):
    CASES.append(Case(export, tag, make, tuple(options)))


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def gen(*seed):
    return torch.Generator().manual_seed(abs(hash(tuple(int(s * 1000) if isinstance(s, float) else int(s) for s in seed))) % (2 ** 31))


def rn(g, *shape, scale=1.0, shift=0.0):
    return torch.randn(*shape, generator=g) * scale + shift


def out(*shape, dtype=f32):
    return torch.zeros(*shape, dtype=dtype)


def row_mask(g, B, T, holes=True):
    """(B*T) bytes: sequence 0 full, the others with a padded tail, a hole inside the valid part of the last"""
    m = torch.ones(B, T, dtype=torch.uint8)
    for b in range(1, B):
        n = int(torch.randint(max(T // 2, 1), T + 1, (1,), generator=g))
        m[b, n:] = 0
    if B == 1 and T > 4:
        m[0, T - max(T // 5, 1):] = 0
    if holes and T > 8:
        m[-1, 3] = 0
    return m.view(-1)


def opt(v, name):
    return p(v[name]) if name in v else None


# ================================================================================================ GEMM family
def _linear(M, N, K, act, nterms=None, bias=True):
    def make():
        g = gen(1, M, N, K, act)
        specs = [('A', rn(g, M, K), 'in'), ('W', rn(g, N, K, scale=1 / math.sqrt(K)), 'in'), ('C', out(M, N), 'out')]
        if bias:
            specs.append(('b', rn(g, N), 'in'))
        if nterms is None:
            return specs, lambda c, v: c.lib.dcf_op_linear(p(v['A']), p(v['W']), opt(v, 'b'), p(v['C']), M, N, K, act, c.stream())
        return specs, lambda c, v: c.lib.dcf_op_linear_split(p(v['A']), p(v['W']), opt(v, 'b'), p(v['C']), M, N, K, act, nterms, c.stream())
    return make


# N = 32 / 96 / 160 / 256 / 288 (the tile widths of the dispatch), partial row tiles, one row, K = 128 (the k-sliced kernel of the
# split path at small grids) and a grid large enough for the 64-row tile kernels
for M, N, K, act in [(130, 32, 32, 0), (1, 96, 32, 1), (77, 160, 64, 2), (77, 256, 32, 0), (3, 288, 32, 0), (77, 64, 128, 0)]:
    case('dcf_op_linear', f'{M}x{N}x{K}-act{act}', _linear(M, N, K, act))
case('dcf_op_linear', '77x32x32-nobias', _linear(77, 32, 32, 0, bias=False))
for M, N, K, act, nt in [(130, 32, 32, 0, 16), (1, 96, 32, 1, 6), (77, 160, 64, 2, 16), (77, 256, 32, 0, 6), (3, 288, 32, 0, 16),
                         (77, 64, 128, 1, 16), (77, 64, 128, 0, 6), (4200, 256, 32, 0, 16), (16500, 128, 32, 2, 6), (2, 256, 512, 0, 6)]:
    case('dcf_op_linear_split', f'{M}x{N}x{K}-act{act}-n{nt}', _linear(M, N, K, act, nterms=nt))


def _linear_cm(M, N, K, bias, nterms=None):
    def make():
        g = gen(2, M, N, K)
        specs = [('A', rn(g, K, M), 'in', M * 4), ('W', rn(g, N, K, scale=1 / math.sqrt(K)), 'in'), ('C', out(M, N), 'out')]
        if bias:
            specs.append(('b', rn(g, N), 'in'))
        if nterms is None:
            return specs, lambda c, v: c.lib.dcf_op_linear_cm(p(v['A']), p(v['W']), opt(v, 'b'), p(v['C']), M, N, K, c.stream())
        return specs, lambda c, v: c.lib.dcf_op_linear_cm_split(p(v['A']), p(v['W']), opt(v, 'b'), p(v['C']), M, N, K, nterms, c.stream())
    return make


for M, N, K, bias in [(77, 32, 32, 1), (250, 64, 32, 0), (3, 96, 64, 1), (1, 32, 32, 1), (130, 256, 32, 0)]:      # T % 4 != 0
    case('dcf_op_linear_cm', f'{M}x{N}x{K}-b{bias}', _linear_cm(M, N, K, bias))
for M, N, K, nt in [(132, 128, 32, 16), (4, 128, 32, 6), (1000, 256, 64, 16), (68, 128, 96, 6)]:                  # needs M % 4 == 0, N % 128 == 0
    case('dcf_op_linear_cm_split', f'{M}x{N}x{K}-n{nt}', _linear_cm(M, N, K, 1, nterms=nt))


def _linear_ln(M, K, relu, raw, nterms):
    def make():
        g = gen(3, M, K)
        N = 256
        specs = [('A', rn(g, M, K, scale=2.0), 'in'), ('W', rn(g, N, K, scale=1 / math.sqrt(K)), 'in'), ('b', rn(g, N), 'in'),
                 ('lw', torch.rand(N, generator=g) + 0.5, 'in'), ('lb', rn(g, N), 'in'), ('Y', out(M, N), 'out')]
        if raw:
            specs.append(('C', out(M, N), 'out'))
        return specs, lambda c, v: c.lib.dcf_op_linear_ln(p(v['A']), p(v['W']), p(v['b']), p(v['lw']), p(v['lb']), opt(v, 'C'), p(v['Y']),
                                                          M, N, K, relu, nterms, c.stream())
    return make


# only the shapes the engine fuses exist: N = 256, at least 448 row tiles; the last row tile partial
case('dcf_op_linear_ln', '28700x256x32-relu-raw-f16', _linear_ln(28700, 32, 1, True, 16))
case('dcf_op_linear_ln', '28610x256x64-bf16', _linear_ln(28610, 64, 0, False, 6))


def _ln_carry(M, N1, K1, N2, res, gelu, nterms):
    def make():
        g = gen(4, M, N1, K1, N2)
        specs = [('A', rn(g, M, K1), 'in'), ('W1', rn(g, N1, K1, scale=1 / math.sqrt(K1)), 'in'), ('b1', rn(g, N1, scale=0.3), 'in'),
                 ('lw', torch.rand(N1, generator=g) + 0.5, 'in'), ('lb', rn(g, N1, scale=0.5), 'in'),
                 ('W2', rn(g, N2, N1, scale=1 / math.sqrt(N1)), 'in'), ('b2', rn(g, N2, scale=0.3), 'in'),
                 ('X', out(M, N1), 'out'), ('Y', out(M, N2), 'out')]
        if res:
            specs.append(('R', rn(g, M, N1), 'in'))
        return specs, lambda c, v: c.lib.dcf_op_linear_ln_carry(p(v['A']), p(v['W1']), p(v['b1']), opt(v, 'R'), p(v['lw']), p(v['lb']), p(v['W2']),
                                                                p(v['b2']), p(v['X']), p(v['Y']), M, N1, K1, N2, gelu, nterms, c.stream())
    return make


# K < 128 never takes the k-sliced kernel, so small row counts carry statistics there; at K >= 128 only grids of more than 256
# 64 x 64 tiles do; 1 / 2 / 4 statistics slots per row
case('dcf_op_linear_ln_carry', '77x64x32-64', _ln_carry(77, 64, 32, 64, 1, 1, 16))
case('dcf_op_linear_ln_carry', '1x64x32-128', _ln_carry(1, 64, 32, 128, 0, 0, 6))
case('dcf_op_linear_ln_carry', '4200x128x64-256', _ln_carry(4200, 128, 64, 256, 1, 0, 16))
case('dcf_op_linear_ln_carry', '8200x256x128-256', _ln_carry(8200, 256, 128, 256, 0, 1, 16))


def _ffn(M, E, chain, with_ln, with_ls, with_mask, with_stats):
    def make():
        g = gen(5, M, E, chain)
        specs = [('X', rn(g, M, E), 'in'), ('W1', rn(g, 4 * E, E, scale=1 / math.sqrt(E)), 'in'), ('b1', rn(g, 4 * E, scale=0.3), 'in'),
                 ('W2', rn(g, E, 4 * E, scale=1 / math.sqrt(4 * E)), 'in'), ('b2', rn(g, E, scale=0.3), 'in'), ('C', out(M, E), 'out')]
        if with_ln:
            specs += [('lw', torch.rand(E, generator=g) + 0.5, 'in'), ('lb', rn(g, E, scale=0.5), 'in')]
        if with_ls:
            specs.append(('ls', rn(g, E), 'in'))
        if with_mask:
            specs.append(('mask', (torch.rand(M, generator=g) > 0.3).to(torch.uint8), 'in'))
        if with_stats:
            specs.append(('S', out(M, E // 64, 2), 'out'))
        return specs, lambda c, v: c.lib.dcf_op_ffn(p(v['X']), opt(v, 'lw'), opt(v, 'lb'), p(v['W1']), p(v['b1']), p(v['W2']), p(v['b2']), opt(v, 'ls'),
                                                    opt(v, 'mask'), p(v['C']), opt(v, 'S'), M, E, chain, c.stream())
    return make


for chain in (0, 1, 2, 3):                                  # `chain` of dcf_op_ffn: the GEMM pair and the three one-kernel forms
    case('dcf_op_ffn', f'77x256-chain{chain}-ln-ls-mask', _ffn(77, 256, chain, 1, 1, 1, int(chain > 0)))
    case('dcf_op_ffn', f'1x256-chain{chain}', _ffn(1, 256, chain, 0, 0, 0, 0))
case('dcf_op_ffn', '130x64-chain0-ln-mask', _ffn(130, 64, 0, 1, 0, 1, 0))
case('dcf_op_ffn', '300x256-chain3-stats', _ffn(300, 256, 3, 0, 1, 1, 1))


# ================================================================================================ convolutions, heads, LayerNorm
def _conv3(B, T, Cin, N, nterms=None):
    def make():
        g = gen(6, B, T, Cin, N)
        specs = [('X', rn(g, B * T, Cin), 'in'), ('mask', row_mask(g, B, T), 'in'), ('W', rn(g, N, Cin, 3, scale=1 / math.sqrt(3 * Cin)), 'in'),
                 ('Y', out(B * T, N), 'out')]
        if nterms is None:
            return specs, lambda c, v: c.lib.dcf_op_conv3(p(v['X']), p(v['mask']), p(v['W']), p(v['Y']), B, T, Cin, N, c.stream())
        return specs, lambda c, v: c.lib.dcf_op_conv3_split(p(v['X']), p(v['mask']), p(v['W']), p(v['Y']), B, T, Cin, N, nterms, c.stream())
    return make


for B, T, Cin, N in [(2, 39, 32, 32), (2, 65, 32, 96), (3, 43, 32, 160), (2, 39, 64, 256), (2, 39, 32, 288), (1, 1, 32, 32), (2, 3, 32, 96)]:
    case('dcf_op_conv3', f'{B}x{T}-{Cin}-{N}', _conv3(B, T, Cin, N))
for B, T, Cin, N, nt in [(2, 39, 32, 32, 16), (2, 65, 32, 96, 6), (3, 43, 32, 160, 16), (2, 39, 64, 256, 6), (2, 39, 32, 288, 16), (1, 1, 32, 32, 6),
                         (2, 3, 32, 96, 16), (2, 2111, 32, 256, 16)]:
    case('dcf_op_conv3_split', f'{B}x{T}-{Cin}-{N}-n{nt}', _conv3(B, T, Cin, N, nterms=nt))


def _head(B, T, C, NO, scale, chain):
    def make():
        g = gen(7, B, T, C, NO)
        w = lambda: rn(g, C, C, 3, scale=1 / math.sqrt(3 * C))
        specs = [('X', rn(g, B * T, C), 'in'), ('mask', row_mask(g, B, T), 'in'), ('W1', w(), 'in'), ('W2', w(), 'in'),
                 ('l1w', torch.rand(C, generator=g) + 0.5, 'in'), ('l1b', rn(g, C, scale=0.3), 'in'),
                 ('l2w', torch.rand(C, generator=g) + 0.5, 'in'), ('l2b', rn(g, C, scale=0.3), 'in'),
                 ('Wo', rn(g, NO, C, 3, scale=1 / math.sqrt(3 * C)), 'in'), ('bo', rn(g, NO), 'in'), ('out', out(B * T, NO), 'out')]
        return specs, lambda c, v: c.lib.dcf_op_head(p(v['X']), p(v['mask']), p(v['W1']), p(v['l1w']), p(v['l1b']), p(v['W2']), p(v['l2w']), p(v['l2b']),
                                                     p(v['Wo']), p(v['bo']), p(v['out']), B, T, C, NO, scale, chain, c.stream())
    return make


# the one-kernel form (C = 256 / 288; a 104-row tile: shorter, longer, several sequences) and the separate launches; NO = 1 / 2
for B, T, C, NO, scale, chain in [(2, 39, 256, 1, 0.0, 1), (2, 131, 288, 2, 1.7, 1), (1, 3, 256, 2, 0.6, 1), (1, 1, 288, 1, 0.0, 1),
                                  (2, 39, 32, 1, 0.0, 0), (3, 43, 64, 2, 1.7, 0), (1, 1, 32, 2, 0.6, 0), (2, 39, 256, 2, 1.7, 0)]:
    case('dcf_op_head', f'{B}x{T}-{C}-no{NO}-chain{chain}', _head(B, T, C, NO, scale, chain))


def _layernorm(rows, C, relu, affine):
    def make():
        g = gen(8, rows, C)
        specs = [('X', rn(g, rows, C, scale=3.0, shift=1.0), 'in'), ('Y', out(rows, C), 'out')]
        if affine:
            specs += [('w', rn(g, C), 'in'), ('b', rn(g, C), 'in')]
        return specs, lambda c, v: c.lib.dcf_op_layernorm(p(v['X']), opt(v, 'w'), opt(v, 'b'), p(v['Y']), rows, C, relu, c.stream())
    return make


for rows, C, relu, aff in [(77, 32, 0, 1), (77, 288, 1, 0), (1, 256, 0, 1), (3, 1024, 1, 1), (130, 4, 0, 1)]:
    case('dcf_op_layernorm', f'{rows}x{C}-relu{relu}-aff{aff}', _layernorm(rows, C, relu, aff))


def _conv_bwd_data(B, T, Cin, N, k, masked=True):
    def make():
        g = gen(9, B, T, Cin, N, k)
        specs = [('dY', rn(g, B * T, N), 'in'), ('W', rn(g, N, Cin, k, scale=1 / math.sqrt(k * Cin)), 'in'), ('dX', out(B * T, Cin), 'out')]
        if masked:
            specs.append(('mask', row_mask(g, B, T), 'in'))
        return specs, lambda c, v: c.lib.dcf_op_conv_bwd_data(p(v['dY']), opt(v, 'mask'), p(v['W']), p(v['dX']), B, T, Cin, N, k, c.stream())
    return make


def _conv_bwd_weight(B, T, Cin, N, k, acc, with_db=True):
    def make():
        g = gen(10, B, T, Cin, N, k)
        specs = [('X', rn(g, B * T, Cin), 'in'), ('mask', row_mask(g, B, T), 'in'), ('dY', rn(g, B * T, N), 'in'),
                 ('dW', rn(g, N, Cin, k) if acc else out(N, Cin, k), 'inout' if acc else 'out')]
        if with_db:
            specs.append(('db', rn(g, N) if acc else out(N), 'inout' if acc else 'out'))
        return specs, lambda c, v: c.lib.dcf_op_conv_bwd_weight(p(v['X']), p(v['mask']), p(v['dY']), p(v['dW']), opt(v, 'db'), B, T, Cin, N, k, acc,
                                                                c.stream())
    return make


# N = 1 / 2 (the heads' output convolutions, vector ALU) and the matrix-core widths, k = 1 / 3, accumulate 0 / 1
for B, T, Cin, N, k in [(2, 39, 32, 1, 3), (2, 39, 64, 2, 3), (2, 77, 32, 32, 3), (3, 43, 32, 96, 1), (2, 39, 32, 160, 3), (2, 39, 32, 256, 1),
                        (2, 39, 32, 288, 3), (1, 1, 32, 32, 3), (1, 3, 32, 2, 3), (2, 130, 256, 32, 3)]:
    case('dcf_op_conv_bwd_data', f'{B}x{T}-{Cin}-{N}-k{k}', _conv_bwd_data(B, T, Cin, N, k))
    case('dcf_op_conv_bwd_weight', f'{B}x{T}-{Cin}-{N}-k{k}-acc{(T + N) % 2}', _conv_bwd_weight(B, T, Cin, N, k, (T + N) % 2))
case('dcf_op_conv_bwd_data', '2x39-32-32-k3-nomask', _conv_bwd_data(2, 39, 32, 32, 3, masked=False))
case('dcf_op_conv_bwd_weight', '2x39-32-32-k3-acc1-nodb', _conv_bwd_weight(2, 39, 32, 32, 3, 1, with_db=False))
case('dcf_op_conv_bwd_weight', '2x39-32-1-k3-acc1', _conv_bwd_weight(2, 39, 32, 1, 3, 1))
case('dcf_op_conv_bwd_weight', '2x300-32-64-k3-acc0', _conv_bwd_weight(2, 300, 32, 64, 3, 0))          # several row slices


def _layernorm_bwd(rows, C, relu, acc, affine=True):
    def make():
        g = gen(11, rows, C)
        specs = [('X', rn(g, rows, C, scale=2.0, shift=0.5), 'in'), ('dOut', rn(g, rows, C), 'in'), ('dX', out(rows, C), 'out')]
        if affine:
            specs += [('w', rn(g, C), 'in'), ('b', rn(g, C), 'in'), ('dw', rn(g, C) if acc else out(C), 'inout' if acc else 'out'),
                      ('db', rn(g, C) if acc else out(C), 'inout' if acc else 'out')]
        return specs, lambda c, v: c.lib.dcf_op_layernorm_bwd(p(v['X']), opt(v, 'w'), opt(v, 'b'), p(v['dOut']), p(v['dX']), opt(v, 'dw'), opt(v, 'db'),
                                                              rows, C, relu, acc, c.stream())
    return make


for rows, C, relu, acc, aff in [(77, 32, 1, 0, 1), (1, 288, 0, 1, 1), (130, 1024, 1, 1, 1), (3, 64, 0, 0, 0), (300, 32, 0, 0, 1)]:
    case('dcf_op_layernorm_bwd', f'{rows}x{C}-relu{relu}-acc{acc}-aff{aff}', _layernorm_bwd(rows, C, relu, acc, aff))


def _conv5s2(kind, B, T, Cin, N, nterms=16, acc=0):
    def make():
        g = gen(12, B, T, Cin, N)
        To = T // 2
        W = rn(g, N, Cin, 5, scale=1 / math.sqrt(5 * Cin))
        mask = row_mask(g, B, T)
        if kind == 'fwd':
            specs = [('X', rn(g, B * T, Cin), 'in'), ('mask', mask, 'in'), ('W', W, 'in'), ('Y', out(B * To, N), 'out')]
            return specs, lambda c, v: c.lib.dcf_op_conv5s2_split(p(v['X']), p(v['mask']), p(v['W']), p(v['Y']), B, T, Cin, N, nterms, c.stream())
        if kind == 'data':
            specs = [('dY', rn(g, B * To, N), 'in'), ('mask', mask, 'in'), ('W', W, 'in'), ('dX', out(B * T, Cin), 'out')]
            return specs, lambda c, v: c.lib.dcf_op_conv5s2_bwd_data(p(v['dY']), p(v['mask']), p(v['W']), p(v['dX']), B, T, Cin, N, c.stream())
        specs = [('X', rn(g, B * T, Cin), 'in'), ('mask', mask, 'in'), ('dY', rn(g, B * To, N), 'in'),
                 ('dW', rn(g, N, Cin, 5) if acc else out(N, Cin, 5), 'inout' if acc else 'out')]
        return specs, lambda c, v: c.lib.dcf_op_conv5s2_bwd_weight(p(v['X']), p(v['mask']), p(v['dY']), p(v['dW']), B, T, Cin, N, acc, c.stream())
    return make


for B, T, Cin, N, nt in [(2, 38, 32, 32, 16), (1, 2, 32, 96, 6), (3, 130, 32, 160, 16), (2, 38, 64, 256, 6), (2, 6, 32, 288, 16)]:
    case('dcf_op_conv5s2_split', f'{B}x{T}-{Cin}-{N}-n{nt}', _conv5s2('fwd', B, T, Cin, N, nt))
    case('dcf_op_conv5s2_bwd_data', f'{B}x{T}-{Cin}-{N}', _conv5s2('data', B, T, Cin, N))
    case('dcf_op_conv5s2_bwd_weight', f'{B}x{T}-{Cin}-{N}-acc{B % 2}', _conv5s2('weight', B, T, Cin, N, acc=B % 2))


# ================================================================================================ attention
def _xattn(B, T, Lk, C, heads, bwd=False, masked=True, which='qkv'):
    def make():
        g = gen(13, B, T, Lk, C)
        kvm = torch.ones(B, Lk, dtype=torch.uint8)
        if Lk > 1:
            kvm[-1, (Lk + 1) // 2:] = 0
        specs = [('Q', rn(g, B * T, C), 'in'), ('K', rn(g, B * Lk, C), 'in'), ('V', rn(g, B * Lk, C), 'in')]
        if masked:
            specs.append(('kvmask', kvm.view(-1), 'in'))
        if not bwd:
            specs.append(('O', out(B * T, C), 'out'))
            return specs, lambda c, v: c.lib.dcf_op_xattn(p(v['Q']), p(v['K']), p(v['V']), opt(v, 'kvmask'), p(v['O']), B, T, Lk, C, heads, c.stream())
        specs.append(('dO', rn(g, B * T, C), 'in'))
        for n, rows in (('dQ', B * T), ('dK', B * Lk), ('dV', B * Lk)):
            if n[1].lower() in which:
                specs.append((n, out(rows, C), 'out'))
        return specs, lambda c, v: c.lib.dcf_op_xattn_bwd(p(v['Q']), p(v['K']), p(v['V']), opt(v, 'kvmask'), p(v['dO']), opt(v, 'dQ'), opt(v, 'dK'),
                                                          opt(v, 'dV'), B, T, Lk, C, heads, c.stream())
    return make


# head dims 16 / 32 / 64 / 128 on the matrix-core kernel with 0 .. 4 key tiles and 0 .. 2 trailing keys, head dim 8 on the vector ALU
for B, T, Lk, C, heads in [(2, 77, 17, 64, 4), (1, 3, 5, 128, 2), (2, 39, 33, 32, 4), (1, 1, 64, 64, 2), (2, 130, 1, 256, 2), (3, 43, 48, 128, 4),
                           (2, 39, 34, 64, 2)]:
    case('dcf_op_xattn', f'{B}x{T}-k{Lk}-{C}-h{heads}', _xattn(B, T, Lk, C, heads))
case('dcf_op_xattn', '2x39-k70-32-h4-valu', _xattn(2, 39, 70, 32, 4))
for B, T, Lk, C, heads in [(2, 77, 17, 64, 4), (1, 3, 5, 128, 2), (1, 1, 64, 64, 2), (2, 130, 1, 256, 2), (2, 600, 33, 128, 4)]:
    case('dcf_op_xattn_bwd', f'{B}x{T}-k{Lk}-{C}-h{heads}', _xattn(B, T, Lk, C, heads, bwd=True))
case('dcf_op_xattn_bwd', '2x77-k17-64-h4-dQ-only-nomask', _xattn(2, 77, 17, 64, 4, bwd=True, masked=False, which='q'))
case('dcf_op_xattn_bwd', '2x77-k17-64-h4-dKdV', _xattn(2, 77, 17, 64, 4, bwd=True, which='kv'))


def _local_attn(B, T, C, heads, w, bwd=False, which='qkv', masked=True):
    def make():
        g = gen(14, B, T, C, w)
        specs = [('Q', rn(g, B * T, C), 'in'), ('K', rn(g, B * T, C), 'in'), ('V', rn(g, B * T, C), 'in')]
        if masked:
            specs.append(('mask', row_mask(g, B, T), 'in'))
        if not bwd:
            specs.append(('O', out(B * T, C), 'out'))
            return specs, lambda c, v: c.lib.dcf_op_local_attn(p(v['Q']), p(v['K']), p(v['V']), opt(v, 'mask'), p(v['O']), B, T, C, heads, w, c.stream())
        specs.append(('dO', rn(g, B * T, C), 'in'))
        for n in ('dQ', 'dK', 'dV'):
            if n[1].lower() in which:
                specs.append((n, out(B * T, C), 'out'))
        return specs, lambda c, v: c.lib.dcf_op_local_attn_bwd(p(v['Q']), p(v['K']), p(v['V']), opt(v, 'mask'), p(v['dO']), opt(v, 'dQ'), opt(v, 'dK'),
                                                               opt(v, 'dV'), B, T, C, heads, w, c.stream())
    return make


# window 5 / 9 (the EAGER kernel below 8193 rows, C <= 256), 19, above 19 (the any-window kernel), 0 (global); C % 256 == 0 and not;
# two chunks per row (C = 512: never EAGER); odd T (the second row of a wave's pair is missing at a sequence end); one to three rows
for B, T, C, heads, w in [(2, 39, 64, 2, 5), (3, 43, 256, 4, 9), (2, 39, 32, 4, 19), (2, 39, 64, 2, 71), (2, 1, 256, 4, 9), (1, 3, 128, 4, 5),
                          (2, 39, 512, 8, 9), (2, 2, 64, 2, 19), (2, 77, 64, 2, 0), (1, 3, 128, 4, 0), (3, 65, 256, 4, 0)]:
    case('dcf_op_local_attn', f'{B}x{T}-{C}-h{heads}-w{w}', _local_attn(B, T, C, heads, w))
for B, T, C, heads, w in [(2, 39, 64, 2, 5), (3, 43, 256, 4, 9), (2, 39, 32, 4, 19), (2, 39, 64, 2, 71), (2, 1, 256, 4, 9), (1, 3, 128, 4, 5),
                          (2, 39, 512, 8, 9)]:
    case('dcf_op_local_attn_bwd', f'{B}x{T}-{C}-h{heads}-w{w}', _local_attn(B, T, C, heads, w, bwd=True))
case('dcf_op_local_attn_bwd', '2x39-64-h2-w9-dQ-only-nomask', _local_attn(2, 39, 64, 2, 9, bwd=True, which='q', masked=False))
case('dcf_op_local_attn_bwd', '2x39-64-h2-w9-dKdV', _local_attn(2, 39, 64, 2, 9, bwd=True, which='kv'))


# ================================================================================================ encoder-block pieces
def _dwconv3(B, T, C, n, stride, bwd=False, acc=0, which='xw'):
    def make():
        g = gen(15, B, T, C, n, stride)
        To = T // stride
        specs = [('X', rn(g, B * T, C), 'in'), ('mask', row_mask(g, B, T), 'in'), ('W', rn(g, n, C, 3, scale=0.6), 'in')]
        if not bwd:
            specs.append(('Y', out(n, B * To, C), 'out'))
            return specs, lambda c, v: c.lib.dcf_op_dwconv3(p(v['X']), p(v['mask']), p(v['W']), p(v['Y']), B, T, C, n, stride, c.stream())
        specs.append(('dY', rn(g, n, B * To, C), 'in'))
        if 'x' in which:
            specs.append(('dX', out(B * T, C), 'out'))
        if 'w' in which:
            specs.append(('dW', rn(g, n, C, 3) if acc else out(n, C, 3), 'inout' if acc else 'out'))
        return specs, lambda c, v: c.lib.dcf_op_dwconv3_bwd(p(v['X']), p(v['mask']), p(v['W']), p(v['dY']), opt(v, 'dX'), opt(v, 'dW'), B, T, C, n, stride,
                                                            acc, c.stream())
    return make


for B, T, C, n, stride in [(2, 39, 32, 3, 1), (2, 38, 64, 3, 2), (3, 43, 4, 1, 1), (1, 1, 256, 3, 1), (1, 2, 32, 1, 2), (2, 3, 1024, 2, 1), (2, 130, 36, 3, 2)]:
    case('dcf_op_dwconv3', f'{B}x{T}-{C}-n{n}-s{stride}', _dwconv3(B, T, C, n, stride))
    case('dcf_op_dwconv3_bwd', f'{B}x{T}-{C}-n{n}-s{stride}-acc{T % 2}', _dwconv3(B, T, C, n, stride, bwd=True, acc=T % 2))
case('dcf_op_dwconv3_bwd', '2x39-32-n3-s1-dX-only', _dwconv3(2, 39, 32, 3, 1, bwd=True, which='x'))
case('dcf_op_dwconv3_bwd', '2x300-32-n3-s1-dW-only', _dwconv3(2, 300, 32, 3, 1, bwd=True, which='w'))


def _maxpool(B, T, C, bwd=False, mask_out=True):
    def make():
        g = gen(16, B, T, C)
        X = rn(g, B * T, C)
        k = X[1::3].size(0)
        X[::3][:k] = X[1::3]                                                     # ties between neighbours
        specs = [('X', X, 'in'), ('mask', row_mask(g, B, T), 'in')]
        if not bwd:
            specs.append(('Y', out(B * T // 2, C), 'out'))
            if mask_out:
                specs.append(('mo', out(B * T // 2, dtype=torch.uint8), 'out'))
            return specs, lambda c, v: c.lib.dcf_op_masked_maxpool(p(v['X']), p(v['mask']), p(v['Y']), opt(v, 'mo'), B, T, C, c.stream())
        specs += [('dY', rn(g, B * T // 2, C), 'in'), ('dX', out(B * T, C), 'out')]
        return specs, lambda c, v: c.lib.dcf_op_masked_maxpool_bwd(p(v['X']), p(v['mask']), p(v['dY']), p(v['dX']), B, T, C, c.stream())
    return make


for B, T, C in [(2, 38, 32), (3, 42, 4), (1, 2, 256), (2, 130, 36), (2, 6, 1024)]:
    case('dcf_op_masked_maxpool', f'{B}x{T}-{C}', _maxpool(B, T, C))
    case('dcf_op_masked_maxpool_bwd', f'{B}x{T}-{C}', _maxpool(B, T, C, bwd=True))
case('dcf_op_masked_maxpool', '2x38-32-no-mask-out', _maxpool(2, 38, 32, mask_out=False))


def _gelu(n, bwd=False):
    def make():
        g = gen(17, n)
        specs = [('X', rn(g, n, scale=3.0), 'in')]
        if not bwd:
            return specs + [('Y', out(n), 'out')], lambda c, v: c.lib.dcf_op_gelu(p(v['X']), p(v['Y']), n, c.stream())
        specs += [('dY', rn(g, n), 'in'), ('dX', out(n), 'out')]
        return specs, lambda c, v: c.lib.dcf_op_gelu_bwd(p(v['X']), p(v['dY']), p(v['dX']), n, c.stream())
    return make


for n in (1, 3, 385, 4099):                                 # n % 4 != 0: the last 16-byte group is partial
    case('dcf_op_gelu', f'n{n}', _gelu(n))
    case('dcf_op_gelu_bwd', f'n{n}', _gelu(n, bwd=True))


def _lsres(rows, C, mR, mH, withH=True, bwd=False, acc=0):
    def make():
        g = gen(18, rows, C, mR, mH)
        specs = []
        if mR:
            specs.append(('mR', (torch.rand(rows, generator=g) > 0.3).to(torch.uint8), 'in'))
        if mH:
            specs.append(('mH', (torch.rand(rows, generator=g) > 0.3).to(torch.uint8), 'in'))
        if withH:
            specs += [('H', rn(g, rows, C), 'in'), ('ls', rn(g, C), 'in')]
        if not bwd:
            specs += [('R', rn(g, rows, C), 'in'), ('Y', out(rows, C), 'out')]
            return specs, lambda c, v: c.lib.dcf_op_layerscale_residual(p(v['R']), opt(v, 'mR'), opt(v, 'H'), opt(v, 'mH'), opt(v, 'ls'), p(v['Y']), rows, C,
                                                                        c.stream())
        specs += [('dY', rn(g, rows, C), 'in'), ('dR', out(rows, C), 'out')]
        if withH:
            specs += [('dH', out(rows, C), 'out'), ('dls', rn(g, C) if acc else out(C), 'inout' if acc else 'out')]
        return specs, lambda c, v: c.lib.dcf_op_layerscale_residual_bwd(p(v['dY']), opt(v, 'H'), opt(v, 'mR'), opt(v, 'mH'), opt(v, 'ls'), p(v['dR']),
                                                                        opt(v, 'dH'), opt(v, 'dls'), rows, C, acc, c.stream())
    return make


for rows, C, mR, mH, withH in [(77, 32, 0, 1, 1), (77, 256, 1, 0, 1), (1, 4, 1, 1, 1), (3, 1024, 0, 0, 1), (130, 36, 1, 0, 0), (300, 32, 0, 1, 1)]:
    case('dcf_op_layerscale_residual', f'{rows}x{C}-mR{mR}-mH{mH}-H{withH}', _lsres(rows, C, mR, mH, withH))
    case('dcf_op_layerscale_residual_bwd', f'{rows}x{C}-mR{mR}-mH{mH}-H{withH}-acc{rows % 2}', _lsres(rows, C, mR, mH, withH, bwd=True, acc=rows % 2))


def _adaln(rows, C, norm, masked, bwd=False, which='xh'):
    def make():
        g = gen(19, rows, C, norm)
        specs = [('X', rn(g, rows, C, scale=1.5, shift=0.3), 'in'), ('H', rn(g, rows, 2 * C), 'in')]
        if masked:
            specs.append(('mask', (torch.rand(rows, generator=g) > 0.3).to(torch.uint8), 'in'))
        if not bwd:
            specs.append(('Y', out(rows, C), 'out'))
            return specs, lambda c, v: c.lib.dcf_op_adaln(p(v['X']), opt(v, 'mask'), p(v['H']), p(v['Y']), rows, C, norm, c.stream())
        specs.append(('dY', rn(g, rows, C), 'in'))
        if 'x' in which:
            specs.append(('dX', out(rows, C), 'out'))
        if 'h' in which:
            specs.append(('dH', out(rows, 2 * C), 'out'))
        return specs, lambda c, v: c.lib.dcf_op_adaln_bwd(p(v['X']), opt(v, 'mask'), p(v['H']), p(v['dY']), opt(v, 'dX'), opt(v, 'dH'), rows, C, norm,
                                                          c.stream())
    return make


for rows, C, norm, masked in [(77, 32, 1, 1), (77, 256, 0, 1), (1, 4, 1, 0), (3, 1024, 1, 1), (130, 36, 0, 0)]:
    case('dcf_op_adaln', f'{rows}x{C}-norm{norm}-m{masked}', _adaln(rows, C, norm, masked))
    case('dcf_op_adaln_bwd', f'{rows}x{C}-norm{norm}-m{masked}', _adaln(rows, C, norm, masked, bwd=True))
case('dcf_op_adaln_bwd', '77x32-norm1-dX-only', _adaln(77, 32, 1, 1, bwd=True, which='x'))
case('dcf_op_adaln_bwd', '77x32-norm1-dH-only', _adaln(77, 32, 1, 1, bwd=True, which='h'))


# ================================================================================================ refinement stage
def _refine_in(B, T0, L, bwd=False, acc=0, masked=True):
    def make():
        g = gen(20, B, T0, L)
        S = sum(T0 >> l for l in range(L))
        specs = [('logits1', rn(g, B, S), 'in'), ('W_in', rn(g, 32, L, scale=0.5), 'in')]
        if masked:
            specs.append(('mask0', row_mask(g, B, T0), 'in'))
        if not bwd:
            specs += [('b_in', rn(g, 32), 'in'), ('H', out(B * T0, 32), 'out')]
            return specs, lambda c, v: c.lib.dcf_op_refine_in(p(v['logits1']), opt(v, 'mask0'), p(v['W_in']), p(v['b_in']), p(v['H']), B, T0, L, c.stream())
        specs += [('dH', rn(g, B * T0, 32), 'in'), ('dlogits1', out(B, S), 'out'), ('dW_in', rn(g, 32, L) if acc else out(32, L), 'inout' if acc else 'out'),
                  ('db_in', rn(g, 32) if acc else out(32), 'inout' if acc else 'out')]
        return specs, lambda c, v: c.lib.dcf_op_refine_in_bwd(p(v['logits1']), opt(v, 'mask0'), p(v['W_in']), p(v['dH']), p(v['dlogits1']), p(v['dW_in']),
                                                              p(v['db_in']), B, T0, L, acc, c.stream())
    return make


for B, T0, L, masked in [(2, 40, 4, 1), (3, 77, 1, 1), (1, 1, 1, 0), (2, 2, 2, 1), (2, 136, 3, 1), (1, 32768 // 128, 9, 0)]:
    case('dcf_op_refine_in', f'{B}x{T0}-L{L}-m{masked}', _refine_in(B, T0, L, masked=masked))
    case('dcf_op_refine_in_bwd', f'{B}x{T0}-L{L}-m{masked}-acc{B % 2}', _refine_in(B, T0, L, bwd=True, acc=B % 2, masked=masked))


def _tcn_layer(B, T0, dil, pdrop, bwd=False, acc=0, masked=True):
    def make():
        g = gen(21, B, T0, dil)
        specs = [('X', rn(g, B * T0, 32), 'in'), ('Wd', rn(g, 32, 32, 3, scale=0.15), 'in'), ('bd', rn(g, 32, scale=0.2), 'in'),
                 ('Wp', rn(g, 32, 32, scale=0.2), 'in'), ('bp', rn(g, 32, scale=0.2), 'in'), ('ln_w', torch.rand(32, generator=g) + 0.5, 'in'),
                 ('ln_b', rn(g, 32, scale=0.3), 'in')]
        if masked:
            specs.append(('mask', row_mask(g, B, T0), 'in'))
        seed, layer, b0 = 0x1234567890, 2, 3
        if not bwd:
            specs.append(('Y', out(B * T0, 32), 'out'))
            return specs, lambda c, v: c.lib.dcf_op_tcn_layer(p(v['X']), opt(v, 'mask'), p(v['Wd']), p(v['bd']), p(v['Wp']), p(v['bp']), p(v['ln_w']), p(v['ln_b']),
                                                              p(v['Y']), B, T0, dil, seed, pdrop, layer, b0, c.stream())
        specs.append(('dY', rn(g, B * T0, 32), 'in'))
        outs = [('dX', (B * T0, 32)), ('dWd', (32, 32, 3)), ('dbd', (32,)), ('dWp', (32, 32)), ('dbp', (32,)), ('dln_w', (32,)), ('dln_b', (32,))]
        for n, shape in outs:
            specs.append((n, rn(g, *shape) if acc and n != 'dX' else out(*shape), 'inout' if acc and n != 'dX' else 'out'))
        return specs, lambda c, v: c.lib.dcf_op_tcn_layer_bwd(p(v['X']), opt(v, 'mask'), p(v['Wd']), p(v['bd']), p(v['Wp']), p(v['bp']), p(v['ln_w']),
                                                              p(v['ln_b']), p(v['dY']), *[p(v[n]) for n, _ in outs], B, T0, dil, seed, pdrop, layer, b0, acc,
                                                              c.stream())
    return make


# dilation 1 / 4 / larger than the sequence, with and without dropout (two kernels), one to three rows
for B, T0, dil, pd, masked in [(2, 39, 1, 0.0, 1), (3, 77, 4, 0.25, 1), (1, 1, 1, 0.0, 0), (2, 3, 8, 0.5, 1), (2, 130, 64, 0.0, 1), (2, 300, 2, 0.1, 0)]:
    case('dcf_op_tcn_layer', f'{B}x{T0}-d{dil}-p{pd}-m{masked}', _tcn_layer(B, T0, dil, pd, masked=masked))
    case('dcf_op_tcn_layer_bwd', f'{B}x{T0}-d{dil}-p{pd}-m{masked}-acc{B % 2}', _tcn_layer(B, T0, dil, pd, bwd=True, acc=B % 2, masked=masked))


# ================================================================================================ scoring
def _sidekick(D, T, nq, norm):
    def make():
        g = gen(22, D, T, nq)
        specs = [('shallow', rn(g, D, T), 'in', T * 4), ('cls', rn(g, nq, D), 'in'), ('correl', out(nq, T), 'out')]
        return specs, lambda c, v: c.lib.dcf_op_sidekick(p(v['shallow']), p(v['cls']), p(v['correl']), D, T, nq, norm, c.stream())
    return make


for D, T, nq, norm in [(64, 77, 3, 1), (32, 1, 1, 0), (36, 3, 2, 1), (256, 250, 8, 1), (64, 130, 11, 0)]:          # T % 4 != 0
    case('dcf_op_sidekick', f'D{D}-T{T}-q{nq}-norm{norm}', _sidekick(D, T, nq, norm))


def _gate(T, vl, nq, sn, sratio, msf):
    def make():
        g = gen(23, T, nq, sn)
        specs = [('correl', rn(g, nq, T), 'in'), ('vid_mask', (torch.arange(T) < vl).to(torch.uint8), 'in'), ('gate', out(nq, T), 'out'),
                 ('mo', out(nq, T, dtype=torch.uint8), 'out')]
        return specs, lambda c, v: c.lib.dcf_op_gate(p(v['correl']), p(v['vid_mask']), p(v['gate']), p(v['mo']), T, nq, sn, sratio, msf, c.stream())
    return make


for T, vl, nq, sn, sr, msf in [(77, 60, 2, 8, 0.3, 1), (77, 77, 3, 8, 0.3, 0), (1, 1, 1, 4, 0.5, 1), (3, 2, 2, 2, 0.5, 0), (250, 201, 2, 60, 0.3, 1),
                               (130, 130, 1, 1, 0.1, 0)]:
    case('dcf_op_gate', f'T{T}-v{vl}-q{nq}-sn{sn}-msf{msf}', _gate(T, vl, nq, sn, sr, msf))


# ================================================================================================ composite blocks on a scratch model
def enc_shapes(E):
    sh = {'ln_attn.weight': (E, 1), 'ln_attn.bias': (E, 1), 'ln_ffn.weight': (E, 1), 'ln_ffn.bias': (E, 1),
          'drop_path_attn.scale': (1, E, 1), 'drop_path_ffn.scale': (1, E, 1),
          'ffn.fc.weight': (4 * E, E, 1), 'ffn.fc.bias': (4 * E,), 'ffn.proj.weight': (E, 4 * E, 1), 'ffn.proj.bias': (E,)}
    for n in 'qkv':
        sh[f'attn.{n}_conv.conv.weight'] = (E, 1, 3)
        sh[f'attn.{n}_norm.weight'] = (E, 1)
        sh[f'attn.{n}_norm.bias'] = (E, 1)
    for n in ('query', 'key', 'value', 'proj'):
        sh[f'attn.attn.{n}.weight'] = (E, E, 1)
        sh[f'attn.attn.{n}.bias'] = (E,)
    return sh


def dec_shapes(E, TE):
    return {'ln_xattn_q.weight': (E, 1), 'ln_xattn_q.bias': (E, 1), 'ln_xattn_kv.weight': (TE, 1), 'ln_xattn_kv.bias': (TE, 1),
            'xattn.q_conv.conv.weight': (E, 1, 3), 'xattn.q_norm.weight': (E, 1), 'xattn.q_norm.bias': (E, 1),
            'xattn.xattn.query.weight': (E, E, 1), 'xattn.xattn.query.bias': (E,), 'xattn.xattn.key.weight': (E, TE, 1),
            'xattn.xattn.key.bias': (E,), 'xattn.xattn.value.weight': (E, TE, 1), 'xattn.xattn.value.bias': (E,),
            'xattn.xattn.proj.weight': (2 * E, E, 1), 'xattn.xattn.proj.bias': (2 * E,), 'ln_ffn.weight': (E, 1), 'ln_ffn.bias': (E, 1),
            'ffn.fc.weight': (4 * E, E, 1), 'ffn.fc.bias': (4 * E,), 'ffn.proj.weight': (E, 4 * E, 1), 'ffn.proj.bias': (E,),
            'drop_path_ffn.scale': (1, E, 1)}


def scratch_model(ctx, weights, prefix, **cfg):
    """dcf_model_create + dcf_model_bind of one block's parameters (never finalized), as tests/test_gpu_ops.py builds it; the bound
    weights stay outside the arena and alive in ``keep``"""
    L = ctx.pkg._lib
    c = L.DcfConfig()
    base = dict(D=32, E=32, TE=32, vid_heads=4, fusion_heads=4, fusion_layers=0, n_embd_convs=0, n_stem=0, n_levels=1, win=9,
                head_layers=0, sn=60, sratio=0.3, msf=1, norm=1, max_batch=8)
    base.update(cfg)
    for k, val in base.items():
        setattr(c, k, val)
    h = ctypes.c_void_p()
    L.check(ctx.lib.dcf_model_create(ctypes.byref(c), ctypes.byref(h)), 'dcf_model_create')
    keep = []
    for k, val in weights.items():
        t = val.contiguous().cuda()
        keep.append(t)
        shape = (ctypes.c_int64 * max(t.dim(), 1))(*(t.shape if t.dim() else (1,)))
        L.check(ctx.lib.dcf_model_bind(h, f'{prefix}.{k}'.encode(), p(t), shape, max(t.dim(), 1)), 'dcf_model_bind')
    return h, keep


def _enc_model(ctx, E, win):
    def factory():
        sd = ctx.pkg.synth.make_state_dict(enc_shapes(E), 5000 + E)
        return scratch_model(ctx, sd, 'e', E=E, win=win, vid_heads=4, gemm_mode=16)
    return ctx.model(('enc', E, win), factory)


def _encoder(B, T, E, stride, win=9, pre=False):
    def make():
        g = gen(24, B, T, E, stride)
        To = T // stride
        specs = [('X', rn(g, B * T, E, scale=1.5, shift=0.3), 'in'), ('mask', row_mask(g, B, T), 'in')]
        if pre:
            specs += [(n, out(B * To, E), 'out') for n in ('Qc', 'Kc', 'Vc')] + ([('Skip', out(B * To, E), 'out')] if stride == 2 else [])
            return specs, lambda c, v: c.lib.dcf_op_enc_pre(_enc_model(c, E, win), b'e', p(v['X']), p(v['mask']), B, T, stride, p(v['Qc']), p(v['Kc']), p(v['Vc']),
                                                            opt(v, 'Skip'), c.stream())
        specs += [('Y', out(B * To, E), 'out'), ('mo', out(B * To, dtype=torch.uint8), 'out')]
        return specs, lambda c, v: c.lib.dcf_op_encoder(_enc_model(c, E, win), b'e', p(v['X']), p(v['mask']), B, T, stride, p(v['Y']), p(v['mo']), c.stream())
    return make


# E = 256 with the one-kernel halves (enc_chain_min_rows / enc_attn_min_rows 0) and as separate launches (1 << 30); E = 32 has no
# chain kernel; T / stride is a multiple of win // 2 (blocks.py:216); a 128-row window with a partial tail
BIG = 1 << 30
for tag, rows in (('chain', 0), ('launches', BIG)):
    opts = (('enc_chain_min_rows', rows), ('enc_attn_min_rows', rows))
    for B, T, stride in [(2, 76, 1), (2, 136, 2), (1, 4, 1), (1, 8, 2), (3, 132, 1)]:
        case('dcf_op_encoder', f'{B}x{T}-256-s{stride}-{tag}', _encoder(B, T, 256, stride), opts)
    for B, T, stride in [(2, 76, 1), (2, 136, 2), (1, 4, 1)]:
        case('dcf_op_enc_pre', f'{B}x{T}-256-s{stride}-{tag}', _encoder(B, T, 256, stride, pre=True), opts)
case('dcf_op_encoder', '2x76-32-s1', _encoder(2, 76, 32, 1))
case('dcf_op_encoder', '2x40-32-s2-w5', _encoder(2, 40, 32, 2, win=5))
case('dcf_op_encoder', '2x90-64-s1-w19', _encoder(2, 90, 64, 1, win=19))
case('dcf_op_enc_pre', '2x39-32-s1', _encoder(2, 39, 32, 1, pre=True))
case('dcf_op_enc_pre', '2x38-64-s2', _encoder(2, 38, 64, 2, pre=True))
case('dcf_op_enc_pre', '1x1-32-s1', _encoder(1, 1, 32, 1, pre=True))


def _decoder(B, T, E, TE, lens, affine):
    def make():
        g = gen(25, B, T, E, TE)
        Lk = max(lens)
        specs = [('X', rn(g, B * T, E, scale=1.5, shift=0.3), 'inout'), ('mask', row_mask(g, B, T), 'in')]
        for b in range(B):
            tm = torch.ones(lens[b], dtype=torch.uint8)
            if b == B - 1 and lens[b] > 2:
                tm[lens[b] * 2 // 3:] = 0
            specs += [(f'text{b}', rn(g, TE, lens[b]), 'in', lens[b] * 4), (f'tmask{b}', tm, 'in')]

        def call(c, v):
            def factory():
                sd = c.pkg.synth.make_state_dict(dec_shapes(E, TE), 4000 + E + TE)
                return scratch_model(c, sd, 'd', E=E, TE=TE, fusion_heads=4, gemm_mode=16, xattn_affine=int(affine))
            h = c.model(('dec', E, TE, affine), factory)
            tp = (ctypes.c_void_p * B)(*[v[f'text{b}'].data_ptr() for b in range(B)])
            mp = (ctypes.c_void_p * B)(*[v[f'tmask{b}'].data_ptr() for b in range(B)])
            ln = (ctypes.c_int32 * B)(*lens)
            return c.lib.dcf_op_decoder(h, b'd', p(v['X']), p(v['mask']), B, T, tp, mp, ln, c.stream())
        assert Lk <= 64
        return specs, call
    return make


# E = 256 with the attention half as one kernel (dec_chain_min_rows 0) and as separate launches; queries of different token counts
# (odd: the channel-major text rows are not 16-byte multiples); E = 64 has no chain kernel
for tag, rows in (('chain', 0), ('launches', BIG)):
    opts = (('dec_chain_min_rows', rows),)
    case('dcf_op_decoder', f'2x77-256-k33-{tag}', _decoder(2, 77, 256, 256, [33, 17], 0), opts)
    case('dcf_op_decoder', f'3x130-256-k5-affine-{tag}', _decoder(3, 130, 256, 64, [5, 3, 1], 1), opts)
    case('dcf_op_decoder', f'1x3-256-k7-{tag}', _decoder(1, 3, 256, 256, [7], 0), opts)
case('dcf_op_decoder', '2x39-64-k9', _decoder(2, 39, 64, 32, [9, 6], 0))


def _tcn(B, T):
    def make():
        ops = Golden('ops.npz')
        w = ops.sub('tcn/w/')
        n_in = ops.t('tcn/x').shape[1]
        g = gen(26, B, T)
        specs = [('x', rn(g, B * T, n_in), 'in'), ('mask', (torch.rand(B * T, generator=g) > 0.15).to(torch.uint8), 'in'), ('Y', out(B * T, 32), 'out')]
        return specs, lambda c, v: c.lib.dcf_op_tcn(c.model(('tcn',), lambda: scratch_model(c, w, 'r')), b'r', p(v['x']), p(v['mask']), B, T, n_in, 4, p(v['Y']),
                                                    c.stream())
    return make


# the four layers of the reference fixture's weights: the stacked launch over LDS windows (tcn_stack 3 / 2) and layer by layer (0), the
# weight fragments from the per-model image (tcn_frag 1) and built by every workgroup (0)
for tag, opts in (('default', ()), ('stack0', (('tcn_stack', 0),)), ('stack2', (('tcn_stack', 2),)), ('stack3', (('tcn_stack', 3),)), ('frag0', (('tcn_frag', 0),)),
                  ('frag1', (('tcn_frag', 1),))):
    for B, T in [(2, 77), (1, 3), (3, 1000)]:
        case('dcf_op_tcn', f'{B}x{T}-{tag}', _tcn(B, T), opts)


# ================================================================================================ losses and the objective
def _focal(n, alpha, gamma, smoothing, sel, outs, grad=None):
    def make():
        g = gen(27, n, smoothing)
        specs = [('x', rn(g, n, scale=2.0), 'in'), ('t', (torch.rand(n, generator=g) > 0.7).float(), 'in')]
        if sel:
            specs.append(('sel', (torch.rand(n, generator=g) > 0.4).to(torch.uint8), 'in'))
        if grad is None:
            if 'e' in outs:
                specs.append(('elem', out(n), 'out'))
            if 's' in outs:
                specs += [('sum', out(1), 'out'), ('count', out(1, dtype=torch.int32), 'out')]
            return specs, lambda c, v: c.lib.dcf_sigmoid_focal_loss(p(v['x']), p(v['t']), opt(v, 'sel'), n, alpha, gamma, smoothing, opt(v, 'elem'), opt(v, 'sum'),
                                                                    opt(v, 'count'), c.stream())
        if grad == 'elem':
            specs.append(('g_elem', rn(g, n), 'in'))
        else:
            specs += [('g_scalar', torch.tensor([0.7]), 'in'), ('count', torch.tensor([max(n // 2, 1)], dtype=torch.int32), 'in')]
        specs.append(('g', out(n), 'out'))
        return specs, lambda c, v: c.lib.dcf_sigmoid_focal_loss_grad(p(v['x']), p(v['t']), opt(v, 'sel'), n, alpha, gamma, smoothing, opt(v, 'g_elem'),
                                                                     opt(v, 'g_scalar'), opt(v, 'count'), p(v['g']), c.stream())
    return make


def _iou(n, kind, sel, outs, grad=None):
    def make():
        g = gen(28, n, kind)
        specs = [('a', torch.rand(n, 2, generator=g) * 6, 'in'), ('b', torch.rand(n, 2, generator=g) * 6, 'in')]
        if sel:
            specs.append(('sel', (torch.rand(n, generator=g) > 0.4).to(torch.uint8), 'in'))
        if grad is None:
            if 'e' in outs:
                specs.append(('elem', out(n), 'out'))
            if 's' in outs:
                specs += [('sum', out(1), 'out'), ('count', out(1, dtype=torch.int32), 'out')]
            return specs, lambda c, v: c.lib.dcf_ctr_iou_loss(p(v['a']), p(v['b']), opt(v, 'sel'), n, kind, 1e-8, opt(v, 'elem'), opt(v, 'sum'), opt(v, 'count'),
                                                              c.stream())
        if grad == 'elem':
            specs.append(('g_elem', rn(g, n), 'in'))
        else:
            specs += [('g_scalar', torch.tensor([0.7]), 'in'), ('count', torch.tensor([max(n // 2, 1)], dtype=torch.int32), 'in')]
        specs.append(('g', out(n, 2), 'out'))
        return specs, lambda c, v: c.lib.dcf_ctr_iou_loss_grad(p(v['a']), p(v['b']), opt(v, 'sel'), n, kind, 1e-8, opt(v, 'g_elem'), opt(v, 'g_scalar'),
                                                               opt(v, 'count'), p(v['g']), c.stream())
    return make


for n, sel, outs in [(77, 1, 'es'), (1, 0, 'e'), (3, 1, 's'), (5003, 1, 'es'), (2049, 0, 's')]:           # several workgroups, a ragged last one
    case('dcf_sigmoid_focal_loss', f'n{n}-sel{sel}-{outs}', _focal(n, 0.5, 2.0, n % 2, sel, outs))
    case('dcf_ctr_iou_loss', f'n{n}-sel{sel}-{outs}-kind{n % 2}', _iou(n, n % 2, sel, outs))
    case('dcf_sigmoid_focal_loss_grad', f'n{n}-sel{sel}-{"elem" if "e" in outs else "scalar"}', _focal(n, 0.5, 2.0, n % 2, sel, outs, grad='elem' if 'e' in outs else 'scalar'))
    case('dcf_ctr_iou_loss_grad', f'n{n}-sel{sel}-{"elem" if "e" in outs else "scalar"}-kind{n % 2}', _iou(n, n % 2, sel, outs, grad='elem' if 'e' in outs else 'scalar'))
case('dcf_sigmoid_focal_loss', 'n77-alpha-off-gamma1.5', _focal(77, -1.0, 1.5, 0, 1, 'es'))


def _objective(kind, nrows, T, L, valid, use_offset, cs, iou_kind, heads2=True, acc=0, values=False, extra=True):
    def make():
        g = gen(29, nrows, T, L)
        S = sum(T >> l for l in range(L))
        c0 = torch.rand(nrows, generator=g) * T * 0.8
        targets = torch.stack((c0, c0 + torch.rand(nrows, generator=g) * T * 0.3 + 0.5), -1).contiguous()
        rule = (T, L, 4.0, 0.5, use_offset, T, cs, 1.5)
        if kind == 'annotate':
            specs = [('targets', targets, 'in'), ('labels', out(nrows, S, dtype=torch.uint8), 'out'), ('offsets', out(nrows, S, 2), 'out')]
            if extra:
                specs += [('win', out(nrows, S, dtype=torch.uint8), 'out'), ('rng', out(nrows, S, dtype=torch.uint8), 'out')]
            return specs, lambda c, v: c.lib.dcf_annotate_points(p(v['targets']), nrows, *rule, p(v['labels']), p(v['offsets']), opt(v, 'win'), opt(v, 'rng'),
                                                                 c.stream())
        masks = torch.zeros(nrows, S, dtype=torch.uint8)
        for b in range(nrows):
            m = torch.arange(T) < valid[b % len(valid)]
            masks[b] = torch.cat([m[::2 ** l] for l in range(L)])
        specs = [('logits2', rn(g, nrows, S, scale=2.0, shift=-2.0), 'in'), ('offsets', torch.rand(nrows, S, 2, generator=g) * 6, 'in'), ('masks', masks, 'in'),
                 ('targets', targets, 'in'), ('loss_norm', torch.tensor([37.5]), 'in')]
        if heads2:
            specs.append(('logits1', rn(g, nrows, S, scale=2.0, shift=-2.0), 'in'))
        common = lambda v: (opt(v, 'logits1'), p(v['logits2']), p(v['offsets']), p(v['masks']), p(v['targets']), nrows, *rule, 0.5, 0.2, iou_kind, 1e-8,
                            p(v['loss_norm']), 2.0, 0.25)
        if kind == 'objective':
            specs += [('rows', out(nrows, 4), 'out'), ('out4', out(4), 'out')]
            return specs, lambda c, v: c.lib.dcf_point_objective(*common(v), p(v['rows']), p(v['out4']), c.stream())
        io = 'inout' if acc else 'out'
        mk = (lambda *s: rn(g, *s)) if acc else out
        specs += [('g2', mk(nrows, S), io), ('go', mk(nrows, S, 2), io)]
        if heads2:
            specs.append(('g1', mk(nrows, S), io))
        if extra:
            specs += [('grad_total', torch.tensor([0.5]), 'in'), ('grad_parts', torch.tensor([0.25, -1.5]), 'in')]
        if values:
            specs += [('rows', out(nrows, 4), 'out'), ('out4', out(4), 'out')]
        return specs, lambda c, v: c.lib.dcf_point_objective_grad(*common(v), opt(v, 'grad_total'), opt(v, 'grad_parts'), opt(v, 'g1'), p(v['g2']), p(v['go']), acc,
                                                                  opt(v, 'rows'), opt(v, 'out4'), c.stream())
    return make


# S = sum of T >> l is odd for L >= 2 with T = 2^(L-1) * odd: rows of the packed outputs start at odd offsets
for nrows, T, L, valid, uo, cs, ik in [(3, 40, 4, [40, 31], 0, 1, 1), (1, 1, 1, [1], 1, 0, 0), (2, 2, 2, [2, 1], 0, 1, 0), (5, 328, 4, [328, 201, 77], 1, 1, 1),
                                       (2, 1536, 10, [1536, 1000], 0, 0, 0)]:
    case('dcf_annotate_points', f'{nrows}x{T}-L{L}-uo{uo}-cs{cs}', _objective('annotate', nrows, T, L, valid, uo, cs, ik))
    case('dcf_point_objective', f'{nrows}x{T}-L{L}-uo{uo}-cs{cs}-iou{ik}', _objective('objective', nrows, T, L, valid, uo, cs, ik))
    case('dcf_point_objective_grad', f'{nrows}x{T}-L{L}-uo{uo}-cs{cs}-iou{ik}-acc{nrows % 2}', _objective('grad', nrows, T, L, valid, uo, cs, ik, acc=nrows % 2,
                                                                                                       values=bool(T % 3)))
case('dcf_annotate_points', '3x40-L4-labels-only', _objective('annotate', 3, 40, 4, [40, 31], 0, 1, 1, extra=False))
case('dcf_point_objective', '3x40-L4-one-head', _objective('objective', 3, 40, 4, [40, 31], 0, 1, 1, heads2=False))
case('dcf_point_objective_grad', '3x40-L4-one-head-defaults', _objective('grad', 3, 40, 4, [40, 31], 0, 1, 1, heads2=False, extra=False))


# ================================================================================================ post-processing
def _collect(nq, T, L, topk, ext, shift=-1.0):
    def make():
        g = gen(30, nq, T, L, topk)
        S = sum(T >> l for l in range(L))
        masks = torch.ones(nq, S, dtype=torch.uint8)
        masks[-1, int(S * 0.9):] = 0
        specs = [('logits', rn(g, nq, S, scale=2.0, shift=shift), 'in'), ('offsets', torch.rand(nq, S, 2, generator=g) * 5, 'in'), ('masks', masks, 'in'),
                 ('segs', out(nq, topk, 2), 'out'), ('scores', out(nq, topk), 'out'), ('counts', out(nq, dtype=torch.int32), 'out')]
        if ext:
            e = torch.rand(nq, T, generator=g)
            e[:, ::3] = 0
            specs.append(('ext', e, 'in'))
            return specs, lambda c, v: c.lib.dcf_collect_segments_ext(p(v['logits']), p(v['offsets']), p(v['masks']), p(v['ext']), nq, T, L, 0.001, topk, 0.0,
                                                                      p(v['segs']), p(v['scores']), p(v['counts']), c.stream())
        return specs, lambda c, v: c.lib.dcf_collect_segments(p(v['logits']), p(v['offsets']), p(v['masks']), nq, T, L, 0.001, topk, 0.0, p(v['segs']),
                                                              p(v['scores']), p(v['counts']), c.stream())
    return make


# fewer points than threads, fewer candidates than top-k, the bitonic network (top-k 4000) with the keys re-read from global scratch
# (49152 points), the radix sort with the keys in registers
for nq, T, L, topk, shift in [(2, 40, 4, 50, -1.0), (1, 1, 1, 8, 2.0), (3, 328, 4, 2000, -1.0), (1, 32768, 2, 4000, -2.0), (2, 4096, 8, 300, -9.0)]:
    for ext in (0, 1):
        case('dcf_collect_segments_ext' if ext else 'dcf_collect_segments', f'{nq}x{T}-L{L}-k{topk}', _collect(nq, T, L, topk, ext, shift))


def _segs(g, nq, n):
    c0 = torch.rand(nq, n, generator=g) * (20 + 3 * n ** 0.5)
    ln = torch.rand(nq, n, generator=g) * 30 + 0.1
    return torch.stack((c0 - ln / 2, c0 + ln / 2), -1).contiguous(), torch.rand(nq, n, generator=g).sort(1, descending=True)[0].contiguous()


def _nms(nq, n_max, stride, counts, soft=None, max_iters=0):
    def make():
        g = gen(31, nq, n_max, stride)
        segs, scores = _segs(g, nq, stride)
        specs = [('segs', segs, 'in'), ('scores', scores, 'in')]
        if counts is not None:
            specs.append(('counts', torch.tensor(counts, dtype=torch.int32), 'in'))
        if soft is None:
            specs += [('keep', out(nq, stride, dtype=torch.int64), 'out'), ('kc', out(nq, dtype=torch.int32), 'out')]
            return specs, lambda c, v: c.lib.dcf_nms_1d(p(v['segs']), p(v['scores']), opt(v, 'counts'), nq, n_max, stride, 0.5, p(v['keep']), p(v['kc']), c.stream())
        specs += [('dets', out(nq, stride, 3), 'out'), ('inds', out(nq, stride, dtype=torch.int64), 'out'), ('oc', out(nq, dtype=torch.int32), 'out')]
        return specs, lambda c, v: c.lib.dcf_softnms_1d(p(v['segs']), p(v['scores']), opt(v, 'counts'), nq, n_max, stride, 0.5, 0.5, 0.05, soft, max_iters,
                                                        p(v['dets']), p(v['inds']), p(v['oc']), c.stream())
    return make


# below and above the 4096 candidates one workgroup's LDS holds (beyond: the same kernels over a global scratch block)
# (the kernels run 256 / 512 / 1024 threads up to 768 / 3072 / 4096 candidates)
for nq, n_max, stride, counts in [(3, 77, 80, [77, 3, 0]), (1, 1, 1, None), (2, 130, 130, None), (1, 801, 801, None), (1, 3100, 3101, None),
                                  (1, 4099, 4100, [4099])]:
    case('dcf_nms_1d', f'{nq}x{n_max}-ld{stride}', _nms(nq, n_max, stride, counts))
    for method in ((0, 1, 2) if n_max < 800 else (2,)):
        case('dcf_softnms_1d', f'{nq}x{n_max}-ld{stride}-m{method}', _nms(nq, n_max, stride, counts, soft=method, max_iters=0 if n_max < 800 else 40))
case('dcf_softnms_1d', '3x77-ld80-m1-k5', _nms(3, 77, 80, [77, 3, 0], soft=1, max_iters=5))


def _voting(nq, n1, n1_stride, ld, n2, n2_stride, counted):
    def make():
        g = gen(32, nq, n1, n2)
        all_segs, all_scores = _segs(g, nq, n2_stride)
        nms = torch.zeros(nq, n1_stride, ld)
        nms[:, :, :2] = all_segs[:, :n1_stride] + 0.25 if n1_stride <= n2_stride else _segs(g, nq, n1_stride)[0]
        if ld == 3:
            nms[:, :, 2] = all_scores[:, :n1_stride]
        specs = [('nms', nms, 'in'), ('all_segs', all_segs, 'in'), ('all_scores', all_scores, 'in'), ('out', out(nq, n1_stride, 2), 'out')]
        if counted:
            specs += [('c1', torch.tensor([max(n1 - 3 * q, 0) for q in range(nq)], dtype=torch.int32), 'in'),
                      ('c2', torch.tensor([max(n2 - 7 * q, 1) for q in range(nq)], dtype=torch.int32), 'in')]
        return specs, lambda c, v: c.lib.dcf_segment_voting(p(v['nms']), ld, opt(v, 'c1'), n1, n1_stride, p(v['all_segs']), p(v['all_scores']), opt(v, 'c2'), n2,
                                                            n2_stride, 0.75, nq, p(v['out']), c.stream())
    return make


for nq, n1, n1s, ld, n2, n2s, counted in [(3, 5, 7, 3, 77, 80, 1), (1, 1, 1, 2, 1, 1, 0), (2, 50, 50, 2, 2001, 2001, 0), (2, 9, 9, 3, 4099, 4100, 1)]:
    case('dcf_segment_voting', f'{nq}x{n1}-ld{ld}-of-{n2}', _voting(nq, n1, n1s, ld, n2, n2s, counted))


# ================================================================================================ the training update
CHUNK = 4096
_ROW = np.dtype([('p', '<u8'), ('g', '<u8'), ('exp_avg', '<u8'), ('exp_avg_sq', '<u8'), ('ema', '<u8'), ('n', '<i8'), ('group', '<i4'), ('flags', '<i4'),
                 ('chunk0', '<i8')])


def _optim(kind, sizes, misaligned=(), no_grad=(), no_ema=(), mode=0, with_ema=1, use_coef=True):
    """parameter, gradient, both moments and the EMA copy of every tensor are arena operands, the row table (n x 8 int64 = the 64-byte
    dcf_optim_row records) and the chunk map too; ``misaligned`` tensors start one element into their operand (4-byte aligned only)"""
    def make():
        g = gen(33, len(sizes), sum(sizes))
        n_t = len(sizes)
        specs = []
        roles = {'norm': dict(p='in', g='in', m='in', v='in', e='in'), 'scale': dict(p='in', g='inout', m='in', v='in', e='in'),
                 'adam': dict(p='inout', g='in', m='inout', v='inout', e='inout')}[kind]
        for i, n in enumerate(sizes):
            pad = 1 if i in misaligned else 0
            for col, scale in (('p', 1.0), ('g', 0.1), ('m', 0.01), ('v', None), ('e', 1.0)):
                t = torch.rand(n + pad, generator=g) * 1e-3 if scale is None else rn(g, n + pad, scale=scale)
                specs.append((f'{col}{i}', t, roles[col]))
        counts = [-(-n // CHUNK) for n in sizes]
        cmap = np.repeat(np.arange(n_t, dtype=np.int32), counts)
        specs += [('table', torch.zeros(n_t, 8, dtype=torch.int64), 'in'), ('cmap', torch.from_numpy(cmap.copy()), 'in')]
        if kind == 'norm':
            specs += [('norm', out(1), 'out'), ('coef', out(1), 'out')]
        else:
            specs.append(('coef', torch.tensor([0.37]), 'in'))

        def fixup(v, update):
            rec = np.zeros(n_t, dtype=_ROW)
            for i, n in enumerate(sizes):
                off = 4 if i in misaligned else 0
                for col, f in (('p', 'p'), ('g', 'g'), ('m', 'exp_avg'), ('v', 'exp_avg_sq'), ('e', 'ema')):
                    rec[f][i] = v[f'{col}{i}'].data_ptr() + off
                if i in no_ema:
                    rec['ema'][i] = 0
                rec['n'][i], rec['group'][i], rec['flags'][i] = n, i % 2, int(i in no_grad)
            rec['chunk0'] = np.cumsum(counts) - np.array(counts)
            update('table', torch.from_numpy(rec.view(np.int64).reshape(n_t, 8).copy()))

        def call(c, v):
            args = (p(v['table']), p(v['cmap']), n_t, len(cmap))
            if kind == 'norm':
                return c.lib.dcf_optim_grad_norm(*args, 1.0, p(v['norm']), p(v['coef']), c.stream())
            if kind == 'scale':
                return c.lib.dcf_optim_scale(*args, p(v['coef']), c.stream())
            groups = (c.pkg._lib.DcfOptimGroup * 2)()
            for k, wd in enumerate((0.05, 0.0)):
                h = groups[k]
                h.lr, h.weight_decay, h.b1, h.b2, h.eps = 1e-3, wd, 0.9, 0.999, 1e-8
                h.one_minus_b1, h.one_minus_b2 = 1.0 - 0.9, 1.0 - 0.999
                h.bc1, h.sqrt_bc2 = 1.0 - 0.9 ** 3, math.sqrt(1.0 - 0.999 ** 3)
                h.mode = mode
            return c.lib.dcf_optim_adam_step(*args, ctypes.cast(groups, ctypes.c_void_p), 2, p(v['coef']) if use_coef else None, with_ema, 0.999, c.stream())
        return specs, call, fixup
    return make


# one element, sizes around a 16-byte group and around a chunk, an empty tensor, a tensor without a gradient, one without an EMA copy,
# one that is only 4-byte aligned (the element-at-a-time path); both modes
_SIZES = [1, 3, 5, 257, 0, CHUNK - 1, CHUNK + 1, 2 * CHUNK + 7, 77]
for kind, export in (('norm', 'dcf_optim_grad_norm'), ('scale', 'dcf_optim_scale'), ('adam', 'dcf_optim_adam_step')):
    case(export, 'nine-tensors', _optim(kind, _SIZES, misaligned=(3, 7), no_grad=(2,), no_ema=(5,)))
    case(export, 'one-element', _optim(kind, [1]))
case('dcf_optim_adam_step', 'adam-mode-no-ema-no-coef', _optim('adam', [5, CHUNK + 3, 130], misaligned=(1,), mode=1, with_ema=0, use_coef=False))


# ================================================================================================ dropout
def _keep(e0, n, pdrop):
    def make():
        specs = [('out', out(n, dtype=torch.uint8), 'out')]
        return specs, lambda c, v: c.lib.dcf_debug_dropout_keep(0x1234567890, (4 << 16) | (2 << 4) | 5, e0, n, pdrop, p(v['out']), c.stream())
    return make


for e0, n, pd in [(0, 1, 0.5), (5, 3, 0.25), (3, 1003, 0.1), (4096, 4099, 0.9)]:      # e0 % 4 != 0: the first Philox block is partial
    case('dcf_debug_dropout_keep', f'e{e0}-n{n}-p{pd}', _keep(e0, n, pd))


# ================================================================================================ what the table does not hold
EXCLUDED = {
    # no caller-owned device extent
    'dcf_last_error': 'returns a host string',
    'dcf_abi_version': 'returns a number',
    'dcf_model_create': 'host structures only',
    'dcf_model_destroy': 'host structures only',
    'dcf_model_bind': 'borrows a parameter; nothing is read or written until a forward',
    'dcf_model_set_pe': 'borrows a buffer; nothing is read or written until a forward',
    'dcf_model_set_text_pe': 'borrows a buffer; nothing is read or written until a forward',
    'dcf_model_set_dropout': 'host state of the model',
    'dcf_model_set_graph_mode': 'host state of the model',
    'dcf_model_set_ln_carry': 'host state of the model',
    'dcf_model_finalize': "repacks bound parameters into the model's own memory",
    'dcf_numerics_status': "reads the model's own status word",
    'dcf_numerics_status_async': "copies the model's own status word to pinned host memory",
    'dcf_points_per_query': 'host arithmetic',
    'dcf_graph_active': 'host state of the model',
    'dcf_debug_set_option': 'process-wide host switch',
    'dcf_debug_copy': "copies from the model's own workspace into a buffer of caller-stated size (a test tap)",
    'dcf_profile_enable': 'host switch',
    'dcf_profile_report': 'writes a host buffer',
    'dcf_calib_mfma_rate': 'register-only kernels, host outputs',
    # the forward and hybrid entry points: their inputs are covered by test_engine_inputs_between_poisoned_borders, their outputs are
    # allocated inside modeling.py
    'dcf_text_encode': 'forward entry point: inputs covered by the engine test',
    'dcf_forward_eval': 'forward entry point: inputs covered by the engine test',
    'dcf_forward_eval_videos': 'forward entry point: inputs covered by the engine test',
    'dcf_forward_train_videos': 'forward entry point: same input path as dcf_forward_eval_videos',
    'dcf_forward_eval_gated': 'forward entry point: same input path as dcf_forward_eval',
    'dcf_hybrid_phase1': 'hybrid entry point: same input path as dcf_forward_eval_gated',
    'dcf_hybrid_phase2': 'hybrid entry point',
    'dcf_hybrid_phase3': 'hybrid entry point',
}
