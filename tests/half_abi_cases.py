"""One entry per export of the half-feature extension (include/decafnet_hip_half.h, ``_lib.HALF_SIGNATURES``) for
tests/test_gpu_half_borders.py, in the format of tests/abi_cases.py: ``Case(export, tag, make, options)`` with ``make()`` ->
``(specs, call)``.

A half operand is placed as the BYTES of its binary16 values -- a uint8 tensor of shape (rows, 2 * columns) with its own row pitch --
because tests/arena.py defines its fills per dtype and has none for float16: fill 1 (bytes 0xFF) reads as the half NaN 0xFFFF on
every side of the operand, fill 2 (bytes 0) as zeros.  The export gets the address of that view.

dcf_op_linear_cm_split_ld_h: windows of M clips of rows lda > M long, at the start and at the end of the rows (the last row's window
ends with the operand).  dcf_op_linear_cm_split_h: M = 4 (one quarter-filled row group of a 64-row tile), M = 68 (a second tile with four rows), M = 132,
N = 128 and 256 (the two tile widths), both operand splits, both scales.  dcf_op_sidekick_h: T % 4 == 0 (8-byte loads) and T % 4 != 0
(clip by clip; T = 1 .. 3 far below a wave), more than eight queries (two query chunks).  The two forwards: a finalized model of
E = 128 (three operand sets of the shallow / expert halves share a grid, the scores ride on the GEMM) and of E = 256 (the expert
halves of all videos in one grid), videos shorter than their padded length T = 192 = three 64-clip tiles of which the gate keeps one
per query, outputs inside the arena; once more with the scoring kernels (fuse_scores = 0) and on the upcast path (half_native = 0).
``text``, ``text_mask``, ``text_len`` and ``nq_per_video`` are host arrays, and the encoded text is the model's own: no operands of
the arena."""
import ctypes
import math

import torch

from abi_cases import Case, gen, opt, out, p, rn

CASES = []


def case(export, tag, make, options=()):
    CASES.append(Case(export, tag, make, tuple(options)))


def half_bytes(t):
    """(rows, cols) float -> the bytes of its binary16 rounding, (rows, 2 cols) uint8"""
    return t.half().contiguous().view(torch.uint8)


def _linear(M, N, K, nterms, unscaled, bias=True):
    def make():
        g = gen(71, M, N, K, nterms, unscaled)
        specs = [('A', half_bytes(rn(g, K, M)), 'in', M * 2), ('W', rn(g, N, K, scale=1 / math.sqrt(K)), 'in'), ('C', out(M, N), 'out')]
        if bias:
            specs.append(('b', rn(g, N), 'in'))
        return specs, lambda c, v: c.lib.dcf_op_linear_cm_split_h(p(v['A']), p(v['W']), opt(v, 'b'), p(v['C']), M, N, K, nterms, unscaled, c.stream())
    return make


def _linear_ld(M, lda, N, K, nterms, col0):
    """the window [col0, col0 + M) of every row of a (K, lda) half matrix: the columns beside it are finite values the product must not use"""
    def make():
        g = gen(74, M, lda, N, K, nterms)
        specs = [('A', half_bytes(rn(g, K, lda)), 'in', lda * 2), ('W', rn(g, N, K, scale=1 / math.sqrt(K)), 'in'), ('b', rn(g, N), 'in'), ('C', out(M, N), 'out')]

        def call(c, v):
            a = ctypes.c_void_p(v['A'].data_ptr() + 2 * col0)
            return c.lib.dcf_op_linear_cm_split_ld_h(a, lda, p(v['W']), p(v['b']), p(v['C']), M, N, K, nterms, 0, c.stream())
        return specs, call
    return make


for M, lda, N, K, nt, col0 in [(68, 200, 128, 64, 16, 132), (68, 200, 128, 64, 6, 0), (132, 136, 256, 96, 16, 4), (4, 1028, 128, 32, 6, 1024)]:
    case('dcf_op_linear_cm_split_ld_h', f'{M}of{lda}at{col0}x{N}x{K}-n{nt}', _linear_ld(M, lda, N, K, nt, col0))

for M, N, K, nt, un in [(4, 128, 32, 16, 0), (68, 128, 64, 6, 0), (132, 256, 96, 16, 1), (68, 256, 32, 6, 1), (1000, 256, 64, 16, 0)]:
    case('dcf_op_linear_cm_split_h', f'{M}x{N}x{K}-n{nt}-u{un}', _linear(M, N, K, nt, un, bias=M != 68))


def _sidekick(D, T, nq, norm):
    def make():
        g = gen(72, D, T, nq)
        specs = [('shallow', half_bytes(rn(g, D, T)), 'in', T * 2), ('cls', rn(g, nq, D), 'in'), ('correl', out(nq, T), 'out')]
        return specs, lambda c, v: c.lib.dcf_op_sidekick_h(p(v['shallow']), p(v['cls']), p(v['correl']), D, T, nq, norm, c.stream())
    return make


for D, T, nq, norm in [(64, 68, 4, 1), (64, 77, 3, 1), (32, 1, 1, 0), (36, 3, 2, 1), (256, 252, 8, 1), (64, 130, 11, 0), (64, 132, 9, 1)]:
    case('dcf_op_sidekick_h', f'D{D}-T{T}-q{nq}-norm{norm}', _sidekick(D, T, nq, norm))


# ================================================================================================ the forwards
KW = dict(D=64, TE=32, text_in=32, n_levels=4, win=5, n_heads=4, sn=64, sratio=0.4, msf=True, norm=True, max_seq_len=128, text_layers=1,
          text_max_len=24)
T_FWD, LEVELS = 192, 4
S_FWD = sum(T_FWD >> l for l in range(LEVELS))


def _model(c, E, nqs):
    """(model, encoded text per query, their masks): built once per (E, query counts), its engine bound by one ordinary forward"""
    def factory():
        pkg = c.pkg
        model = pkg.modeling.create_model(pkg.config.make_opt(**dict(KW, E=E)))
        model.load_state_dict(pkg.synth.make_state_dict({k: list(t.shape) for k, t in model.state_dict().items()}, 51))
        model = model.cuda().eval().requires_grad_(False)
        g = torch.Generator().manual_seed(52)
        texts, tmasks = [], []
        for q in range(sum(nqs)):
            tok = torch.randn(1, 32, 5 + q, generator=g).cuda()
            t, m = model.encode_text(tok, torch.ones(1, 1, tok.size(-1), dtype=torch.bool, device='cuda'))
            texts.append(t[0].contiguous().float())
            tmasks.append(m.reshape(-1).to(torch.bool).contiguous())
        inp = pkg.synth.make_inputs(64, T_FWD, T_FWD, 1, 32, 5, 53)
        model(inp['vid'].cuda(), inp['shallow_vid'].cuda(), inp['vid_masks'].cuda(), (texts[0][None],), inp['text_cls'].cuda(), (tmasks[0][None, None],), eval=True)
        torch.cuda.synchronize()
        assert model.numerics_status() & 1 == 0
        return model, texts, tmasks
    return c.model(('half', E, tuple(nqs)), factory)


def _forward(E, lens, nqs, videos_export):
    def make():
        g = gen(73, E, len(lens), sum(nqs))
        specs = []
        for v, (vl, nq) in enumerate(zip(lens, nqs)):
            vid, shallow = rn(g, 64, T_FWD), rn(g, 64, T_FWD)
            vid[:, vl:] = 0
            shallow[:, vl:] = 0
            specs += [(f'vid{v}', half_bytes(vid), 'in', T_FWD * 2), (f'shallow{v}', half_bytes(shallow), 'in', T_FWD * 2),
                      (f'mask{v}', (torch.arange(T_FWD) < vl).to(torch.uint8), 'in'), (f'cls{v}', rn(g, nq, 64), 'in')]
        nq_all = sum(nqs)
        specs += [('logits', out(nq_all, S_FWD), 'out'), ('offsets', out(nq_all, S_FWD, 2), 'out'), ('masks', out(nq_all, S_FWD, dtype=torch.uint8), 'out')]

        def call(c, v):
            model, texts, tmasks = _model(c, E, nqs)
            h = model._engine.handle
            assert c.lib.dcf_points_per_query(h, T_FWD) == S_FWD
            tptr, mptr, tlen = (ctypes.c_void_p * nq_all)(), (ctypes.c_void_p * nq_all)(), (ctypes.c_int32 * nq_all)()
            for q in range(nq_all):
                tptr[q], mptr[q], tlen[q] = texts[q].data_ptr(), tmasks[q].data_ptr(), texts[q].size(1)
            if not videos_export:
                return c.lib.dcf_forward_eval_h(h, p(v['vid0']), p(v['shallow0']), p(v['mask0']), T_FWD, nq_all, tptr, mptr, tlen, p(v['cls0']),
                                                p(v['logits']), p(v['offsets']), p(v['masks']), c.stream())
            n = len(lens)
            arr = lambda name: (ctypes.c_void_p * n)(*[v[f'{name}{i}'].data_ptr() for i in range(n)])
            return c.lib.dcf_forward_eval_videos_h(h, n, arr('vid'), arr('shallow'), arr('mask'), T_FWD, (ctypes.c_int32 * n)(*nqs), tptr, mptr, tlen,
                                                   arr('cls'), p(v['logits']), p(v['offsets']), p(v['masks']), c.stream())
        return specs, call
    return make


NATIVE = (('half_native', 2),)                  # native, or the call fails: the case cannot pass on the upcast path
case('dcf_forward_eval_h', 'E128-q2-native', _forward(128, [150], [2], False), NATIVE)
case('dcf_forward_eval_h', 'E128-q1-scoring-kernels', _forward(128, [192], [1], False), NATIVE + (('fuse_scores', 0),))
case('dcf_forward_eval_h', 'E256-q2-upcast', _forward(256, [150], [2], False), (('half_native', 0),))
case('dcf_forward_eval_videos_h', 'E128-v3-q2_1_1-native', _forward(128, [192, 150, 70], [2, 1, 1], True), NATIVE)
case('dcf_forward_eval_videos_h', 'E256-v2-q2_1-one-grid', _forward(256, [150, 192], [2, 1], True), NATIVE)
case('dcf_forward_eval_videos_h', 'E256-v2-q2_1-scoring-kernels', _forward(256, [150, 192], [2, 1], True), NATIVE + (('fuse_scores', 0),))
case('dcf_forward_eval_videos_h', 'E128-v2-q1_1-upcast', _forward(128, [192, 70], [1, 1], True), (('half_native', 0),))

EXCLUDED = {'dcf_half_ext_version': 'no device operand: returns a constant'}
