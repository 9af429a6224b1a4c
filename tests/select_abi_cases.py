"""One entry per export of the selected-clip extension (include/decafnet_hip_select.h, ``_lib.SELECT_TABLE``) for
tests/test_gpu_select_borders.py, in the format of tests/abi_cases.py: ``Case(export, tag, make, options)`` with ``make()`` ->
``(specs, call)``.

dcf_op_select_clips: T = 1; T = 16 with every clip kept; T = 4096 (exactly one strip) and 4097 (a second strip of one clip); T = 5000
with three queries and a padded tail (the carry between strips, a partly filled last strip); ``clips`` is placed with its capacity T,
so the entries at and beyond ``count`` must keep the sentinel in every run.  dcf_op_gather_clip_rows(_h): D = 64 (one tile) and
D = 100 (a partly filled second tile), n = 1, n = 70 (a second tile with six rows; no multiple of 4), windows of a longer row
(ldx > T); a half operand is placed as the bytes of its binary16 values as in tests/half_abi_cases.py.  The two forwards: the
finalized models of tests/half_abi_cases.py (E = 128 and 256), T = 192 = three blocks of 64 clips of which each query keeps one, one
and two queries, a video shorter than its padded length; ``text`` / ``text_mask`` / ``text_len`` are host arrays and the encoded
text is the model's own: no operands of the arena."""
import ctypes

import torch

import select_ref
from abi_cases import Case, gen, out, p, rn
from half_abi_cases import S_FWD, T_FWD, _model, half_bytes

CASES = []
i32 = torch.int32


def case(export, tag, make, options=()):
    CASES.append(Case(export, tag, make, tuple(options)))


def block_gate(g, nq, T, vid_len, sn, keep):
    """(nq, T) 0 / 1: per query ``keep`` random blocks of ``sn`` clips of the first vid_len clips (keep = 0: every block)"""
    n = (vid_len + sn - 1) // sn
    gate = torch.zeros(nq, T)
    for q in range(nq):
        blocks = torch.randperm(n, generator=g)[:keep] if keep else torch.arange(n)
        for b in blocks.tolist():
            gate[q, b * sn:min((b + 1) * sn, vid_len)] = 1
    return gate


def _select(T, nq, vid_len, sn, keep):
    def make():
        g = gen(81, T, nq, vid_len, sn, keep)
        specs = [('gate', block_gate(g, nq, T, vid_len, sn, keep), 'in'), ('mask', (torch.arange(T) < vid_len).to(torch.uint8), 'in'),
                 ('clips', out(T, dtype=i32), 'out'), ('pos', out(T, dtype=i32), 'out'), ('count', out(1, dtype=i32), 'out')]
        return specs, lambda c, v: c.lib.dcf_op_select_clips(p(v['gate']), p(v['mask']), T, nq, p(v['clips']), p(v['pos']), p(v['count']), c.stream())
    return make


for T, nq, vl, sn, keep in [(1, 1, 1, 8, 0), (16, 2, 16, 8, 0), (4096, 1, 4096, 64, 19), (4097, 2, 4097, 64, 19), (5000, 3, 4700, 60, 23)]:
    case('dcf_op_select_clips', f'T{T}-v{vl}-q{nq}-keep{keep}', _select(T, nq, vl, sn, keep))


def _gather(D, T, ldx, n, half):
    def make():
        g = gen(82, D, T, ldx, n, half)
        x = rn(g, D, ldx)
        clips = torch.randperm(T, generator=g)[:n].sort().values.to(i32)
        if half:
            specs = [('X', half_bytes(x), 'in', ldx * 2), ('clips', clips, 'in'), ('rows', out(n, 2 * D, dtype=torch.uint8), 'out')]
            return specs, lambda c, v: c.lib.dcf_op_gather_clip_rows_h(p(v['X']), ldx, p(v['clips']), n, D, p(v['rows']), c.stream())
        specs = [('X', x, 'in', ldx * 4), ('clips', clips, 'in'), ('rows', out(n, D), 'out')]
        return specs, lambda c, v: c.lib.dcf_op_gather_clip_rows(p(v['X']), ldx, p(v['clips']), n, D, p(v['rows']), c.stream())
    return make


for D, T, ldx, n in [(64, 77, 77, 1), (100, 200, 200, 70), (64, 130, 200, 70), (3, 5, 5, 5)]:
    case('dcf_op_gather_clip_rows', f'D{D}-T{T}of{ldx}-n{n}', _gather(D, T, ldx, n, False))
    case('dcf_op_gather_clip_rows_h', f'D{D}-T{T}of{ldx}-n{n}', _gather(D, T, ldx, n, True))


def _forward(E, vid_len, nq, half):
    def make():
        g = gen(83, E, vid_len, nq, half)
        vid, shallow = rn(g, 64, T_FWD), rn(g, 64, T_FWD)
        shallow[:, vid_len:] = 0
        mask = torch.arange(T_FWD) < vid_len
        gate = block_gate(g, nq, T_FWD, vid_len, 64, 1)
        clips, pos, n = select_ref.select_clips(gate, mask)
        rows = select_ref.gather_clip_rows(vid, clips)
        if half:
            specs = [('rows', half_bytes(rows), 'in'), ('shallow', half_bytes(shallow), 'in', T_FWD * 2)]
        else:
            specs = [('rows', rows, 'in'), ('shallow', shallow, 'in', T_FWD * 4)]
        specs += [('pos', pos, 'in'), ('mask', mask.to(torch.uint8), 'in'), ('gate', gate, 'in'), ('logits', out(nq, S_FWD), 'out'),
                  ('offsets', out(nq, S_FWD, 2), 'out'), ('masks', out(nq, S_FWD, dtype=torch.uint8), 'out')]

        def call(c, v):
            model, texts, tmasks = _model(c, E, [nq])
            h = model._engine.handle
            assert c.lib.dcf_points_per_query(h, T_FWD) == S_FWD
            tptr, mptr, tlen = (ctypes.c_void_p * nq)(), (ctypes.c_void_p * nq)(), (ctypes.c_int32 * nq)()
            for q in range(nq):
                tptr[q], mptr[q], tlen[q] = texts[q].data_ptr(), tmasks[q].data_ptr(), texts[q].size(1)
            fn = c.lib.dcf_forward_eval_selected_h if half else c.lib.dcf_forward_eval_selected
            return fn(h, p(v['rows']), n, p(v['pos']), p(v['shallow']), p(v['mask']), T_FWD, nq, tptr, mptr, tlen, p(v['gate']), p(v['logits']),
                      p(v['offsets']), p(v['masks']), c.stream())
        return specs, call
    return make


for E, vl, nq in [(128, 150, 2), (256, 192, 1)]:
    case('dcf_forward_eval_selected', f'E{E}-v{vl}-q{nq}', _forward(E, vl, nq, False))
    case('dcf_forward_eval_selected_h', f'E{E}-v{vl}-q{nq}', _forward(E, vl, nq, True))

EXCLUDED = {'dcf_select_ext_version': 'no device operand: returns a constant'}
