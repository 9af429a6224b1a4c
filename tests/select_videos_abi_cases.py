"""One entry per export of the several-video selected-clip extension (include/decafnet_hip_select_videos.h,
``_lib.SELECT_VIDEOS_TABLE``) for tests/test_gpu_select_videos_borders.py, in the format of tests/abi_cases.py:
``Case(export, tag, make, options)`` with ``make()`` -> ``(specs, call)``.

dcf_op_select_clips_videos: three videos of T = 5000 with valid lengths 5000 / 4700 / 77 and 3 / 1 / 2 queries (strip seams, a partly
filled strip, a short video); 16 videos of T = 1; two of T = 4097 (a second strip of one clip).  ``clips`` is placed with its
capacity (nvid, T), so the entries at and beyond each count must keep the sentinel in every run.
dcf_op_gather_clip_rows_videos(_h): D = 100 (a partly filled second tile), three videos with 70 / 1 / 131 rows -- row_first 0, 70,
71, 202: no video starts on a tile boundary --, windows of longer rows (ldx > T); and a video without rows between two with some.  A
half operand is placed as the bytes of its binary16 values as in tests/half_abi_cases.py.
dcf_select_videos(_h) and the two forwards: the finalized models of tests/half_abi_cases.py (E = 128 and 256), T = 192 = three
blocks of 64 clips of which each query keeps one, two videos, one shorter than its padded length.
``nq_per_video``, ``row_first``, the arrays of pointers and ``text`` / ``text_mask`` / ``text_len`` are HOST arrays, and the encoded
text is the model's own: no operands of the arena."""
import ctypes

import torch

import select_videos_ref as V
from abi_cases import Case, gen, out, p, rn
from half_abi_cases import S_FWD, T_FWD, _model, half_bytes
from select_abi_cases import block_gate

CASES = []
i32 = torch.int32


def case(export, tag, make, options=()):
    CASES.append(Case(export, tag, make, tuple(options)))


def ints(xs):
    return (ctypes.c_int32 * len(xs))(*xs)


def ptrs(v, name, n):
    return (ctypes.c_void_p * n)(*[v[f'{name}{i}'].data_ptr() for i in range(n)])


def gates_and_masks(g, T, lens, nqs, sn, keep):
    gate = torch.cat([block_gate(g, nq, T, vl, sn, keep) for vl, nq in zip(lens, nqs)])
    masks = torch.stack([torch.arange(T) < vl for vl in lens]).to(torch.uint8)
    return gate, masks


def _select(T, lens, nqs, sn, keep):
    def make():
        g = gen(91, T, len(lens), sum(nqs), sn, keep)
        gate, masks = gates_and_masks(g, T, lens, nqs, sn, keep)
        nv = len(lens)
        specs = [('gate', gate, 'in'), ('masks', masks, 'in'), ('clips', out(nv, T, dtype=i32), 'out'), ('pos', out(nv, T, dtype=i32), 'out'),
                 ('counts', out(nv, dtype=i32), 'out')]
        return specs, lambda c, v: c.lib.dcf_op_select_clips_videos(p(v['gate']), p(v['masks']), T, nv, ints(nqs), p(v['clips']), p(v['pos']),
                                                                    p(v['counts']), c.stream())
    return make


SELECT_SHAPES = [(5000, [5000, 4700, 77], [3, 1, 2], 60, 23), (1, [1] * 16, [1] * 16, 8, 0), (4097, [4097, 4000], [2, 1], 64, 19)]
for T, lens, nqs, sn, keep in SELECT_SHAPES:
    case('dcf_op_select_clips_videos', f'T{T}-v{len(lens)}-q{sum(nqs)}', _select(T, lens, nqs, sn, keep))


def _gather(D, T, ldx, counts, half):
    def make():
        g = gen(92, D, T, ldx, len(counts), half)
        nv = len(counts)
        first = [0]
        for n in counts:
            first.append(first[-1] + n)
        clips = torch.zeros(nv, T, dtype=i32)
        for v, n in enumerate(counts):
            clips[v, :n] = torch.randperm(T, generator=g)[:n].sort().values.to(i32)
        xs = [rn(g, D, ldx) for _ in range(nv)]
        if half:
            specs = [(f'X{v}', half_bytes(x), 'in', ldx * 2) for v, x in enumerate(xs)]
            specs += [('clips', clips, 'in'), ('rows', out(first[-1], 2 * D, dtype=torch.uint8), 'out')]
            fn = 'dcf_op_gather_clip_rows_videos_h'
        else:
            specs = [(f'X{v}', x, 'in', ldx * 4) for v, x in enumerate(xs)]
            specs += [('clips', clips, 'in'), ('rows', out(first[-1], D), 'out')]
            fn = 'dcf_op_gather_clip_rows_videos'
        return specs, lambda c, v: getattr(c.lib, fn)(ptrs(v, 'X', nv), ldx, p(v['clips']), T, nv, ints(first), D, p(v['rows']), c.stream())
    return make


GATHER_SHAPES = [(100, 300, 333, [70, 1, 131]), (64, 77, 77, [5, 0, 66])]
for D, T, ldx, counts in GATHER_SHAPES:
    tag = f'D{D}-T{T}of{ldx}-n{"_".join(map(str, counts))}'
    case('dcf_op_gather_clip_rows_videos', tag, _gather(D, T, ldx, counts, False))
    case('dcf_op_gather_clip_rows_videos_h', tag, _gather(D, T, ldx, counts, True))


def _features(g, lens, half):
    """per video the shallow features (zero beyond the valid length) as arena operands"""
    specs = []
    for v, vl in enumerate(lens):
        shallow = rn(g, 64, T_FWD)
        shallow[:, vl:] = 0
        specs.append((f'shallow{v}', half_bytes(shallow), 'in', T_FWD * 2) if half else (f'shallow{v}', shallow, 'in', T_FWD * 4))
        specs.append((f'mask{v}', (torch.arange(T_FWD) < vl).to(torch.uint8), 'in'))
    return specs


def _select_videos(E, lens, nqs, half, with_scores):
    def make():
        g = gen(93, E, len(lens), sum(nqs), half)
        nv, NQ = len(lens), sum(nqs)
        specs = _features(g, lens, half)
        specs += [(f'cls{v}', rn(g, nq, 64), 'in') for v, nq in enumerate(nqs)]
        specs += [('gate', out(NQ, T_FWD), 'out'), ('clips', out(nv, T_FWD, dtype=i32), 'out'), ('pos', out(nv, T_FWD, dtype=i32), 'out'),
                  ('counts', out(nv, dtype=i32), 'out')]
        if with_scores:
            specs.append(('correl', out(NQ, T_FWD), 'out'))

        def call(c, v):
            model, _, _ = _model(c, E, nqs)
            fn = c.lib.dcf_select_videos_h if half else c.lib.dcf_select_videos
            return fn(model._engine.handle, nv, ptrs(v, 'shallow', nv), ptrs(v, 'mask', nv), T_FWD, ints(nqs), ptrs(v, 'cls', nv), p(v['gate']),
                      p(v['correl']) if with_scores else None, p(v['clips']), p(v['pos']), p(v['counts']), c.stream())
        return specs, call
    return make


def _forward(E, lens, nqs, half):
    def make():
        g = gen(94, E, len(lens), sum(nqs), half)
        nv, NQ = len(lens), sum(nqs)
        gate, masks = gates_and_masks(g, T_FWD, lens, nqs, 64, 1)
        clips, pos, counts, first = V.select_clips_videos(gate, masks, nqs)
        rows = V.gather_clip_rows_videos([rn(g, 64, T_FWD) for _ in range(nv)], clips, counts)
        specs = _features(g, lens, half)
        specs += [('rows', half_bytes(rows) if half else rows, 'in'), ('pos', pos, 'in'), ('gate', gate, 'in'), ('logits', out(NQ, S_FWD), 'out'),
                  ('offsets', out(NQ, S_FWD, 2), 'out'), ('masks', out(NQ, S_FWD, dtype=torch.uint8), 'out')]

        def call(c, v):
            model, texts, tmasks = _model(c, E, nqs)
            h = model._engine.handle
            assert c.lib.dcf_points_per_query(h, T_FWD) == S_FWD
            tptr, mptr, tlen = (ctypes.c_void_p * NQ)(), (ctypes.c_void_p * NQ)(), (ctypes.c_int32 * NQ)()
            for q in range(NQ):
                tptr[q], mptr[q], tlen[q] = texts[q].data_ptr(), tmasks[q].data_ptr(), texts[q].size(1)
            fn = c.lib.dcf_forward_eval_videos_selected_h if half else c.lib.dcf_forward_eval_videos_selected
            return fn(h, nv, p(v['rows']), ints(first), p(v['pos']), ptrs(v, 'shallow', nv), ptrs(v, 'mask', nv), T_FWD, ints(nqs), tptr, mptr,
                      tlen, p(v['gate']), None, p(v['logits']), p(v['offsets']), p(v['masks']), c.stream())
        return specs, call
    return make


for E, lens, nqs in [(128, [150, 192], [2, 1]), (256, [192, 70], [1, 1])]:
    tag = f'E{E}-v{"_".join(map(str, lens))}-q{"_".join(map(str, nqs))}'
    case('dcf_select_videos', tag + ('-scores' if E == 128 else ''), _select_videos(E, lens, nqs, False, E == 128))
    case('dcf_select_videos_h', tag + ('-scores' if E == 256 else ''), _select_videos(E, lens, nqs, True, E == 256))
    case('dcf_forward_eval_videos_selected', tag, _forward(E, lens, nqs, False))
    case('dcf_forward_eval_videos_selected_h', tag, _forward(E, lens, nqs, True))

EXCLUDED = {'dcf_select_videos_ext_version': 'no device operand: returns a constant'}
