"""Selected-clip inference on several videos per forward, on the GPU (include/decafnet_hip_select_videos.h):
``model.select_clips_videos`` -> the packed expert rows -> ``model.forward_videos_selected``, and the evaluator's switch
``select_videos=True``.

Exact wherever nothing is summed differently: the clip lists, their inverses and the counts against tests/select_videos_ref.py and
against the one-video operator run video by video, the gathered rows against indexing, the gates against the one-video
``model.select_clips`` (every top-k choice of these inputs is decided by more than 1e-4, tests/test_select_videos_cpu.py, against the
2e-6 the scoring kernels differ by), masks, repeated calls, half rows against fp32 rows of the same values, one video against
``forward_selected``.  Where the GPU meets a reference the gate is the project's parity rule (tests/forward_parity.py):

    e_gpu <= max(4 e_ref, 2^-21 max|y64|)

with y32 the reference's fixture or the fp32 oracle and y64 the fp64 oracle, per video, on that video's dense features.  The
difference to per-video ``forward_selected`` and to the dense ``forward_videos`` is printed (``SELVDIFF`` lines, recorded in
profiles/selected_videos.md) and not asserted: the packed product may take another tile form than a per-video one."""
import ctypes

import pytest
import torch

import forward_parity as P
import select_ref as S
import select_videos_abi_cases as C
import select_videos_ref as V
from abi_cases import gen
from conftest import load_pkg

pytestmark = pytest.mark.gpu
R = S.R
i32 = torch.int32


def build(pkg, kw, shapes_or_none, wseed, max_batch=None):
    opt = pkg.config.make_opt(**kw)
    if max_batch:
        opt.model['max_batch'] = max_batch
    model = pkg.modeling.create_model(opt)
    shapes = shapes_or_none or {k: list(v.shape) for k, v in model.state_dict().items()}
    sd = pkg.synth.make_state_dict(shapes, wseed)
    model.load_state_dict(sd)
    return opt, model.cuda().eval().requires_grad_(False), sd


def encode(model, tokens):
    tm = [model.encode_text(t[None].cuda(), torch.ones(1, 1, t.size(-1), dtype=torch.bool, device='cuda')) for t in tokens]
    return tuple(t for t, _ in tm), tuple(m for _, m in tm)


def video_of(model, inp, half=False):
    texts, tmasks = encode(model, inp['tokens'])
    cast = (lambda x: x.half()) if half else (lambda x: x)
    return (cast(inp['vid']).cuda(), cast(inp['shallow_vid']).cuda(), inp['vid_masks'].cuda(), texts, inp['text_cls'].cuda(), tmasks)


def flat(out):
    """every tensor of one video's (logits, offsets, masks) result on the host, in one list"""
    return [x.cpu().clone() for part in out for q in part for x in q]


def same_bits(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------- dcf_op_select_clips_videos
@pytest.mark.parametrize('T,lens,nqs,sn,keep', C.SELECT_SHAPES, ids=[f'T{s[0]}-v{len(s[1])}' for s in C.SELECT_SHAPES])
def test_select_clips_videos_equals_the_restatement_and_the_one_video_operator(T, lens, nqs, sn, keep):
    pkg = load_pkg()
    lib, p, st = pkg._lib.lib(), pkg._lib.ptr, pkg._lib.current_stream()
    gate, masks = C.gates_and_masks(gen(95, T, len(lens)), T, lens, nqs, sn, keep)
    if T == 5000:
        masks[0, 4090:4100] = 0                                   # invalid clips under open gates, across the strip seam
        gate[:3, 4080:4110] = 1
    nv = len(lens)
    gd, md = gate.cuda(), masks.cuda()
    clips = torch.full((nv, T), -7, dtype=i32, device='cuda')
    pos = torch.full((nv, T), -7, dtype=i32, device='cuda')
    counts = torch.full((nv,), -7, dtype=i32, device='cuda')
    pkg._lib.check(lib.dcf_op_select_clips_videos(p(gd), p(md), T, nv, C.ints(nqs), p(clips), p(pos), p(counts), st), 'dcf_op_select_clips_videos')
    want_clips, want_pos, want_counts, _ = V.select_clips_videos(gate, masks, nqs, fill=-7)
    assert counts.cpu().tolist() == want_counts
    assert torch.equal(clips.cpu(), want_clips), 'a list differs, or an entry at or beyond a count was written'
    assert torch.equal(pos.cpu(), want_pos)
    if T > 1:
        assert 0 < min(want_counts) and max(want_counts) < T
    q = 0
    for v in range(nv):                                           # row v: the bits of dcf_op_select_clips on video v alone
        c1 = torch.full((T,), -7, dtype=i32, device='cuda')
        p1 = torch.full((T,), -7, dtype=i32, device='cuda')
        n1 = torch.full((1,), -7, dtype=i32, device='cuda')
        pkg._lib.check(lib.dcf_op_select_clips(p(gd[q:q + nqs[v]].contiguous()), p(md[v].contiguous()), T, nqs[v], p(c1), p(p1), p(n1), st),
                       'dcf_op_select_clips')
        assert torch.equal(c1, clips[v]) and torch.equal(p1, pos[v]) and int(n1) == int(counts[v])
        q += nqs[v]


def test_select_clips_videos_refusals():
    pkg = load_pkg()
    lib, p, st = pkg._lib.lib(), pkg._lib.ptr, pkg._lib.current_stream()
    gate, masks = torch.ones(17, 4, device='cuda'), torch.ones(17, 4, dtype=torch.uint8, device='cuda')
    clips = torch.full((17, 4), -7, dtype=i32, device='cuda')
    pos, counts = clips.clone(), torch.full((17,), -7, dtype=i32, device='cuda')
    for nv, nqs, word in ((17, [1] * 17, 'videos'), (0, [1], 'videos'), (2, [1, 0], 'queries')):
        assert lib.dcf_op_select_clips_videos(p(gate), p(masks), 4, nv, C.ints(nqs), p(clips), p(pos), p(counts), st) == -1
        assert word in lib.dcf_last_error().decode()
    torch.cuda.synchronize()
    assert bool((clips == -7).all()) and bool((pos == -7).all()) and bool((counts == -7).all())


# ---------------------------------------------------------------------------------------------- dcf_op_gather_clip_rows_videos
@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
def test_gather_clip_rows_videos_equals_indexing(dtype):
    """D = 100, counts 70 / 1 / 131 (row_first 0, 70, 71, 202: no video starts on a tile boundary), windows of longer rows"""
    pkg = load_pkg()
    lib, p = pkg._lib.lib(), pkg._lib.ptr
    D, T, ldx, counts = C.GATHER_SHAPES[0]
    assert (D, counts) == (100, [70, 1, 131]) and ldx > T
    g = torch.Generator().manual_seed(17)
    xs = [torch.randn(D, ldx, generator=g).to(dtype) for _ in counts]
    clips = torch.full((3, T), -1, dtype=i32)
    for v, n in enumerate(counts):
        clips[v, :n] = torch.randperm(T, generator=g)[:n].sort().values.to(i32)
    first = [0, 70, 71, 202]
    xd, cd = [x.cuda() for x in xs], clips.cuda()
    rows = torch.full((first[-1] + 3, D), float('nan'), dtype=dtype, device='cuda')       # three rows of capacity behind the last
    fn = lib.dcf_op_gather_clip_rows_videos_h if dtype == torch.float16 else lib.dcf_op_gather_clip_rows_videos
    xp = (ctypes.c_void_p * 3)(*[x.data_ptr() for x in xd])
    pkg._lib.check(fn(xp, ldx, p(cd), T, 3, C.ints(first), D, p(rows), pkg._lib.current_stream()), 'dcf_op_gather_clip_rows_videos')
    got = rows.cpu()
    assert torch.equal(got[:first[-1]], V.gather_clip_rows_videos(xs, clips, counts))
    assert bool(got[first[-1]:].isnan().all()), 'a row beyond row_first[nvid] was written'


# ---------------------------------------------------------------------------------------------- the three videos
VARIANTS = ['msf', 'nomsf', 'msf_chunked', 'scat', 'half']


@pytest.fixture(scope='module')
def runs():
    """per variant: the model, the three videos, the batch, the packed rows and the result of one forward_videos_selected"""
    pkg = load_pkg()
    made = {}

    def get(variant):
        if variant not in made:
            kw = dict(V.KW3, msf=variant != 'nomsf', scat=variant == 'scat')
            opt, model, sd = build(pkg, kw, None, V.WSEED3, max_batch=4 if variant == 'msf_chunked' else None)
            inputs = V.three_inputs(pkg)
            videos = [video_of(model, inp, half=variant == 'half') for inp in inputs]
            batch = model.select_clips_videos(videos)
            rows = model.gather_clip_rows_videos([a[0] for a in videos], batch)
            out = model.forward_videos_selected(rows, batch, videos)
            made[variant] = (pkg, opt, model, sd, inputs, videos, batch, rows, out, [flat(o) for o in out])
        return made[variant]
    return get


@pytest.mark.parametrize('variant', ['msf', 'scat', 'half'])
def test_select_clips_videos_equals_per_video_select_clips(runs, variant, monkeypatch):
    """gate, pos, clips and counts of the one call are those of the one-video method, video by video; the scores of a scat model are
    handed on; the call reads the device ONCE"""
    pkg, opt, model, sd, inputs, videos, batch, rows, out, bits = runs(variant)
    assert batch.nvid == 3 and batch.nqs == [2, 1, 3] and batch.T == V.T3 and batch.row_first[-1] == sum(batch.counts) == rows.size(0)
    assert (batch.scores is not None) == (variant == 'scat')
    assert batch.gate.dtype == torch.float32 and batch.pos.dtype == batch.clips.dtype == i32
    if variant == 'scat':
        plain = build(pkg, V.KW3, None, V.WSEED3)[1]              # the one-video method refuses scat: the same gate, from a model without
        lib, p = pkg._lib.lib(), pkg._lib.ptr
    q = 0
    for v, a in enumerate(videos):
        sel = (plain if variant == 'scat' else model).select_clips(a[1], a[2], a[4])
        n = sel.count
        assert batch.counts[v] == n and 0 < n <= V.LENS3[v][0]
        assert torch.equal(batch.gate[q:q + sel.nq], sel.gate) and torch.equal(batch.pos[v], sel.pos)
        assert torch.equal(batch.clips[v, :n], sel.clips) and torch.equal(batch.clips_host(v), sel.clips_host())
        one = batch.selection(v)
        assert one.count == n and torch.equal(one.clips, sel.clips) and torch.equal(one.gate, sel.gate) and torch.equal(one.pos, sel.pos)
        want = S.oracle_gates(opt.model, inputs[v]['shallow_vid'].half().float() if variant == 'half' else inputs[v]['shallow_vid'],
                              inputs[v]['vid_masks'], inputs[v]['text_cls'])
        assert torch.equal(sel.gate.cpu(), want)
        if variant == 'scat':                                     # the scores: those of dcf_op_sidekick on this video
            correl = torch.empty(sel.nq, V.T3, device='cuda')
            pkg._lib.check(lib.dcf_op_sidekick(p(a[1][0].contiguous()), p(a[4].contiguous()), p(correl), 64, V.T3, sel.nq, 1,
                                               pkg._lib.current_stream()), 'dcf_op_sidekick')
            assert torch.equal(batch.scores[q:q + sel.nq], correl)
        q += sel.nq
    want_rows = V.gather_clip_rows_videos([a[0][0].cpu() for a in videos], batch.clips.cpu(), batch.counts)
    assert rows.dtype == videos[0][0].dtype and torch.equal(rows.cpu(), want_rows)
    reads = []
    for name in ('cpu', 'item', 'tolist', 'numpy', 'to'):
        def counted(self, *args, _orig=getattr(torch.Tensor, name), _name=name, **kwargs):
            res = _orig(self, *args, **kwargs)
            if self.is_cuda and not (torch.is_tensor(res) and res.is_cuda):
                reads.append(_name)
            return res
        monkeypatch.setattr(torch.Tensor, name, counted)
    again = model.select_clips_videos(videos)
    assert reads == ['cpu'], f'device-to-host reads of one select_clips_videos call: {reads}'
    monkeypatch.undo()
    assert again.counts == batch.counts and torch.equal(again.gate, batch.gate) and torch.equal(again.pos, batch.pos)


def _oracle(sd, cfg, inp, a, half):
    rnd = (lambda x: x.half().float()) if half else (lambda x: x)
    args = (rnd(inp['vid']), rnd(inp['shallow_vid']), inp['vid_masks'], [t.cpu() for t in a[3]], inp['text_cls'], [m.cpu() for m in a[5]])
    with torch.no_grad():
        y32 = R.forward_eval(sd, cfg, *args)
    return y32, P.oracle64.forward_eval(sd, cfg, *args)


@pytest.mark.parametrize('variant', VARIANTS)
def test_forward_videos_selected_against_the_oracle(runs, variant):
    """per video: masks exact, logits and offsets under the parity rule against the fp32 / fp64 oracle on that video's dense features"""
    pkg, opt, model, sd, inputs, videos, batch, rows, out, bits = runs(variant)
    assert len(out) == 3 and model.graph_active() == 0 and model.numerics_status() & 1 == 0
    assert model.last_feature_dtype == (torch.float16 if variant == 'half' else torch.float32)
    for v, (inp, a) in enumerate(zip(inputs, videos)):
        lg, of, mk = out[v]
        y32, y64 = _oracle(sd, opt.model, inp, a, variant == 'half')
        assert len(lg) == len(of) == len(mk) == V.LENS3[v][1]
        for q in range(len(lg)):
            for l in range(4):
                assert torch.equal(y32[2][q][l], y64[2][q][l]) and torch.equal(mk[q][l].cpu(), y32[2][q][l]), (v, q, l)
        P.check(f'videos-selected {variant} v{v} logits', P.pool(lg), P.pool(y64[0]), P.pool(y32[0]))
        P.check(f'videos-selected {variant} v{v} offsets', P.pool(of), P.pool(y64[1]), P.pool(y32[1]))


@pytest.mark.parametrize('variant', VARIANTS)
def test_repeats_capacity_rows_and_unselected_clips(runs, variant):
    """two calls give equal bits; NaN capacity rows behind the packed rows change nothing; 3e4 in every unselected clip of the dense
    source changes neither the gathered rows nor the outputs"""
    pkg, opt, model, sd, inputs, videos, batch, rows, out, bits = runs(variant)
    cap = torch.full((rows.size(0) + 5, 64), float('nan'), dtype=rows.dtype, device='cuda')
    cap[:rows.size(0)] = rows
    again = model.forward_videos_selected(cap, batch, videos)
    assert all(same_bits(flat(o), b) for o, b in zip(again, bits))
    vids = []
    for v, a in enumerate(videos):
        outside = torch.ones(V.T3, dtype=torch.bool, device='cuda')
        outside[batch.clips[v, :batch.counts[v]].long()] = False
        assert bool(outside.any())
        x = a[0].clone()
        x[:, :, outside] = 3.0e4
        vids.append(x)
    rows2 = model.gather_clip_rows_videos(vids, batch)
    assert torch.equal(rows2, rows)
    third = model.forward_videos_selected(rows2, batch, videos)
    assert all(same_bits(flat(o), b) for o, b in zip(third, bits))
    assert all(bool(torch.isfinite(x).all()) for b in bits for x in b if x.is_floating_point())


def test_half_rows_give_what_fp32_rows_of_the_same_values_give(runs):
    pkg, opt, model, sd, inputs, videos, batch, rows, out, bits = runs('half')
    assert rows.dtype == torch.float16
    videos32 = [(a[0].float(), a[1].float()) + a[2:] for a in videos]
    batch32 = model.select_clips_videos(videos32)
    assert batch32.counts == batch.counts and torch.equal(batch32.gate, batch.gate) and torch.equal(batch32.pos, batch.pos)
    want = model.forward_videos_selected(rows.float(), batch32, videos32)
    assert model.last_feature_dtype == torch.float32
    assert all(same_bits(flat(o), b) for o, b in zip(want, bits))
    with pytest.raises(ValueError, match='float16'):
        model.forward_videos_selected(rows, batch, videos32)


@pytest.mark.parametrize('variant', ['msf', 'nomsf', 'msf_chunked', 'half'])
def test_one_video_is_bit_identical_to_forward_selected(runs, variant):
    pkg, opt, model, sd, inputs, videos, batch, rows, out, bits = runs(variant)
    for v, a in enumerate(videos):
        b1 = model.select_clips_videos([a])
        got = model.forward_videos_selected(model.gather_clip_rows_videos([a[0]], b1), b1, [a])
        sel = model.select_clips(a[1], a[2], a[4])
        assert b1.counts == [sel.count] and torch.equal(b1.pos[0], sel.pos) and torch.equal(b1.gate, sel.gate)
        want = model.forward_selected(model.gather_clip_rows(a[0], sel), sel, a[1], a[2], a[3], a[5])
        assert len(got) == 1 and same_bits(flat(got[0]), flat(want)), (variant, v)


@pytest.mark.parametrize('variant', VARIANTS)
def test_difference_to_the_per_video_and_the_dense_forwards_is_printed(runs, variant):
    pkg, opt, model, sd, inputs, videos, batch, rows, out, bits = runs(variant)
    dense = model.forward_videos(videos)
    for v, a in enumerate(videos):
        assert all(torch.equal(x, y) for qa, qb in zip(out[v][2], dense[v][2]) for x, y in zip(qa, qb))     # masks
        refs = [('dense forward_videos', dense[v])]
        if variant != 'scat':                                     # (the one-video forward refuses scat)
            sel = batch.selection(v)
            refs.append(('per-video forward_selected', model.forward_selected(model.gather_clip_rows(a[0], sel), sel, a[1], a[2], a[3], a[5])))
        for what, ref in refs:
            for kind, x, y in (('logits', out[v][0], ref[0]), ('offsets', out[v][1], ref[1])):
                print(f'SELVDIFF {variant} v{v} {kind}: max |videos-selected - {what}| = {float((P.pool(x) - P.pool(y)).abs().max()):.3e}, '
                      f'max |y| = {float(P.pool(y).abs().max()):.3e}')


def test_refusals_of_the_entry_points(runs):
    """by the C entry points themselves, before any launch (rc -1 and a message; the outputs keep their bits)"""
    pkg, opt, model, sd, inputs, videos, batch, rows, out, bits = runs('msf')
    lib, p, st = pkg._lib.lib(), pkg._lib.ptr, pkg._lib.current_stream()
    h = model._engine.handle
    S_pts = lib.dcf_points_per_query(h, V.T3)
    logits, offsets = torch.full((6, S_pts), -3.0, device='cuda'), torch.full((6, S_pts, 2), -3.0, device='cuda')
    masks = torch.zeros(6, S_pts, dtype=torch.bool, device='cuda')
    keep = [(t[0].contiguous().float(), m.reshape(-1).contiguous()) for a in videos for t, m in zip(a[3], a[5])]
    tptr, mptr = (ctypes.c_void_p * 6)(*[t.data_ptr() for t, _ in keep]), (ctypes.c_void_p * 6)(*[m.data_ptr() for _, m in keep])
    tlen = C.ints([t.size(1) for t, _ in keep])
    sh = [a[1][0].contiguous() for a in videos]
    vm = [a[2].reshape(-1).contiguous() for a in videos]
    sp, mp = (ctypes.c_void_p * 3)(*[x.data_ptr() for x in sh]), (ctypes.c_void_p * 3)(*[x.data_ptr() for x in vm])

    def call(first, correl=None, nqs=(2, 1, 3), nv=3):
        rc = lib.dcf_forward_eval_videos_selected(h, nv, p(rows), C.ints(first), p(batch.pos), sp, mp, V.T3, C.ints(list(nqs)), tptr, mptr, tlen,
                                                  p(batch.gate), p(correl), p(logits), p(offsets), p(masks), st)
        return rc, lib.dcf_last_error().decode()
    f = batch.row_first
    for bad in ([1] + f[1:], [f[0], f[1], f[1], f[3]], [f[0], f[2], f[1], f[3]], [0, V.T3 + 1, V.T3 + 2, V.T3 + 3]):
        rc, msg = call(bad)
        assert rc == -1 and 'row' in msg, (bad, msg)
    rc, msg = call(f, correl=batch.gate)                          # scores for a model without scat
    assert rc == -1 and 'scat' in msg
    rc, msg = call(f, nv=17)
    assert rc == -1 and 'videos' in msg
    torch.cuda.synchronize()
    assert bool((logits == -3.0).all()) and bool((offsets == -3.0).all())
    pkg2, opt2, scat, *_ = runs('scat')
    rc = lib.dcf_forward_eval_videos_selected(scat._engine.handle, 3, p(rows), C.ints(f), p(batch.pos), sp, mp, V.T3, C.ints([2, 1, 3]), tptr, mptr,
                                              tlen, p(batch.gate), None, p(logits), p(offsets), p(masks), st)
    assert rc == -1 and 'scat' in lib.dcf_last_error().decode()   # a scat model without the scores
    torch.cuda.synchronize()
    assert bool((logits == -3.0).all())


# ---------------------------------------------------------------------------------------------- the fixtures
@pytest.mark.parametrize('name', ['c1', 'scat'])
def test_fixture_beside_a_second_video(name):
    """the reference's fixture as video 0 of a forward of two: its gates are the oracle's, its outputs pass the rule against the
    fixture's recorded values; the second video passes it against the oracle"""
    pkg = load_pkg()
    c = P.e2e_case(name)
    opt, model, sd = build(pkg, c.kw, c.g.js('shapes'), c.meta['wseed'])
    second = V.second_input(pkg, c)
    videos = [video_of(model, c.inp), video_of(model, second)]
    batch = model.select_clips_videos(videos)
    q = 0
    for v, inp in enumerate((c.inp, second)):
        want = S.oracle_gates(c.opt.model, inp['shallow_vid'], inp['vid_masks'], inp['text_cls'])
        nq = want.shape[0]
        assert torch.equal(batch.gate[q:q + nq].cpu(), want)
        clips, pos, n = S.select_clips(want, inp['vid_masks'][0])
        assert batch.counts[v] == n and torch.equal(batch.clips[v, :n].cpu(), clips) and torch.equal(batch.pos[v].cpu(), pos)
        q += nq
    assert (batch.scores is not None) == (name == 'scat')
    rows = model.gather_clip_rows_videos([a[0] for a in videos], batch)
    out = model.forward_videos_selected(rows, batch, videos)
    lg, of, mk = out[0]
    for q in range(c.nq):
        for l in range(c.L):
            assert torch.equal(mk[q][l].cpu(), c.masks[q][l]), (q, l)
    for kind, got in (('logits', lg), ('offsets', of)):
        P.check(f'videos-selected e2e_{name} {kind}', P.pool(got), P.pool(c.y64[kind]), P.pool(c.y32[kind]))
    y32, y64 = _oracle(sd, opt.model, second, videos[1], False)
    lg, of, mk = out[1]
    for q in range(2):
        for l in range(c.L):
            assert torch.equal(mk[q][l].cpu(), y32[2][q][l])
    P.check(f'videos-selected e2e_{name} second video logits', P.pool(lg), P.pool(y64[0]), P.pool(y32[0]))
    P.check(f'videos-selected e2e_{name} second video offsets', P.pool(of), P.pool(y64[1]), P.pool(y32[1]))
    assert model.numerics_status() & 1 == 0 and model.graph_active() == 0


# ---------------------------------------------------------------------------------------------- the evaluator
def test_evaluator_select_videos():
    """run(batch_videos=3) with select_videos=True against run(batch_videos=1) with expert='selected': expert_fn once per video with
    ascending indices below the video's length, logits under the rule, the same kept segments, equal device tables"""
    pkg = load_pkg()
    ev = pkg.evaluator
    opt, model, sd = build(pkg, V.TINY, None, 21)
    samples = V.evaluator_samples()
    lens = {s['clip_id']: s['vid'].size(-1) for s in samples}
    calls = []

    def expert_fn(sample, clips):
        assert clips.dtype == torch.int64 and not clips.is_cuda and clips.numel() >= 1
        assert bool((clips[1:] > clips[:-1]).all()) and int(clips.min()) >= 0 and int(clips.max()) < lens[sample['clip_id']]
        calls.append(sample['clip_id'])
        return sample['vid'][:, clips].t().contiguous()

    class Recorder(ev.RecallCounter):
        def __init__(self):
            super().__init__()
            self.results = []

        def update(self, results, targets):
            self.results.append(results)
            super().update(results, targets)

    one = ev.GroundingEvaluator(opt, model, expert='selected', expert_fn=expert_fn)
    many = ev.GroundingEvaluator(opt, model, expert='selected', expert_fn=expert_fn, select_videos=True)
    gathered = ev.GroundingEvaluator(opt, model, expert='selected', select_videos=True)
    # ---- the logits of the group of three under the rule, against the oracle on each video's window
    pending = []
    for s in samples[:3]:
        args, T, ext = many.prepare(s)
        assert T == 128
        pending.append((s, args, T, ext))
    many._forward_group(pending)
    assert calls == [s['clip_id'] for s in samples[:3]]
    logits, offsets, masks = (x.cpu().clone() for x in model._last_flat)
    gathered._forward_group([(s, gathered.prepare(s)[0], 128, None) for s in samples[:3]])
    assert all(torch.equal(x.cpu(), y) for x, y in zip(model._last_flat, (logits, offsets, masks))), 'expert_fn=None gathers the same rows'
    sizes = [128 >> l for l in range(4)]
    q = 0
    for s, args, T, _ in pending:
        window, shallow_w, mask, texts, text_cls, tmasks = gathered.prepare(s)[0]
        nq = len(texts)
        ocpu = (window.cpu(), shallow_w.cpu(), mask.cpu(), [t.cpu() for t in texts], text_cls.cpu(), [m.cpu() for m in tmasks])
        with torch.no_grad():
            y32 = R.forward_eval(sd, opt.model, *ocpu)
        y64 = P.oracle64.forward_eval(sd, opt.model, *ocpu)
        lg = [[x[None] for x in logits[q + i].split(sizes)] for i in range(nq)]
        for i in range(nq):
            assert torch.equal(torch.cat([m.reshape(-1) for m in y32[2][i]]), masks[q + i])
        P.check(f'evaluator select_videos {s["clip_id"]} logits', P.pool(lg), P.pool(y64[0]), P.pool(y32[0]))
        (lg1, _, _), _ = one.forward(s)
        d = float((lg1.cpu() - logits[q:q + nq]).abs().max())
        print(f'SELVDIFF evaluator {s["clip_id"]} logits: max |batch_videos=3 - batch_videos=1| = {d:.3e}')
        q += nq
    # ---- the host route: the same kept segments
    del calls[:]
    r1 = one.run(samples, counter=Recorder())
    assert calls == [s['clip_id'] for s in samples]
    del calls[:]
    r3 = many.run(samples, counter=Recorder(), batch_videos=3)
    assert calls == [s['clip_id'] for s in samples], 'expert_fn once per video'
    assert many.last_selection.nvid == 1                          # the video of another padded length went alone
    assert r1.n_queries == r3.n_queries == sum(len(s['text']) for s in samples) and len(r1.results) == len(r3.results) == len(samples)
    kept = 0
    for res1, res3 in zip(r1.results, r3.results):
        assert len(res1) == len(res3)
        for a, b in zip(res1, res3):
            assert a['segments'].shape == b['segments'].shape, 'another number of kept segments'
            torch.testing.assert_close(b['segments'].cpu(), a['segments'].cpu(), rtol=1e-4, atol=1e-3)
            torch.testing.assert_close(b['scores'].cpu(), a['scores'].cpu(), rtol=1e-4, atol=1e-5)
            kept += a['segments'].shape[0]
    assert kept > 0 and (r1.hits == r3.hits).all()
    # ---- the device route: equal tables
    d1 = one.run(samples, counter=ev.DeviceRecallCounter())
    d3 = many.run(samples, counter=ev.DeviceRecallCounter(), batch_videos=3)
    d3g = gathered.run(samples, counter=ev.DeviceRecallCounter(), batch_videos=3)
    assert d1.n_queries == d3.n_queries == d3g.n_queries == r1.n_queries
    assert (d1.hits == d3.hits).all() and (d1.hits == d3g.hits).all()
    assert model.numerics_status() & 1 == 0


def test_evaluator_select_videos_takes_a_scat_model():
    pkg = load_pkg()
    ev = pkg.evaluator
    opt, model, sd = build(pkg, dict(V.TINY, scat=True), None, 21)
    samples = V.evaluator_samples()
    dense = ev.GroundingEvaluator(opt, model).run(samples, counter=ev.DeviceRecallCounter(), batch_videos=3)
    sel = ev.GroundingEvaluator(opt, model, expert='selected', select_videos=True)
    got = sel.run(samples, counter=ev.DeviceRecallCounter(), batch_videos=3)
    assert sel.last_selection.scores is not None
    assert got.n_queries == dense.n_queries == sum(len(s['text']) for s in samples) and got.hits.shape == dense.hits.shape
    alone = sel.run(samples[:1], counter=ev.DeviceRecallCounter())          # batch_videos = 1: a group of one, scat included
    assert alone.n_queries == len(samples[0]['text'])
    with pytest.raises(NotImplementedError, match='scat'):
        ev.GroundingEvaluator(opt, model, expert='selected').run(samples[:1])
