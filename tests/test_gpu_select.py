"""Selected-clip inference on the GPU (include/decafnet_hip_select.h): ``model.select_clips`` -> the expert rows of the selected clips
-> ``model.forward_selected``, and the evaluator's opt-in ``expert='selected'``.

Exact wherever nothing is summed differently: the clip list and its inverse against tests/select_ref.py, the gathered rows against
indexing, the gates of the fixtures against the oracle's (their top-k choice is decided by more than 1e-4, tests/test_select_cpu.py,
against the 2e-6 the scoring kernels are known to differ by), masks, repeated calls, half rows against fp32 rows of the same values.
Where the GPU meets a reference the gate is the project's parity rule (tests/forward_parity.py):

    e_gpu <= max(4 e_ref, 2^-21 max|y64|)

with y32 the reference's fixture (the four fixtures) or the fp32 oracle (the probe-width model, the evaluator's window) and y64 the
fp64 oracle.  The difference between ``forward_selected`` and ``forward_window(dense vid, gate=selection.gate)`` is printed
(``SELDIFF`` lines, recorded in profiles/selected_clips.md) and not asserted: the two expert products accumulate in different tile
shapes."""
import ctypes

import pytest
import torch

import forward_parity as P
import select_ref as S
from conftest import load_pkg
from select_abi_cases import block_gate

pytestmark = pytest.mark.gpu
R = S.R
i32 = torch.int32


def build(pkg, kw, shapes_or_none, wseed, gemm_mode=None):
    opt = pkg.config.make_opt(**kw)
    if gemm_mode:
        opt.model['gemm_mode'] = gemm_mode
    model = pkg.modeling.create_model(opt)
    shapes = shapes_or_none or {k: list(v.shape) for k, v in model.state_dict().items()}
    sd = pkg.synth.make_state_dict(shapes, wseed)
    model.load_state_dict(sd)
    return opt, model.cuda().eval().requires_grad_(False), sd


def encode(model, tokens):
    tm = [model.encode_text(t[None].cuda(), torch.ones(1, 1, t.size(-1), dtype=torch.bool, device='cuda')) for t in tokens]
    return tuple(t for t, _ in tm), tuple(m for _, m in tm)


def flat(out):
    """every tensor of a (logits, offsets, masks) result on the host, in one list"""
    return [x.cpu().clone() for part in out for q in part for x in q]


def same_bits(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and torch.equal(x, y) and torch.equal(x.isnan() if x.is_floating_point() else x,
                                                                                             y.isnan() if y.is_floating_point() else y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------- dcf_op_select_clips
def run_select(pkg, gate, mask):
    lib = pkg._lib.lib()
    nq, T = gate.shape
    g, m = gate.cuda().contiguous(), mask.to(torch.uint8).cuda().contiguous()
    clips = torch.full((T,), -7, dtype=i32, device='cuda')
    pos = torch.full((T,), -7, dtype=i32, device='cuda')
    count = torch.full((1,), -7, dtype=i32, device='cuda')
    p = pkg._lib.ptr
    pkg._lib.check(lib.dcf_op_select_clips(p(g), p(m), T, nq, p(clips), p(pos), p(count), pkg._lib.current_stream()), 'dcf_op_select_clips')
    return clips.cpu(), pos.cpu(), int(count.item())


def check_select(pkg, gate, mask):
    want_clips, want_pos, n = S.select_clips(gate, mask)
    clips, pos, count = run_select(pkg, gate, mask)
    assert count == n and torch.equal(clips[:n], want_clips) and torch.equal(pos, want_pos)
    assert bool((clips[n:] == -7).all()), 'an entry at or beyond count was written'
    return n


def test_select_clips_random_block_gates_across_strips():
    """T = 5000 is no multiple of the 4096-clip strip (nor of a 1024-clip sub-strip): the carry and a partly filled strip"""
    pkg = load_pkg()
    T, nq = 5000, 3
    gate = block_gate(torch.Generator().manual_seed(5), nq, T, T, 60, 25)
    only0 = (gate[0] != 0) & (gate[1] == 0)
    assert bool(only0.any()), 'a clip that query 0 keeps and query 1 does not'
    n = check_select(pkg, gate, torch.ones(T, dtype=torch.bool))
    assert int((gate != 0).any(0).sum()) == n and 0 < n < T
    hole = torch.ones(T, dtype=torch.bool)
    hole[4090:4100] = False                                   # invalid clips under open gates, across the strip seam
    gate[:, 4080:4110] = 1
    assert check_select(pkg, gate, hole) < T


def test_select_clips_one_clip():
    pkg = load_pkg()
    assert check_select(pkg, torch.ones(1, 1), torch.ones(1, dtype=torch.bool)) == 1
    assert check_select(pkg, torch.ones(2, 1), torch.zeros(1, dtype=torch.bool)) == 0


@pytest.mark.parametrize('T,vid_len,sn,nq', [(16, 16, 8, 2), (64, 40, 8, 2)])
def test_select_clips_on_the_gate_kernel_s_output(T, vid_len, sn, nq):
    """the gate as dcf_op_gate writes it: int(0.3 * 2) = 0 keeps every block (T = 16), and with vid_len < T no padded clip is listed"""
    pkg = load_pkg()
    lib, p = pkg._lib.lib(), pkg._lib.ptr
    correl = torch.randn(nq, T, generator=torch.Generator().manual_seed(T)).cuda()
    mask = (torch.arange(T) < vid_len).cuda()
    gate = torch.empty(nq, T, device='cuda')
    mo = torch.empty(nq, T, dtype=torch.bool, device='cuda')
    pkg._lib.check(lib.dcf_op_gate(p(correl), p(mask), p(gate), p(mo), T, nq, sn, 0.3, 1, pkg._lib.current_stream()), 'dcf_op_gate')
    n = check_select(pkg, gate.cpu(), mask.cpu())
    clips, pos, _ = run_select(pkg, gate.cpu(), mask.cpu())
    if T == 16:
        assert n == T and clips.tolist() == list(range(T))
    else:
        assert 0 < n < vid_len and int(clips[:n].max()) < vid_len and bool((pos[vid_len:] == -1).all())


# ---------------------------------------------------------------------------------------------- dcf_op_gather_clip_rows
@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
@pytest.mark.parametrize('D,T,n', [(64, 300, 70), (100, 300, 131), (100, 77, 1)])
def test_gather_clip_rows_equals_indexing(D, T, n, dtype):
    pkg = load_pkg()
    lib, p = pkg._lib.lib(), pkg._lib.ptr
    g = torch.Generator().manual_seed(D + T + n)
    x = torch.randn(D, T, generator=g).to(dtype)
    clips = torch.randperm(T, generator=g)[:n].sort().values.to(i32)
    assert n % 4 != 0
    xd, cd = x.cuda(), clips.cuda()
    rows = torch.full((n, D), float('nan'), dtype=dtype, device='cuda')
    fn = lib.dcf_op_gather_clip_rows_h if dtype == torch.float16 else lib.dcf_op_gather_clip_rows
    pkg._lib.check(fn(p(xd), T, p(cd), n, D, p(rows), pkg._lib.current_stream()), 'dcf_op_gather_clip_rows')
    assert torch.equal(rows.cpu(), S.gather_clip_rows(x, clips))


# ---------------------------------------------------------------------------------------------- the four fixtures
@pytest.fixture(scope='module')
def fixture_runs():
    """per fixture: (case, model, texts, tmasks, selection, the result of forward_selected on rows gathered from the fixture's vid)"""
    pkg = load_pkg()
    runs = {}

    def get(name):
        if name not in runs:
            c = P.e2e_case(name)
            opt, model, sd = build(pkg, c.kw, c.g.js('shapes'), c.meta['wseed'])
            texts, tmasks = encode(model, c.inp['tokens'])
            vid, sh, vm = c.inp['vid'].cuda(), c.inp['shallow_vid'].cuda(), c.inp['vid_masks'].cuda()
            sel = model.select_clips(sh, vm, c.inp['text_cls'].cuda())
            rows = model.gather_clip_rows(vid, sel)
            out = model.forward_selected(rows, sel, sh, vm, texts, tmasks)
            runs[name] = (c, model, texts, tmasks, sel, rows, out, flat(out))
        return runs[name]
    return get


@pytest.mark.parametrize('name', S.FIXTURES)
def test_select_clips_gates_equal_the_oracle_s(fixture_runs, name):
    c, model, texts, tmasks, sel, rows, out, bits = fixture_runs(name)
    want = S.oracle_gates(c.opt.model, c.inp['shallow_vid'], c.inp['vid_masks'], c.inp['text_cls'])
    assert min(S.gate_gaps(c.opt.model, c.inp['shallow_vid'], c.inp['vid_masks'], c.inp['text_cls'])) > S.GAP_MIN
    assert torch.equal(sel.gate.cpu(), want)
    clips, pos, n = S.select_clips(want, c.inp['vid_masks'][0])
    assert sel.count == n and torch.equal(sel.clips.cpu(), clips) and torch.equal(sel.pos.cpu(), pos)
    assert torch.equal(sel.clips_host(), clips.long()) and sel.clips.dtype == i32 and sel.clips.is_cuda
    assert torch.equal(rows.cpu(), S.gather_clip_rows(c.inp['vid'][0], clips))


@pytest.mark.parametrize('name', S.FIXTURES)
def test_forward_selected_matches_reference_fixture(fixture_runs, name):
    c, model, texts, tmasks, sel, rows, (lg, of, mk), bits = fixture_runs(name)
    assert len(lg) == len(of) == len(mk) == c.nq
    for q in range(c.nq):
        for l in range(c.L):
            assert torch.equal(mk[q][l].cpu(), c.masks[q][l]), (q, l)
            assert lg[q][l].shape == c.y32['logits'][q][l].shape and of[q][l].shape == c.y32['offsets'][q][l].shape
    for kind, got in (('logits', lg), ('offsets', of)):
        P.check(f'selected e2e_{name} {kind}', P.pool(got), P.pool(c.y64[kind]), P.pool(c.y32[kind]))
    assert model.numerics_status() & 1 == 0 and model.graph_active() == 0
    vid, sh, vm = c.inp['vid'].cuda(), c.inp['shallow_vid'].cuda(), c.inp['vid_masks'].cuda()
    dense = model.forward_window(vid, sh, vm, texts, tmasks, sel.gate)
    for kind, a, b in (('logits', lg, dense[0]), ('offsets', of, dense[1])):
        print(f'SELDIFF e2e_{name} {kind}: max |selected - gated dense| = {float((P.pool(a) - P.pool(b)).abs().max()):.3e}, '
              f'max |y| = {float(P.pool(b).abs().max()):.3e}')
    assert all(torch.equal(a.cpu(), b.cpu()) for qa, qb in zip(mk, dense[2]) for a, b in zip(qa, qb))


# ---------------------------------------------------------------------------------------------- the probe-width model
PROBE = dict(D=256, E=128, TE=64, text_in=32, n_levels=4, win=5, n_heads=4, sn=60, sratio=0.3, msf=True, norm=True, max_seq_len=128,
             text_layers=1, text_max_len=24)


@pytest.fixture(scope='module')
def probe():
    """the model of test_expert_product_under_the_gate_is_bit_identical (the split-operand row-major GEMM runs: D = 256, E = 128, f16x3),
    T = 2048, vid_len = 1500, two queries"""
    pkg = load_pkg()
    opt, model, sd = build(pkg, PROBE, None, 37)
    inp = pkg.synth.make_inputs(256, 2048, 1500, 2, 32, 6, 902)      # (an input seed whose top-k choices the oracle decides by > 1e-3)
    texts, tmasks = encode(model, inp['tokens'])
    dev = {k: inp[k].cuda() for k in ('vid', 'shallow_vid', 'vid_masks', 'text_cls')}
    return pkg, opt, model, sd, inp, dev, texts, tmasks


def test_forward_selected_probe_width_against_the_oracle(probe):
    pkg, opt, model, sd, inp, dev, texts, tmasks = probe
    assert min(S.gate_gaps(opt.model, inp['shallow_vid'], inp['vid_masks'], inp['text_cls'])) > S.GAP_MIN
    sel = model.select_clips(dev['shallow_vid'], dev['vid_masks'], dev['text_cls'])
    assert torch.equal(sel.gate.cpu(), S.oracle_gates(opt.model, inp['shallow_vid'], inp['vid_masks'], inp['text_cls']))
    assert 0 < sel.count < 1500 and int(sel.clips_host().max()) < 1500
    rows = model.gather_clip_rows(dev['vid'], sel)
    lg, of, mk = model.forward_selected(rows, sel, dev['shallow_vid'], dev['vid_masks'], texts, tmasks)
    args = (inp['vid'], inp['shallow_vid'], inp['vid_masks'], [t.cpu() for t in texts], inp['text_cls'], [m.cpu() for m in tmasks])
    with torch.no_grad():
        y32 = R.forward_eval(sd, opt.model, *args)
    y64 = P.oracle64.forward_eval(sd, opt.model, *args)
    for q in range(2):
        for l in range(4):
            assert torch.equal(y32[2][q][l], y64[2][q][l]) and torch.equal(mk[q][l].cpu(), y32[2][q][l])
    P.check('selected probe logits', P.pool(lg), P.pool(y64[0]), P.pool(y32[0]))
    P.check('selected probe offsets', P.pool(of), P.pool(y64[1]), P.pool(y32[1]))
    assert model.numerics_status() & 1 == 0
    dense = model.forward_window(dev['vid'], dev['shallow_vid'], dev['vid_masks'], texts, tmasks, sel.gate)
    for kind, a, b in (('logits', lg, dense[0]), ('offsets', of, dense[1])):
        print(f'SELDIFF probe {kind}: max |selected - gated dense| = {float((P.pool(a) - P.pool(b)).abs().max()):.3e}, '
              f'max |y| = {float(P.pool(b).abs().max()):.3e}')


def test_determinism_capacity_rows_and_back_to_back_selections(probe):
    """two calls give equal bits; NaN in the capacity rows beyond count changes nothing; two selections of different count, run back
    to back on the same row and output buffers with graphs asked for, each give what their own single run gave (this forward never
    replays a graph: dcf_graph_active() == 0)"""
    pkg, opt, model, sd, inp, dev, texts, tmasks = probe
    sh, vm, cls = dev['shallow_vid'], dev['vid_masks'], dev['text_cls']
    sel_a = model.select_clips(sh, vm, cls)                               # the union of two queries
    sel_b = model.select_clips(sh, vm, cls[:1].repeat(2, 1))              # the first query twice: its own clips only
    assert sel_b.count < sel_a.count
    tex_b, tm_b = (texts[0], texts[0]), (tmasks[0], tmasks[0])
    cap = torch.full((2048, 256), float('nan'), device='cuda')
    model.graph_mode, model.reuse_output_buffers = 'always', True
    try:
        def run(sel, tx, tm):
            cap.fill_(float('nan'))
            cap[:sel.count] = model.gather_clip_rows(dev['vid'], sel)
            out = flat(model.forward_selected(cap, sel, sh, vm, tx, tm))
            assert model.graph_active() == 0
            return out
        one_a = run(sel_a, texts, tmasks)
        assert same_bits(one_a, flat(model.forward_selected(model.gather_clip_rows(dev['vid'], sel_a), sel_a, sh, vm, texts, tmasks)))
        assert all(bool(torch.isfinite(x).all()) for x in one_a if x.is_floating_point())
        one_b = run(sel_b, tex_b, tm_b)
        assert not same_bits(one_a, one_b)
        for _ in range(2):
            assert same_bits(run(sel_a, texts, tmasks), one_a)
            assert same_bits(run(sel_b, tex_b, tm_b), one_b)
    finally:
        model.graph_mode, model.reuse_output_buffers = 'auto', False
    assert model.numerics_status() & 1 == 0


def test_half_rows_give_what_fp32_rows_of_the_same_values_give(probe):
    pkg, opt, model, sd, inp, dev, texts, tmasks = probe
    sh16, vid16 = dev['shallow_vid'].half(), dev['vid'].half()
    sel = model.select_clips(sh16, dev['vid_masks'], dev['text_cls'])
    sel32 = model.select_clips(sh16.float(), dev['vid_masks'], dev['text_cls'])
    assert torch.equal(sel.gate, sel32.gate) and torch.equal(sel.pos, sel32.pos) and sel.count == sel32.count
    rows16 = model.gather_clip_rows(vid16, sel)
    assert rows16.dtype == torch.float16 and torch.equal(rows16.cpu(), S.gather_clip_rows(vid16[0].cpu(), sel.clips_host()))
    got = flat(model.forward_selected(rows16, sel, sh16, dev['vid_masks'], texts, tmasks))
    assert model.last_feature_dtype == torch.float16
    want = flat(model.forward_selected(rows16.float(), sel, sh16.float(), dev['vid_masks'], texts, tmasks))
    assert model.last_feature_dtype == torch.float32
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and len(got) == len(want)          # equal as numbers
    with pytest.raises(ValueError, match='float16'):
        model.forward_selected(rows16, sel, sh16.float(), dev['vid_masks'], texts, tmasks)


def test_non_finite_rows_raise_the_numerics_flag(probe):
    pkg, opt, model, sd, inp, dev, texts, tmasks = probe
    sel = model.select_clips(dev['shallow_vid'], dev['vid_masks'], dev['text_cls'])
    rows = model.gather_clip_rows(dev['vid'], sel)
    rows[sel.count // 2, 7] = float('inf')
    model.numerics_status(reset=True)
    lg, _, _ = model.forward_selected(rows, sel, dev['shallow_vid'], dev['vid_masks'], texts, tmasks)
    torch.cuda.synchronize()
    assert model.numerics_status(reset=True) & 1 == 1
    assert bool(torch.isnan(P.pool(lg)).all())
    model.acknowledge_ln_carry()                                          # (disarms the pending probe of this forward for the next test)
    model.set_ln_carry(True)


# ---------------------------------------------------------------------------------------------- refusals
TINY = dict(D=64, E=64, TE=32, text_in=32, n_levels=4, win=5, n_heads=4, sn=8, sratio=0.3, msf=True, norm=True, max_seq_len=128,
            text_layers=1, text_max_len=24, max_vid_len=128)


@pytest.mark.parametrize('over,word', [(dict(scat=True), 'scat'), (dict(sfonly=True), 'sfonly'), (dict(vid_stride=2), 'stride')])
def test_refusals_before_a_launch(over, word):
    """by the host layer, and by the C entry point itself (rc -1 and a message; the outputs keep their bits)"""
    pkg = load_pkg()
    lib, p = pkg._lib.lib(), pkg._lib.ptr
    opt, model, sd = build(pkg, dict(TINY, **over), None, 11)
    Dm = model.D                                                          # (sfonly: the feature files are 2 D wide, model.py:546-547)
    inp = pkg.synth.make_inputs(Dm, 128, 100, 1, 32, 5, 12)
    texts, tmasks = encode(model, inp['tokens'])
    vid, sh, vm, cls = (inp[k].cuda() for k in ('vid', 'shallow_vid', 'vid_masks', 'text_cls'))
    with pytest.raises(NotImplementedError, match=word):
        model.select_clips(sh, vm, cls)
    with pytest.raises(NotImplementedError, match=word):
        model.forward_selected(torch.zeros(30, Dm, device='cuda'), None, sh, vm, texts, tmasks)
    model(vid, sh, vm, texts, cls, tmasks, eval=True)                     # binds the engine
    torch.cuda.synchronize()
    S_pts = lib.dcf_points_per_query(model._engine.handle, 128)
    gate, mask = torch.ones(1, 128), torch.arange(128) < 100
    clips, pos, n = S.select_clips(gate, mask)
    rows = torch.zeros(n, Dm, device='cuda')
    gd, pd, md = gate.cuda(), pos.cuda(), mask.cuda()
    logits, offsets = torch.full((1, S_pts), -3.0, device='cuda'), torch.full((1, S_pts, 2), -3.0, device='cuda')
    masks = torch.zeros(1, S_pts, dtype=torch.bool, device='cuda')
    t, m = texts[0][0].contiguous().float(), tmasks[0].reshape(-1).contiguous()
    tptr, mptr, tlen = (ctypes.c_void_p * 1)(t.data_ptr()), (ctypes.c_void_p * 1)(m.data_ptr()), (ctypes.c_int32 * 1)(t.size(1))
    rc = lib.dcf_forward_eval_selected(model._engine.handle, p(rows), n, p(pd), p(sh[0].contiguous()), p(md), 128, 1, tptr, mptr, tlen, p(gd),
                                       p(logits), p(offsets), p(masks), pkg._lib.current_stream())
    torch.cuda.synchronize()
    assert rc == -1 and word in lib.dcf_last_error().decode()
    assert bool((logits == -3.0).all()) and bool((offsets == -3.0).all())


def test_refusals_of_rows_and_counts(probe):
    pkg, opt, model, sd, inp, dev, texts, tmasks = probe
    lib, p = pkg._lib.lib(), pkg._lib.ptr
    sh, vm = dev['shallow_vid'], dev['vid_masks']
    sel = model.select_clips(sh, vm, dev['text_cls'])
    with pytest.raises(ValueError, match='vid_rows'):
        model.forward_selected(torch.zeros(sel.count, 260, device='cuda'), sel, sh, vm, texts, tmasks)       # count rows of the wrong width
    with pytest.raises(ValueError, match='vid_rows'):
        model.forward_selected(torch.zeros(sel.count - 1, 256, device='cuda'), sel, sh, vm, texts, tmasks)
    with pytest.raises(ValueError, match='selection'):
        model.forward_selected(torch.zeros(sel.count, 256, device='cuda'), sel, sh, vm, texts[:1], tmasks[:1])
    model.forward_selected(model.gather_clip_rows(dev['vid'], sel), sel, sh, vm, texts, tmasks)           # binds the engine
    h = model._engine.handle
    S_pts = lib.dcf_points_per_query(h, 2048)
    logits, offsets = torch.full((2, S_pts), -3.0, device='cuda'), torch.full((2, S_pts, 2), -3.0, device='cuda')
    masks = torch.zeros(2, S_pts, dtype=torch.bool, device='cuda')
    keep = [(texts[q][0].contiguous().float(), tmasks[q].reshape(-1).contiguous()) for q in range(2)]
    tptr, mptr = (ctypes.c_void_p * 2)(*[t.data_ptr() for t, _ in keep]), (ctypes.c_void_p * 2)(*[m.data_ptr() for _, m in keep])
    tlen = (ctypes.c_int32 * 2)(*[t.size(1) for t, _ in keep])
    rows = torch.zeros(2049, 256, device='cuda')
    for n_rows in (0, -1, 2049):
        rc = lib.dcf_forward_eval_selected(h, p(rows), n_rows, p(sel.pos), p(sh[0].contiguous()), p(vm.reshape(-1).contiguous()), 2048, 2, tptr, mptr,
                                           tlen, p(sel.gate), p(logits), p(offsets), p(masks), pkg._lib.current_stream())
        torch.cuda.synchronize()
        assert rc == -1 and 'n_rows' in lib.dcf_last_error().decode()
    assert bool((logits == -3.0).all())


# ---------------------------------------------------------------------------------------------- the evaluator
def test_evaluator_selected_expert():
    """expert_fn is called once per window with exactly select_clips' ascending indices, none at or beyond vid_len; with the true rows
    the window's logits pass the parity rule against the oracle; expert_fn=None gives the same bits; the default evaluator's outputs
    are what they were before and after"""
    pkg = load_pkg()
    opt, model, sd = build(pkg, TINY, None, 21)
    g = torch.Generator().manual_seed(6)
    samples = []
    for vid_len in (100, 128, 300):                           # padded lengths 128, 128, 320
        nq = 1 + vid_len % 3
        samples.append(dict(vid=torch.randn(64, vid_len, generator=g), shallow_vid=torch.randn(64, vid_len, generator=g),
                            text=tuple(torch.randn(32, 6, generator=g) for _ in range(nq)), text_cls=torch.randn(nq, 64, generator=g),
                            segment=torch.rand(nq, 2, generator=g).sort(1).values * vid_len * 16 / 30.0,
                            fps=30.0, clip_stride=16, clip_size=32, duration=vid_len * 16 / 30.0 + 2, clip_id=f'v{vid_len}'))
    ev = pkg.evaluator
    dense = ev.GroundingEvaluator(opt, model)
    assert dense.expert == 'dense'
    before = [[x.cpu().clone() for x in dense.forward(s)[0]] for s in samples]
    calls = []

    def expert_fn(sample, clips):
        calls.append((sample['clip_id'], clips.clone()))
        assert clips.dtype == torch.int64 and not clips.is_cuda
        return sample['vid'][:, clips].t().contiguous()

    sel_fn = ev.GroundingEvaluator(opt, model, expert='selected', expert_fn=expert_fn)
    sel_gather = ev.GroundingEvaluator(opt, model, expert='selected')
    for i, s in enumerate(samples):
        vid_len = s['vid'].size(-1)
        args, T, _ = dense.prepare(s)
        window, shallow_w, mask, texts, text_cls, tmasks = args
        cfg = opt.model
        assert min(S.gate_gaps(cfg, shallow_w.cpu(), mask.cpu(), text_cls.cpu())) > S.GAP_MIN
        want_sel = model.select_clips(shallow_w, mask, text_cls)
        n_before = len(calls)
        (logits, offsets, masks), T2 = sel_fn.forward(s)
        got = [x.cpu().clone() for x in (logits, offsets, masks)]
        assert T2 == T and len(calls) == n_before + 1 and calls[-1][0] == s['clip_id']
        clips = calls[-1][1]
        assert torch.equal(clips, want_sel.clips_host()) and bool((clips[1:] > clips[:-1]).all()) and int(clips.max()) < vid_len
        assert sel_fn.last_selection.count == clips.numel()
        again = [x.cpu().clone() for x in sel_gather.forward(s)[0]]
        assert len(calls) == n_before + 1 and same_bits(got, again)
        nq, L = len(texts), TINY['n_levels']
        sizes = [T >> l for l in range(L)]
        lg = [[x[None] for x in got[0][q].split(sizes)] for q in range(nq)]
        ocpu = (window.cpu(), shallow_w.cpu(), mask.cpu(), [t.cpu() for t in texts], text_cls.cpu(), [m.cpu() for m in tmasks])
        with torch.no_grad():
            y32 = R.forward_eval(sd, cfg, *ocpu)
        y64 = P.oracle64.forward_eval(sd, cfg, *ocpu)
        for q in range(nq):
            off = 0
            for l in range(L):
                assert torch.equal(got[2][q][off:off + sizes[l]][None], y32[2][q][l])
                off += sizes[l]
        P.check(f'evaluator selected {s["clip_id"]} logits', P.pool(lg), P.pool(y64[0]), P.pool(y32[0]))
    # a sample without dense expert features runs where the rows come from expert_fn
    vids = {s['clip_id']: s['vid'] for s in samples}
    lean = ev.GroundingEvaluator(opt, model, expert='selected', expert_fn=lambda sample, clips: vids[sample['clip_id']][:, clips].t().contiguous())
    s0 = {k: v for k, v in samples[0].items() if k != 'vid'}
    res = lean.predict(s0)
    assert len(res) == len(samples[0]['text'])
    after = [[x.cpu().clone() for x in dense.forward(s)[0]] for s in samples]
    assert all(same_bits(a, b) for a, b in zip(before, after))
    assert model.numerics_status() & 1 == 0
