"""Clip features in IEEE binary16 (include/decafnet_hip_half.h): the kernels that read half values return what the fp32 kernels return
on the same values upcast -- ``torch.equal``, no tolerance (zeros of either sign compare equal; that is intended) -- from the two
operators up to the evaluator; the native path is asserted to have run (dcf_debug_set_option('half_native', 2): native or an error);
one native case against the fp64 oracle under the rule of tests/forward_parity.py; a non-finite half feature raises the status word.
GPU only."""
import ctypes
import math

import pytest
import torch

from conftest import load_pkg
import forward_parity as FP
from forward_parity import R

pytestmark = pytest.mark.gpu


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope='module')
def ctx():
    pkg = load_pkg()
    return pkg, pkg._lib.lib()


def option(pkg, lib, name, value):
    pkg._lib.check(lib.dcf_debug_set_option(name.encode(), value), name)


# ---------------------------------------------------------------------------------------------- operators
def _operand(kind, K, M, g):
    """(K, M) channel-major, binary16"""
    a = torch.randn(K, M, generator=g)
    if kind == 'subnormal':
        a = a * 2.0 ** -17                              # most entries below the smallest normal half 2^-14
    elif kind == 'zero-column':
        a[K // 2] = 0.0                                 # one k of every row of A[m][k]
        a[:, 1] = 0.0                                   # and one row m
    elif kind == 'to-4000':
        a = a * (4000.0 / float(a.abs().max()))
    h = a.half()
    if kind == 'subnormal':
        assert int(((h != 0) & (h.float().abs() < 2.0 ** -14)).sum()) > h.numel() // 2
    return h


@pytest.mark.parametrize('nterms', [16, 6])
@pytest.mark.parametrize('M,N,K', [(4, 128, 32), (68, 128, 64), (192, 256, 96)])
def test_linear_cm_split_h_equals_the_fp32_operator_on_the_upcast_operand(ctx, M, N, K, nterms):
    """The shapes of the issue with lda = M: one quarter-filled row group, a partial second 64-row tile, three tiles x two column
    tiles.  lda > M: the next test."""
    pkg, lib = ctx
    g = torch.Generator().manual_seed(1000 * M + K + nterms)
    W = (torch.randn(N, K, generator=g) / math.sqrt(K)).cuda()
    bias = torch.randn(N, generator=g).cuda()
    for kind in ('normal', 'subnormal', 'zero-column', 'to-4000'):
        h = _operand(kind, K, M, g).cuda()
        f = h.float()
        got, want = torch.full((M, N), float('nan'), device='cuda'), torch.full((M, N), float('nan'), device='cuda')
        pkg._lib.check(lib.dcf_op_linear_cm_split(p(f), p(W), p(bias), p(want), M, N, K, nterms, None), 'dcf_op_linear_cm_split')
        pkg._lib.check(lib.dcf_op_linear_cm_split_h(p(h), p(W), p(bias), p(got), M, N, K, nterms, 0, None), 'dcf_op_linear_cm_split_h')
        torch.cuda.synchronize()
        assert bool(torch.isfinite(want).all()), kind
        assert torch.equal(got, want), (kind, float((got - want).abs().max()))
        ref = f.double().t() @ W.double().t() + bias.double()
        assert float((want.double() - ref).abs().max()) <= 2.0 ** -18 * max(float(ref.abs().max()), 1.0), kind      # and it IS the product
        # the engine's unscaled planes: the same numbers as long as nothing leaves the range (to-4000 overflows scale 2^4 nowhere)
        un = torch.full((M, N), float('nan'), device='cuda')
        pkg._lib.check(lib.dcf_op_linear_cm_split_h(p(h), p(W), p(bias), p(un), M, N, K, nterms, 1, None), 'dcf_op_linear_cm_split_h')
        torch.cuda.synchronize()
        assert float((un.double() - ref).abs().max()) <= 2.0 ** -18 * max(float(ref.abs().max()), 1.0), kind


@pytest.mark.parametrize('nterms', [16, 6])
@pytest.mark.parametrize('M,lda,N,K,col0', [(68, 200, 128, 64, 0), (68, 200, 128, 64, 132), (132, 136, 256, 96, 4), (4, 1028, 128, 32, 1024)])
def test_linear_cm_split_ld_h_with_a_row_pitch_above_m(ctx, M, lda, N, K, col0, nterms):
    """lda > M: a window of M clips, starting at clip col0, of a (K, lda) half matrix through dcf_op_linear_cm_split_ld_h, against
    dcf_op_linear_cm_split on the same sub-matrix upcast and made contiguous.  What lies beside the window in every row is NaN: a
    loader that stepped by M instead of lda, or read past its M columns into a value it keeps, would show.  (68, 200): a partial
    second tile, window at the start and at the end of the rows; (132, 136): a pitch just above M; (4, 1028): one row group, a
    pitch far above the tile."""
    pkg, lib = ctx
    assert lda > M and lda % 4 == 0 and col0 % 4 == 0 and col0 + M <= lda
    g = torch.Generator().manual_seed(31 * M + lda + nterms)
    W = (torch.randn(N, K, generator=g) / math.sqrt(K)).cuda()
    bias = torch.randn(N, generator=g).cuda()
    for kind in ('normal', 'subnormal', 'to-4000'):
        full = torch.full((K, lda), float('nan'), dtype=torch.float16)
        full[:, col0:col0 + M] = _operand(kind, K, M, g)
        full = full.cuda()
        window = full[:, col0:]                           # its address: 8-byte aligned (col0 % 4 == 0), pitch lda
        assert window.data_ptr() % 8 == 0 and window.stride(0) == lda
        f = full[:, col0:col0 + M].float().contiguous()
        got, want = torch.full((M, N), float('nan'), device='cuda'), torch.full((M, N), float('nan'), device='cuda')
        pkg._lib.check(lib.dcf_op_linear_cm_split(p(f), p(W), p(bias), p(want), M, N, K, nterms, None), 'dcf_op_linear_cm_split')
        pkg._lib.check(lib.dcf_op_linear_cm_split_ld_h(p(window), lda, p(W), p(bias), p(got), M, N, K, nterms, 0, None), 'dcf_op_linear_cm_split_ld_h')
        torch.cuda.synchronize()
        assert bool(torch.isfinite(want).all()), kind
        assert torch.equal(got, want), (kind, float((got - want).abs().max()))


def test_linear_cm_split_h_on_a_misaligned_operand_is_refused(ctx):
    pkg, lib = ctx
    M, N, K = 8, 128, 32
    buf = torch.zeros(K * M + 4, dtype=torch.float16, device='cuda')
    W, C = torch.zeros(N, K, device='cuda'), torch.zeros(M, N, device='cuda')
    for off in (1, 2, 3):
        rc = lib.dcf_op_linear_cm_split_h(p(buf[off:]), p(W), None, p(C), M, N, K, 16, 0, None)
        assert rc == -1 and '8-byte aligned' in lib.dcf_last_error().decode()
    assert lib.dcf_op_linear_cm_split_h(p(buf[4:]), p(W), None, p(C), M, N, K, 16, 0, None) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize('T', [68, 67])
@pytest.mark.parametrize('nq', [1, 4])
@pytest.mark.parametrize('norm', [1, 0])
def test_sidekick_h_equals_the_fp32_operator(ctx, norm, nq, T):
    """D = 64, T = 68 (8-byte loads, a partial last wave) and T = 67 (the clip-by-clip loads)"""
    pkg, lib = ctx
    D = 64
    g = torch.Generator().manual_seed(7 + T + nq)
    h = torch.randn(D, T, generator=g).half().cuda()
    cls = torch.randn(nq, D, generator=g).cuda()
    got, want = torch.full((nq, T), float('nan'), device='cuda'), torch.full((nq, T), float('nan'), device='cuda')
    f = h.float()
    pkg._lib.check(lib.dcf_op_sidekick(p(f), p(cls), p(want), D, T, nq, norm, None), 'dcf_op_sidekick')
    pkg._lib.check(lib.dcf_op_sidekick_h(p(h), p(cls), p(got), D, T, nq, norm, None), 'dcf_op_sidekick_h')
    torch.cuda.synchronize()
    assert bool(torch.isfinite(want).all()) and torch.equal(got, want)


# ---------------------------------------------------------------------------------------------- engine
T_ENGINE = 512                 # eight 64-clip tiles; a multiple of the chunk size 2^3 * 4 of the four-level, win-5 models below
BASE = dict(D=64, TE=32, text_in=32, n_levels=4, win=5, n_heads=4, sn=64, sratio=0.3, msf=True, norm=True, max_seq_len=128, text_layers=1,
            text_max_len=24)


def build(pkg, kw, wseed, gemm_mode=None):
    opt = pkg.config.make_opt(**kw)
    if gemm_mode:
        opt.model['gemm_mode'] = gemm_mode
    model = pkg.modeling.create_model(opt)
    sd = pkg.synth.make_state_dict({k: list(v.shape) for k, v in model.state_dict().items()}, wseed)
    model.load_state_dict(sd)
    return opt, model.cuda().eval().requires_grad_(False), sd


def make_videos(pkg, model, feat_dim, lens_nq, seed, T=T_ENGINE):
    """the argument tuples of forward per video, vid / shallow_vid rounded to binary16 (on the device, as float16 tensors)"""
    videos, cpu = [], []
    for v, (vid_len, nq) in enumerate(lens_nq):
        inp = pkg.synth.make_inputs(feat_dim, T, vid_len, nq, 32, 5 + v, seed + v)
        tm = [model.encode_text(t[None].cuda(), torch.ones(1, 1, t.size(-1), dtype=torch.bool, device='cuda')) for t in inp['tokens']]
        videos.append((inp['vid'].half().cuda(), inp['shallow_vid'].half().cuda(), inp['vid_masks'].cuda(), tuple(t for t, _ in tm),
                       inp['text_cls'].cuda(), tuple(m for _, m in tm)))
        cpu.append(inp)
    return videos, cpu


def flat(out):
    """every tensor of a forward's (or forward_videos') result, cloned"""
    res = []

    def walk(x):
        if isinstance(x, torch.Tensor):
            res.append(x.clone())
        else:
            for y in x:
                walk(y)
    walk(out)
    return res


def same(a, b, what):
    assert len(a) == len(b) and len(a) > 0
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), (what, i)


def gate_tap(pkg, lib, model, nq, T):
    gate = torch.empty(nq, T, device='cuda')
    pkg._lib.check(lib.dcf_debug_copy(model._engine.handle, 1, p(gate), gate.numel(), None), 'dcf_debug_copy')
    torch.cuda.synchronize()
    return gate.cpu()


def both_ways(pkg, lib, model, run, native=True):
    """run() with the half entry points (natively, or an error) and with half_features = False on the same tensors"""
    option(pkg, lib, 'half_native', 2 if native else 1)
    try:
        model.half_features = True
        got = flat(run())
        assert model.last_feature_dtype is torch.float16
    finally:
        option(pkg, lib, 'half_native', -1)
    model.half_features = False
    try:
        want = flat(run())
        assert model.last_feature_dtype is torch.float32
    finally:
        model.half_features = True
    return got, want


@pytest.mark.parametrize('E', [128, 256])
@pytest.mark.parametrize('variant', ['msf', 'nomsf', 'scat', 'sfonly'])
def test_half_forward_equals_the_upcast_forward(ctx, variant, E):
    """two videos with 2 + 1 queries in one forward -- E = 256: the expert halves in the one-grid launch; E = 128: through flush() --,
    three videos (2 + 1 + 1: a three-operand grid), and each video alone; fused scores and the scoring kernels; sn = 64 and
    sratio = 0.3 keep int(0.3 * 8) = 2 of a full video's eight 64-clip tiles per query, so most row tiles of the expert product are
    skipped -- asserted from the gate tap"""
    pkg, lib = ctx
    kw = dict(BASE, E=E, msf=variant != 'nomsf' and variant != 'scat', scat=variant == 'scat', sfonly=variant == 'sfonly')
    opt, model, sd = build(pkg, kw, 41)
    feat = model.D
    lens_nq = [(T_ENGINE, 2), (400, 1), (T_ENGINE, 1)]
    videos, _ = make_videos(pkg, model, feat, lens_nq, 1200)
    for fuse in (1, 0):
        option(pkg, lib, 'fuse_scores', fuse)
        try:
            for group in (videos[:2], videos):
                got, want = both_ways(pkg, lib, model, lambda: model.forward_videos(group))
                same(got, want, (variant, E, fuse, len(group)))
                # the skip is under test: at least one 64-clip tile of a video is kept by none of its queries
                nq_all = sum(len(a[3]) for a in group)
                gate = gate_tap(pkg, lib, model, nq_all, T_ENGINE)
                kept = gate.view(nq_all, T_ENGINE // 64, 64).amax(2)
                q0, open_tiles = 0, []
                for a in group:
                    open_tiles.append(int((kept[q0:q0 + len(a[3])].amax(0) == 0).sum()))
                    q0 += len(a[3])
                assert min(open_tiles) >= 1, open_tiles
            got, want = both_ways(pkg, lib, model, lambda: [model(*a, eval=True) for a in videos])
            same(got, want, (variant, E, fuse, 'single'))
        finally:
            option(pkg, lib, 'fuse_scores', -1)
    assert model.numerics_status() & 1 == 0


def test_half_forward_under_graph_replay(ctx):
    """graph mode on: eager, capture, replay -- each equal to the upcast forward; a replay after the features changed in place follows
    them; an fp32 forward in between does not reuse the half graph"""
    pkg, lib = ctx
    opt, model, sd = build(pkg, dict(BASE, E=256), 42)
    model.graph_mode = 'always'
    model.reuse_output_buffers = True
    videos, _ = make_videos(pkg, model, 64, [(T_ENGINE, 2), (300, 1)], 1300)
    model.half_features = False
    want = flat(model.forward_videos(videos))
    model.half_features = True
    option(pkg, lib, 'half_native', 2)
    try:
        seen = []
        for rep in range(3):
            same(flat(model.forward_videos(videos)), want, ('graph', rep))
            seen.append(model.graph_active())
        assert seen == [0, 2, 1], seen
        videos[1][0].mul_(0.5)                           # exact in binary16 (no subnormal operand here): the replay must read the new bits
        same_ptr = flat(model.forward_videos(videos))
        assert model.graph_active() == 1
        model.half_features = False
        want2 = flat(model.forward_videos(videos))
        assert model.graph_active() == 0 and model.last_feature_dtype is torch.float32
        same(same_ptr, want2, 'replay after an in-place change')
        assert any(not torch.equal(a, b) for a, b in zip(want2, want)), 'halving the features of video 1 changed nothing'
    finally:
        option(pkg, lib, 'half_native', -1)
        model.half_features = True


def test_half_forward_falls_back_where_the_native_path_does_not_apply(ctx):
    """E % 128 != 0 (the e2e configuration of tests/test_gpu_e2e.py test_forward_videos_equals_single_video_forwards, E = 64) and
    gemm_mode = 'fp32': the features are upcast once on the device; with half_native = 2 the same call is an error, which is how the
    tests above know that their forwards ran natively"""
    pkg, lib = ctx
    for kw, mode in ((dict(BASE, E=64, sn=8), None), (dict(BASE, E=128), 'fp32')):
        opt, model, sd = build(pkg, kw, 33, mode)
        videos, _ = make_videos(pkg, model, 64, [(256, 2), (200, 1)], 900, T=256)
        got, want = both_ways(pkg, lib, model, lambda: model.forward_videos(videos), native=False)
        same(got, want, ('fallback', kw['E'], mode))
        got, want = both_ways(pkg, lib, model, lambda: model(*videos[0], eval=True), native=False)
        same(got, want, ('fallback single', kw['E'], mode))
        option(pkg, lib, 'half_native', 2)
        try:
            with pytest.raises(RuntimeError, match='cannot read them natively'):
                model(*videos[0], eval=True)
        finally:
            option(pkg, lib, 'half_native', -1)
    # T % 4 != 0 cannot be a padded length of these models; a feature pointer off the 8-byte grid can: the upcast path serves it
    opt, model, sd = build(pkg, dict(BASE, E=128), 33)
    videos, _ = make_videos(pkg, model, 64, [(T_ENGINE, 1)], 901)
    vid, sh = videos[0][0], videos[0][1]
    odd = torch.zeros(vid.numel() + 1, dtype=torch.float16, device='cuda')[1:].view_as(vid).copy_(vid)
    assert odd.data_ptr() % 8 == 2 and odd.is_contiguous()
    want = flat(model(*videos[0], eval=True))
    same(flat(model(odd, sh, *videos[0][2:], eval=True)), want, 'misaligned feature pointer')


def test_native_half_forward_against_the_fp64_oracle(ctx):
    """e_gpu <= max(4 e_ref, 2^-21 max |y64|) with y64 / y32 the oracle in fp64 / fp32 on the binary16-rounded features.  The video is
    448 = 7 * 64 clips long, a whole number of gate blocks: the gate's nearest-neighbour upsampling then maps clips to blocks with the
    exact scale 1 / 64 in fp32 and in fp64 alike.  (At a length like 470 the two oracles round t * n / len differently at block
    edges, open different clips, and e_ref is 0.36 -- a bound that checks nothing; e_ref is asserted to be of fp32 size for that reason.)"""
    pkg, lib = ctx
    opt, model, sd = build(pkg, dict(BASE, E=128), 43)
    videos, cpu = make_videos(pkg, model, 64, [(448, 2)], 1400)
    option(pkg, lib, 'half_native', 2)
    try:
        lg, of, mk = model(*videos[0], eval=True)
    finally:
        option(pkg, lib, 'half_native', -1)
    assert model.last_feature_dtype is torch.float16 and model.numerics_status() & 1 == 0
    inp = dict(cpu[0], vid=cpu[0]['vid'].half().float(), shallow_vid=cpu[0]['shallow_vid'].half().float())
    ones = lambda t: torch.ones(1, 1, t.size(-1), dtype=torch.bool)
    res = {}
    for name, ns in (('y64', FP.oracle64), ('y32', R)):
        with torch.no_grad():
            texts, tmasks = zip(*[ns.encode_text(sd, opt.model, t[None], ones(t)) for t in inp['tokens']])
            res[name] = ns.forward_eval(sd, opt.model, inp['vid'], inp['shallow_vid'], inp['vid_masks'], list(texts), inp['text_cls'], list(tmasks))
    for q in range(2):
        for l in range(4):
            assert torch.equal(mk[q][l].cpu(), res['y64'][2][q][l]) and torch.equal(mk[q][l].cpu(), res['y32'][2][q][l])
    select = [m.cpu() for q in mk for m in q]
    for k, (name, got) in enumerate((('logits', lg), ('offsets', of))):
        top, e_ref = FP.rule(FP.pool(got, select), FP.pool(res['y64'][k], select), FP.pool(res['y32'][k], select))[:2]
        assert e_ref <= 2.0 ** -16 * top, (name, e_ref, top)      # the two oracles took the same discrete decisions
        FP.check(f'half features {name}', FP.pool(got, select), FP.pool(res['y64'][k], select), FP.pool(res['y32'][k], select))


def test_a_half_inf_raises_the_status_word(ctx):
    """one binary16 inf in vid, at a clip the gate keeps: bit 0 of dcf_numerics_status, as on the fp32 path; a status word, no fault"""
    pkg, lib = ctx
    status = {}
    for half in (True, False):
        opt, model, sd = build(pkg, dict(BASE, E=128), 44)
        model.half_features = half
        videos, _ = make_videos(pkg, model, 64, [(T_ENGINE, 1)], 1500)
        option(pkg, lib, 'half_native', 2 if half else 1)
        try:
            model(*videos[0], eval=True)
            assert model.numerics_status() & 1 == 0
            gate = gate_tap(pkg, lib, model, 1, T_ENGINE)
            t = int(gate[0].nonzero()[0])               # a clip the gate keeps: its row of the expert product is computed
            vid = videos[0][0].clone()
            vid[0, 3, t] = float('inf')
            lg, _, _ = model(vid, *videos[0][1:], eval=True)
            status[half] = model.numerics_status() & 1
            assert model.last_feature_dtype is (torch.float16 if half else torch.float32)
            assert all(bool(torch.isnan(x).all()) for x in lg[0]), 'the flagged forward overwrites its logits with NaN'
        finally:
            option(pkg, lib, 'half_native', -1)
    assert status == {True: 1, False: 1}, status


# ---------------------------------------------------------------------------------------------- evaluator
def test_the_evaluator_in_float16_returns_the_proposals_of_the_rounded_features(ctx):
    pkg, lib = ctx
    kw = dict(BASE, E=128, sn=8, max_vid_len=128)
    opt, model, sd = build(pkg, kw, 21)
    g = torch.Generator().manual_seed(3)
    datas = []
    for v, vid_len in enumerate((300, 128, 77)):
        datas.append(dict(vid=torch.randn(64, vid_len, generator=g), shallow_vid=torch.randn(64, vid_len, generator=g),
                          text=tuple(torch.randn(32, 6, generator=g) for _ in range(2)), text_cls=torch.randn(2, 64, generator=g),
                          fps=30.0, clip_stride=16, clip_size=32, duration=200.0, clip_id=f'v{v}'))
    ev16 = pkg.evaluator.GroundingEvaluator(opt, model, feature_dtype='float16')
    ev32 = pkg.evaluator.GroundingEvaluator(opt, model)
    option(pkg, lib, 'half_native', 2)
    try:
        for data in datas:
            got = ev16.predict(data)
            assert model.last_feature_dtype is torch.float16
            option(pkg, lib, 'half_native', 1)
            model.half_features = False
            want = ev32.predict(dict(data, vid=data['vid'].half().float(), shallow_vid=data['shallow_vid'].half().float()))
            model.half_features = True
            option(pkg, lib, 'half_native', 2)
            assert model.last_feature_dtype is torch.float32 and len(got) == len(want) == 2
            for a, b in zip(got, want):
                assert torch.equal(a['segments'], b['segments']) and torch.equal(a['scores'], b['scores'])
    finally:
        option(pkg, lib, 'half_native', -1)
        model.half_features = True
    with pytest.raises(ValueError, match='video v0: 1 finite values of vid'):
        bad = dict(datas[0], vid=datas[0]['vid'].clone())
        bad['vid'][5, 7] = 1e6
        ev16.predict(bad)
