"""The training forward with dropout and drop-path on the GPU: the keep bits of the Philox stream against the numpy
restatement (tests/philox_ref.py), their statistics, the forward against the reference's train()-mode forward with the
same masks (tests/golden/train_dropout.npz), determinism, and that nothing leaks into the other paths.  GPU only."""
import ctypes
import time

import numpy as np
import pytest
import torch

import philox_ref as P
from conftest import Golden, load_pkg

pytestmark = pytest.mark.gpu
TOL = dict(rtol=2e-4, atol=2e-4)          # the former TOL of test_gpu_e2e.py (no fp64 side here: the oracle draws no masks)


def keep_gpu(pkg, seed, site, e0, n, p):
    out = torch.empty(n, dtype=torch.uint8, device='cuda')
    sseed = seed - (1 << 64) if seed >= 1 << 63 else seed
    lib = pkg._lib.lib()
    pkg._lib.check(lib.dcf_debug_dropout_keep(sseed, site, e0, n, ctypes.c_float(p), pkg._lib.ptr(out), pkg._lib.current_stream()),
                   'dcf_debug_dropout_keep')
    return out.cpu().numpy().astype(bool)


def test_debug_keep_bits_equal_the_restatement():
    pkg = load_pkg()
    for seed in (0, 1, 0x9E3779B97F4A7C15, (1 << 64) - 1):
        for site in (P.site(1, 0, 0), P.site(3, 5, 1), P.site(4, 7, 5), P.site(2, 0, 4)):
            for e0, n in ((0, 1003), (5, 4097), ((1 << 32) - 7, 1001), ((1 << 40) + 3, 515)):
                for p in (0.1, 0.5):
                    got = keep_gpu(pkg, seed, site, e0, n, p)
                    want = P.keep(seed, site, np.arange(e0, e0 + n, dtype=np.uint64), p)
                    assert np.array_equal(got, want), (seed, site, e0, n, p)


def _corr(x, y):
    x, y = x.astype(np.float64), y.astype(np.float64)
    return float(((x - x.mean()) * (y - y.mean())).mean() / (x.std() * y.std()))


@pytest.mark.parametrize('p', [0.1, 0.5])
def test_keep_statistics(p):
    pkg = load_pkg()
    n = 1 << 24
    seed = 0x243F6A8885A308D3
    a = keep_gpu(pkg, seed, P.site(3, 2, 1), 0, n, p)
    sigma = np.sqrt(p * (1 - p) / n)
    assert abs(a.mean() - (1 - p)) < 5 * sigma, (a.mean(), 1 - p, sigma)
    b = keep_gpu(pkg, seed, P.site(3, 2, 2), 0, n, p)           # the neighbouring site, same elements
    assert abs(_corr(a, b)) < 5 / np.sqrt(n)
    c = keep_gpu(pkg, seed, P.site(3, 3, 1), 0, n, p)           # the neighbouring layer
    assert abs(_corr(a, c)) < 5 / np.sqrt(n)
    # neighbouring samples b, b + 1: drop-path (e = b) and one (C, T) plane of a dropout tensor apart
    assert abs(_corr(a[:-1], a[1:])) < 5 / np.sqrt(n)
    plane = 64 * 256
    assert abs(_corr(a[:-plane], a[plane:])) < 5 / np.sqrt(n)


def _fixture_model(pkg, g, case):
    kw, meta = g.js(f'{case}/opt_kwargs'), g.js(f'{case}/meta')
    opt = pkg.config.make_opt(**kw)
    for part in ('vid_net', 'fusion'):
        opt.model[part]['proj_pdrop'] = meta['proj_pdrop']
        opt.model[part]['path_pdrop'] = meta['path_pdrop']
    model = pkg.modeling.create_model(opt)
    model.load_state_dict(pkg.synth.make_state_dict(g.js(f'{case}/shapes'), meta['wseed']))
    return model.cuda().train().requires_grad_(False), kw, meta


def _fixture_args(g, case):
    c = lambda k: g.t(f'{case}/{k}').cuda()
    return (c('vid'), c('shallow'), c('vid_masks'), c('tokens'), c('text_cls'), c('token_masks'))


def _run(model, args, sizes, seed=None):
    if seed is not None:
        model._next_dropout_seed = lambda: seed                 # the fixture's key itself (enable_dropout's generator draws keys)
    vid, shallow, vm, tok, cls, tm = args
    out = model(vid, shallow, vm, tok, cls, tm, text_size=torch.tensor(sizes), eval=False)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('case', ['e64', 'e256'])
def test_forward_matches_reference_with_the_same_masks(case):
    pkg = load_pkg()
    g = Golden('train_dropout.npz')
    model, kw, meta = _fixture_model(pkg, g, case)
    model.enable_dropout(refine_pdrop=meta['refine_pdrop'])
    out4 = _run(model, _fixture_args(g, case), meta['sizes'], seed=meta['seed'])
    assert model.last_dropout_seed == meta['seed']
    L = kw['n_levels']
    assert len(out4) == 4 and all(len(p) == L for p in out4)
    for part, name in zip(out4, ('logits1', 'logits2', 'offsets', 'masks')):
        for l in range(L):
            want = g.t(f'{case}/{name}/l{l}')
            assert part[l].shape == want.shape
            if name == 'masks':
                assert torch.equal(part[l].cpu(), want)
            else:
                torch.testing.assert_close(part[l].cpu(), want, **TOL)
    # the masks the reference was given are the ones the kernels draw
    for s in g.js(f'{case}/sites'):
        sub = s['site'] & 15
        p = meta['path_pdrop'] if sub in (P.PATH_ATTN, P.PATH_FFN) else meta['refine_pdrop'] if sub == P.TCN else meta['proj_pdrop']
        n = min(int(np.prod(s['shape'])), 4096)
        got = keep_gpu(pkg, meta['seed'], s['site'], 0, n, p)
        assert torch.equal(torch.from_numpy(np.packbits(got)), g.t(f'{case}/keep/{s["site"]}'))


def test_same_seed_same_outputs_across_calls_and_graph_modes():
    pkg = load_pkg()
    g = Golden('train_dropout.npz')
    model, kw, meta = _fixture_model(pkg, g, 'e64')
    args = _fixture_args(g, 'e64')
    model.enable_dropout(refine_pdrop=meta['refine_pdrop'])
    outs = []
    for mode in ('never', 'always', 'always', 'never'):
        model.graph_mode = mode
        outs.append(_run(model, args, meta['sizes'], seed=1234567))
    for o in outs[1:]:
        for a, b in zip(o, outs[0]):
            assert all(torch.equal(x, y) for x, y in zip(a, b))
    other = _run(model, args, meta['sizes'], seed=7654321)
    assert not all(torch.equal(x, y) for x, y in zip(other[1], outs[0][1]))
    # the private generator of enable_dropout(seed=int): reproducible key sequence
    model, _, _ = _fixture_model(pkg, g, 'e64')
    model.enable_dropout(seed=99, refine_pdrop=meta['refine_pdrop'])
    r1 = [_run(model, args, meta['sizes'])[1] for _ in range(2)]
    k1 = model.last_dropout_seed
    model.enable_dropout(seed=99, refine_pdrop=meta['refine_pdrop'])
    r2 = [_run(model, args, meta['sizes'])[1] for _ in range(2)]
    assert model.last_dropout_seed == k1
    assert all(torch.equal(x, y) for a, b in zip(r1, r2) for x, y in zip(a, b))
    assert not all(torch.equal(x, y) for x, y in zip(r1[0], r1[1]))


def test_zero_rates_equal_the_disabled_forward():
    pkg = load_pkg()
    g = Golden('train.npz')
    meta, kw = g.js('meta'), g.js('opt_kwargs')
    opt = pkg.config.make_opt(**kw)
    model = pkg.modeling.create_model(opt)
    model.load_state_dict(pkg.synth.make_state_dict(g.js('shapes'), meta['wseed']))
    model = model.cuda().train().requires_grad_(False)
    args = (g.t('vid').cuda(), g.t('shallow').cuda(), g.t('vid_masks').cuda(), g.t('tokens').cuda(), g.t('text_cls').cuda(),
            g.t('token_masks').cuda())
    ref = _run(model, args, meta['sizes'])
    model.enable_dropout(refine_pdrop=0.0)
    got = _run(model, args, meta['sizes'])
    for a, b in zip(got, ref):
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_eval_forward_unaffected_by_a_dropout_forward():
    pkg = load_pkg()
    g = Golden('train_dropout.npz')
    model, kw, meta = _fixture_model(pkg, g, 'e64')
    vid, shallow, vm, tok, cls, tm = _fixture_args(g, 'e64')
    enc, encm = model.encode_text(tok, tm)

    def ev():
        out = model(vid[:1], shallow[:1], vm[:1], tuple(enc[i:i + 1] for i in range(2)), cls[:2], tuple(encm[i:i + 1] for i in range(2)),
                    eval=True)
        torch.cuda.synchronize()
        return out

    before = ev()
    model.enable_dropout(refine_pdrop=meta['refine_pdrop'])
    _run(model, (vid, shallow, vm, tok, cls, tm), meta['sizes'], seed=meta['seed'])
    after = ev()
    for a, b in zip(before, after):
        for x, y in zip(a, b):
            assert all(torch.equal(u, v) for u, v in zip(x, y))


def test_bench_shape_dropout_forward():
    """BASELINE configs[2] shape: T = 16 384, D = 1024, E = 256, 8 levels, 2 videos x 2 queries"""
    pkg = load_pkg()
    kw = dict(D=1024, E=256, TE=256, text_in=512, n_levels=8, win=9, n_heads=4, sn=60, sratio=0.3, msf=True,
              norm=True, max_seq_len=2304, text_layers=5, text_max_len=48, fusion_layers=2)
    opt = pkg.config.make_opt(**kw)
    for part in ('vid_net', 'fusion'):
        opt.model[part]['proj_pdrop'] = 0.1
        opt.model[part]['path_pdrop'] = 0.1
    model = pkg.modeling.create_model(opt)
    model.load_state_dict(pkg.synth.make_state_dict({k: list(v.shape) for k, v in model.state_dict().items()}, 2025))
    model = model.cuda().train().requires_grad_(False)
    T, gen = 16384, torch.Generator().manual_seed(5)
    vid = torch.randn(2, 1024, T, generator=gen).cuda()
    shallow = torch.randn(2, 1024, T, generator=gen).cuda()
    vm = torch.stack([torch.arange(T) < n for n in (T, 15000)]).cuda()
    tok = torch.randn(4, 512, 20, generator=gen).cuda()
    tm = torch.ones(4, 1, 20, dtype=torch.bool, device='cuda')
    cls = torch.randn(4, 1024, generator=gen).cuda()
    args = (vid, shallow, vm, tok, cls, tm)

    def timed(seed=None, reps=3):
        _run(model, args, [2, 2], seed=seed)
        t0 = time.perf_counter()
        for _ in range(reps):
            out = _run(model, args, [2, 2], seed=seed)
        return out, (time.perf_counter() - t0) / reps * 1e3

    model.enable_dropout(refine_pdrop=0.5)
    a, ms_drop = timed(seed=11)
    b, _ = timed(seed=11, reps=1)
    for part in a[:3]:
        assert all(torch.isfinite(x).all() for x in part)
    for x, y in zip(a, b):
        assert all(torch.equal(u, v) for u, v in zip(x, y))
    model.disable_dropout()
    for part in ('vid_net', 'fusion'):
        model.opt.model[part]['proj_pdrop'] = 0.0
        model.opt.model[part]['path_pdrop'] = 0.0
    _, ms_plain = timed()
    print(f'\ntraining forward T={T} 2 videos x 2 queries: dropout {ms_drop:.2f} ms, no dropout {ms_plain:.2f} ms')
