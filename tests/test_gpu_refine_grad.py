"""GPU checks of the refinement stage's forward / backward pairs (csrc/refine_grad.hip: dcf_op_refine_in, dcf_op_tcn_layer and their
`_bwd`) and of the autograd functions over them, up to autograd.fuse_and_predict.

The yardstick is the project's rule (tests/test_gpu_dec_grad.py, test_gpu_enc_grad.py), per tensor:

    e_gpu <= max(4 * e_ref, 2^-21 * max |g_64|),   e = max |g - g_64|

with g_64 the closed forms of tests/refine_grad_ref.py in fp64 on the CPU (tests/test_refine_grad_cpu.py pins them to fp64 autograd
through the oracle; the reference's own fp64 `backward()` for the fixture) and e_ref the error of the same computation in fp32 on the
CPU (the reference's fp32 `backward()` for the fixture).  Forward values go by the same expression.  Every check prints an `RGERR`
line; the error table of profiles/refine_grad.md is filled from them.

Operator inputs: X ~ N(0, 1), dY ~ 1e-3 N(0, 1) on every row, padded ones included; weights at the scale of PyTorch's initialisation with
biases and LayerNorm weights off their initial values; masks with padded tails.
"""
import pytest
import torch

from conftest import load_pkg
import refine_grad_ref as R

pytestmark = pytest.mark.gpu
FLOOR = 2.0 ** -21
SLICE = 128                    # RG_SLICE_ROWS of csrc/refine_grad.h: the (2, SLICE + 6, 8) case relies on it
SEED = 0x5DEECE66D1234567


def check(tag, got, g64, g32):
    got, g64, g32 = got.detach().cpu().double(), g64.detach().double(), g32.detach().double()
    assert got.shape == g64.shape == g32.shape, (tag, got.shape, g64.shape, g32.shape)
    assert bool(torch.isfinite(got).all()), tag
    e_ref, e_gpu, top = float((g32 - g64).abs().max()), float((got - g64).abs().max()), float(g64.abs().max())
    bound = max(4 * e_ref, FLOOR * top)
    print(f'RGERR {tag}: max|g64| {top:.3e} e_ref {e_ref:.3e} e_gpu {e_gpu:.3e} bound {bound:.3e} ratio {e_gpu / bound if bound else 0.0:.3f}')
    assert e_gpu <= bound, (tag, e_gpu, bound)
    return bound


def cu(*ts):
    return [None if t is None else t.cuda() for t in ts]


class Lib:
    def __init__(self):
        self.pkg = load_pkg()
        self.L, self.l = self.pkg._lib.lib(), self.pkg._lib

    def layer(self, x, mask, P, dil, drop=None, layer=0):
        """Y of device tensors, pre-filled with NaN; drop = (seed, p, b0)"""
        (B, T0, _), l = x.shape, self.l
        seed, p, b0 = drop or (0, 0.0, 0)
        y = torch.full_like(x, float('nan'))
        l.check(self.L.dcf_op_tcn_layer(l.ptr(x), l.ptr(mask), *(l.ptr(t) for t in P), l.ptr(y), B, T0, dil, seed, p, layer, b0, l.current_stream()),
                'dcf_op_tcn_layer')
        return y

    def layer_bwd(self, x, mask, P, dil, dy, drop=None, layer=0, want=(True,) * 7, into=None, accumulate=0):
        """(dX, dWd, dbd, dWp, dbp, dln_w, dln_b); outputs pre-filled with NaN (or `into`), None where not wanted"""
        (B, T0, _), l = x.shape, self.l
        seed, p, b0 = drop or (0, 0.0, 0)
        outs = into or [torch.full_like(t, float('nan')) if w else None for t, w in zip((x,) + tuple(P), want)]
        l.check(self.L.dcf_op_tcn_layer_bwd(l.ptr(x), l.ptr(mask), *(l.ptr(t) for t in P), l.ptr(dy), *(l.ptr(t) for t in outs), B, T0, dil, seed, p,
                                            layer, b0, accumulate, l.current_stream()), 'dcf_op_tcn_layer_bwd')
        return outs

    def refine_in(self, lg, mask, W, b, T0):
        B, l = lg.size(0), self.l
        h = torch.full((B, T0, R.C), float('nan'), device=lg.device)
        l.check(self.L.dcf_op_refine_in(l.ptr(lg), l.ptr(mask), l.ptr(W), l.ptr(b), l.ptr(h), B, T0, W.size(1), l.current_stream()), 'dcf_op_refine_in')
        return h

    def refine_in_bwd(self, lg, mask, W, dh, want=(True, True, True), into=None, accumulate=0):
        (B, T0, _), l = dh.shape, self.l
        outs = into or [torch.full_like(t, float('nan')) if w else None for t, w in zip((lg, W, W[:, 0].contiguous()), want)]
        l.check(self.L.dcf_op_refine_in_bwd(l.ptr(lg), l.ptr(mask), l.ptr(W), l.ptr(dh), *(l.ptr(t) for t in outs), B, T0, W.size(1), accumulate,
                                            l.current_stream()), 'dcf_op_refine_in_bwd')
        return outs


@pytest.fixture(scope='module')
def lib():
    return Lib()


def layer_case(B, T0, seed, masked=True):
    gen = torch.Generator().manual_seed(seed)
    P = tuple(t.contiguous() for t in R.random_layer(gen))
    P = (P[0], P[1], P[2].reshape(R.C, R.C).contiguous()) + P[3:]
    x = torch.randn(B, T0, R.C, generator=gen)
    dy = torch.randn(B, T0, R.C, generator=gen) * 1e-3
    mask = R.tail_mask(B, T0, gen) if masked else None
    return x, mask, P, dy


def layer_refs(x, mask, P, dil, dy, ks=None):
    """((Y, dX, dWd, ...) by the closed forms in fp64, the same in fp32)"""
    out = []
    for dt in (torch.float64, torch.float32):
        xd, Pd, dyd = x.to(dt), tuple(t.to(dt) for t in P), dy.to(dt)
        out.append((R.tcn_layer(xd, mask, Pd, dil, ks),) + R.tcn_layer_grads(xd, mask, Pd, dil, dyd, ks))
    return out


def run_layer(lib, x, mask, P, dil, dy, drop=None, layer=0):
    xc, mc, dyc = cu(x, mask, dy)
    Pc = cu(*P)
    return [lib.layer(xc, mc, Pc, dil, drop, layer)] + lib.layer_bwd(xc, mc, Pc, dil, dyc, drop, layer)


LAYER_CASES = [(2, 72, 1, True), (3, 7, 2, True), (1, 63, 4, False), (2, 40, 32, True), (2, 40, 64, True), (2, SLICE + 6, 8, True)]


@pytest.mark.parametrize('B,T0,dil,masked', LAYER_CASES)
def test_layer_forward_and_gradients_match_fp64(lib, B, T0, dil, masked):
    """(2, 72, 1), (3, 7, 2): padded tails, a tile that holds several sequences; (1, 63, 4): one row short of a tile; (2, 40, 32): the side
    taps mostly fall off the sequence; (2, 40, 64): dilation > T0, only the centre tap lands; (2, SLICE + 6, 8): three reduction slices,
    and taps that would cross from one sequence into the other if the kernel indexed flat rows"""
    x, mask, P, dy = layer_case(B, T0, seed=T0 * 5 + dil, masked=masked)
    r64, r32 = layer_refs(x, mask, P, dil, dy)
    got = run_layer(lib, x, mask, P, dil, dy)
    tag = f'layer B{B} T{T0} d{dil}'
    for name, a, b, c in zip(('Y',) + R.GRAD_NAMES, got, r64, r32):
        check(f'{tag} {name}', a, b.reshape(a.shape), c.reshape(a.shape))
    if masked:
        assert torch.equal(got[0].cpu()[~mask], P[5].expand(int((~mask).sum()), R.C)), 'a padded row holds ln_b'
        if dil < T0:
            assert float(got[1].cpu()[~mask].abs().max()) > 0, 'dX is not zero at padded rows'


def test_taps_stay_inside_their_sequence(lib):
    """sequence 1 is 100 times sequence 0: a kernel that let a tap cross the boundary between the two would move Y and the gradients of
    the rows next to it by far more than the bound"""
    B, T0, dil = 2, 40, 8
    x, mask, P, dy = layer_case(B, T0, seed=77, masked=False)
    x[1] *= 100
    r64, r32 = layer_refs(x, mask, P, dil, dy)
    got = run_layer(lib, x, mask, P, dil, dy)
    for name, a, b, c in zip(('Y',) + R.GRAD_NAMES, got, r64, r32):
        check(f'seam {name}', a, b.reshape(a.shape), c.reshape(a.shape))
    flat = x.reshape(1, B * T0, R.C).double()                            # what crossing taps would compute
    wrong = R.tcn_layer(flat, None, tuple(t.double() for t in P), dil).reshape(B, T0, R.C)
    assert float((wrong - r64[0]).abs().max()) > 100 * FLOOR * float(r64[0].abs().max())


REFINE_CASES = [(3, 40, 3, True), (1, 64, 1, False), (2, 128, 8, True)]


@pytest.mark.parametrize('B,T0,L,masked', REFINE_CASES)
def test_refine_in_forward_and_gradients_match_fp64(lib, B, T0, L, masked):
    gen = torch.Generator().manual_seed(T0 + L)
    S = sum(R.sizes(T0, L))
    lg, W, b = torch.randn(B, S, generator=gen), torch.randn(R.C, L, generator=gen) / L ** 0.5, 0.1 * torch.randn(R.C, generator=gen)
    dh = torch.randn(B, T0, R.C, generator=gen) * 1e-3
    mask = R.tail_mask(B, T0, gen) if masked else None
    refs = []
    for dt in (torch.float64, torch.float32):
        refs.append((R.refine_in(lg.to(dt), mask, W.to(dt), b.to(dt), T0),) + R.refine_in_grads(lg.to(dt), mask, W.to(dt), dh.to(dt)))
    lgc, mc, Wc, bc, dhc = cu(lg, mask, W, b, dh)
    got = [lib.refine_in(lgc, mc, Wc, bc, T0)] + lib.refine_in_bwd(lgc, mc, Wc, dhc)
    for name, a, r64, r32 in zip(('H', 'dlogits1', 'dW_in', 'db_in'), got, *refs):
        check(f'refine_in B{B} T{T0} L{L} {name}', a, r64, r32)
    # exactness: repeats, scaling, NULL outputs, accumulate
    again = lib.refine_in_bwd(lgc, mc, Wc, dhc)
    assert all(torch.equal(a, b_) for a, b_ in zip(got[1:], again))
    scaled = lib.refine_in_bwd(lgc, mc, Wc, dhc * 128.0)
    assert all(torch.equal(a * 128.0, b_) for a, b_ in zip(got[1:], scaled))
    for want in ((True, False, False), (False, True, False), (False, False, True), (False, True, True)):
        part = lib.refine_in_bwd(lgc, mc, Wc, dhc, want=want)
        for i in range(3):
            assert (part[i] is None) if not want[i] else torch.equal(part[i], got[1 + i]), (want, i)
    base = [torch.full_like(t, 0.5) for t in got[1:]]
    lib.refine_in_bwd(lgc, mc, Wc, dhc, into=base, accumulate=1)
    assert torch.equal(base[0], got[1]), 'dlogits1 is not a parameter gradient: it is overwritten'
    assert torch.equal(base[1], 0.5 + got[2]) and torch.equal(base[2], 0.5 + got[3])


def test_dropout_follows_the_philox_mask(lib):
    """p = 0.5, b0 = 1, the site of TCN layer 2: forward and gradients against the closed forms with the keep mask of tests/philox_ref.py;
    the dropped elements are those of dcf_debug_dropout_keep; p = 0 gives the bits of the call without dropout"""
    B, T0, dil, layer, drop = 2, 72, 4, 2, (SEED, 0.5, 1)
    x, mask, P, dy = layer_case(B, T0, seed=41)
    ks = R.keep_scale(drop, layer, B, T0)
    r64, r32 = layer_refs(x, mask, P, dil, dy, ks)
    got = run_layer(lib, x, mask, P, dil, dy, drop, layer)
    for name, a, b, c in zip(('Y',) + R.GRAD_NAMES, got, r64, r32):
        check(f'dropout {name}', a, b.reshape(a.shape), c.reshape(a.shape))
    # the dropped set, read off the kernel: with Wp = 0, bp = 1, X = 0 and a full mask, z = keep / (1 - p)
    zero = [torch.zeros_like(t) for t in P]
    probe = (zero[0], zero[1], zero[2], torch.ones(R.C), torch.ones(R.C), zero[5])
    xz = torch.zeros(B, T0, R.C)
    yk = lib.layer(*cu(xz, None), cu(*probe), dil, drop, layer).cpu()
    n = (1 + B) * R.C * T0
    keep = torch.empty(n, dtype=torch.uint8, device='cuda')
    l = lib.l
    l.check(lib.L.dcf_debug_dropout_keep(SEED, R.PH.site(R.PH.G_REFINE, layer, R.PH.TCN), 0, n, 0.5, l.ptr(keep), l.current_stream()),
            'dcf_debug_dropout_keep')
    keep = keep.cpu().reshape(1 + B, R.C, T0)[1:].transpose(1, 2).bool()
    assert torch.equal(keep, ks > 0), 'dcf_debug_dropout_keep and tests/philox_ref.py agree'
    # a row's z is 2 at kept and 0 at dropped channels: LayerNorm maps the kept ones above 0, the dropped ones below (rows of one kind are 0)
    mixed = keep.any(-1) & ~keep.all(-1)
    assert int(mixed.sum()) > B * T0 // 2
    assert torch.equal(yk[mixed] > 0, keep[mixed]), 'the set of dropped elements equals that of dcf_debug_dropout_keep'
    same = run_layer(lib, x, mask, P, dil, dy, (SEED, 0.0, 1), layer)
    plain = run_layer(lib, x, mask, P, dil, dy)
    assert all(torch.equal(a, b) for a, b in zip(same, plain)), 'p = 0 is the call without dropout'
    assert not torch.equal(got[0], plain[0])


def test_layer_exactness(lib):
    """two runs are bit-identical; 2^7 dY scales every output by exactly 2^7; NULL outputs leave the others' bits unchanged; accumulate
    adds into the parameter gradients -- with and without dropout, on three reduction slices"""
    B, T0, dil = 2, SLICE + 6, 8
    x, mask, P, dy = layer_case(B, T0, seed=3)
    xc, mc, dyc = cu(x, mask, dy)
    Pc = cu(*P)
    for drop in (None, (SEED, 0.5, 0)):
        full = lib.layer_bwd(xc, mc, Pc, dil, dyc, drop, 3)
        again = lib.layer_bwd(xc, mc, Pc, dil, dyc, drop, 3)
        assert all(torch.equal(a, b) for a, b in zip(full, again))
        assert torch.equal(lib.layer(xc, mc, Pc, dil, drop, 3), lib.layer(xc, mc, Pc, dil, drop, 3))
        scaled = lib.layer_bwd(xc, mc, Pc, dil, dyc * 128.0, drop, 3)
        for name, a, b in zip(R.GRAD_NAMES, full, scaled):
            assert torch.equal(a * 128.0, b), name
        wants = [tuple(i == k for i in range(7)) for k in range(7)] + [(True,) + (False,) * 6, (False,) + (True,) * 6, (True, False, True, False, True, False, True)]
        for want in wants:
            part = lib.layer_bwd(xc, mc, Pc, dil, dyc, drop, 3, want=want)
            for i in range(7):
                assert (part[i] is None) if not want[i] else torch.equal(part[i], full[i]), (want, i)
        base = [torch.full_like(t, 0.25) for t in full]
        lib.layer_bwd(xc, mc, Pc, dil, dyc, drop, 3, into=base, accumulate=1)
        assert torch.equal(base[0], full[0]), 'dX is overwritten'
        for name, a, b in zip(R.GRAD_NAMES[1:], base[1:], full[1:]):
            assert torch.equal(a, 0.25 + b), name


def build_model(pkg, f):
    model = pkg.modeling.PtTransformerEarlyFusionIterative(pkg.config.make_opt(**f.opt_kwargs), second_fusion=False)
    missing, unexpected = model.load_state_dict(f.sd, strict=False)
    assert not unexpected and not any(k.startswith(('cls_head', 'refine', 'reg_head')) for k in missing)
    return model.cuda()


def test_fuse_and_predict_matches_the_reference_backward(lib):
    """autograd.fuse_and_predict on the fixture: the three outputs of every level, d fpn[l] and every parameter gradient against the
    reference's own fp64 `backward()`"""
    pkg = lib.pkg
    f = R.Fixture(torch.float32)
    model = build_model(pkg, f)
    fpn = [x.cuda().requires_grad_(True) for x in f.fpn]
    l1, l2, off, masks = pkg.autograd.fuse_and_predict(fpn, cu(*f.masks), model)
    for l in range(f.L):
        assert torch.equal(masks[l].cpu(), f.masks[l])
    f.scalar([a.cpu() for a in l1], [a.cpu() for a in l2], [a.cpu() for a in off]).backward()
    for k, outs in (('logits1', l1), ('logits2', l2), ('offsets', off)):
        for l in range(f.L):
            check(f'fixture {k}/l{l}', outs[l], f.out['64'][k][l], f.out['32'][k][l])
    for l in range(f.L):
        check(f'fixture d fpn/l{l}', fpn[l].grad, f.gfpn['64'][l], f.gfpn['32'][l])
    seen = 0
    for k, p in model.named_parameters():
        if k in f.gp['64']:
            check(f'fixture {k}', p.grad, f.gp['64'][k], f.gp['32'][k])
            seen += 1
    assert seen == len(f.gp['64']) == f.meta['n_params']


def test_objective_backward_reaches_every_head_and_the_refinement(lib):
    """fuse_and_predict -> loss.PointObjective -> backward(): a finite, non-zero .grad on every parameter of cls_head, refine, cls_head2
    and reg_head, with the refinement's dropout on.  The Scale of level l takes a gradient from the positive points of level l alone, so
    the targets put positive points on every level (tests/objective_grad_ref.py::annotate with the regression ranges (0, 4), (2, 8),
    (4, 65) and radius 1.5: 4, 5 and 6 of them inside the masks)"""
    pkg = lib.pkg
    f = R.Fixture(torch.float32)
    model = build_model(pkg, f)
    opt = pkg.config.make_opt(**f.opt_kwargs)
    fpn = [x.cuda().requires_grad_(True) for x in f.fpn]
    outputs = pkg.autograd.fuse_and_predict(fpn, cu(*f.masks), model, dropout=(SEED, 0.5, 0))
    targets = torch.tensor([[4.0, 21.0], [3.0, 8.5], [20.0, 25.5]], device='cuda')
    total = pkg.loss.PointObjective(opt)(outputs, targets)['total']
    assert bool(torch.isfinite(total))
    total.backward()
    seen = 0
    for k, p in model.named_parameters():
        if k.startswith(('cls_head.', 'refine.', 'cls_head2.', 'reg_head.')):
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, k
            seen += 1
    assert seen == f.meta['n_params']
    for x in fpn:
        assert bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0


def test_refusals_carry_a_message(lib):
    A, M, l = lib.pkg.autograd, lib.pkg.modeling, lib.l
    net = M.TCN(3, 32, 32, 3).cuda()
    x, m = torch.zeros(1, 8, 32).cuda(), torch.ones(1, 8, dtype=torch.bool).cuda()
    with pytest.raises(RuntimeError, match='GPU'):
        A.tcn_layer(x.cpu(), m, net.layers[0], 1)
    with pytest.raises(RuntimeError, match='GPU'):
        A.refine_in(torch.zeros(1, 14), m, net)
    with pytest.raises(ValueError, match='pyramid'):
        A.refine_in(torch.zeros(1, 13).cuda(), m, net)                        # no T0 gives S = 13 with 3 levels
    with pytest.raises(ValueError, match='pyramid'):
        A.refine_in(torch.zeros(1, 10).cuda(), None, net)                     # T0 = 6 (6 + 3 + 1) is not a multiple of 4
    with pytest.raises(ValueError, match='32 channels'):
        A.tcn_layer(torch.zeros(1, 8, 64).cuda(), None, net.layers[0], 1)
    with pytest.raises(ValueError, match='dilation'):
        A.tcn_layer(x, m, net.layers[0], 0)
    f = R.Fixture(torch.float32)
    model = build_model(lib.pkg, f)
    fpn, masks = cu(*f.fpn), cu(*f.masks)
    with pytest.raises(ValueError, match='length'):
        A.fuse_and_predict([fpn[0][:, :39], fpn[1], fpn[2]], masks, model)    # an odd level length
    with pytest.raises(ValueError, match='channels'):
        A.fuse_and_predict([z[..., :16] for z in fpn], masks, model)
    with pytest.raises(RuntimeError, match='GPU'):
        A.fuse_and_predict(f.fpn, masks, model)
    P = cu(*layer_case(1, 8, 1)[2])
    with pytest.raises(RuntimeError, match='dilation = 0'):
        lib.layer(x, None, P, 0)
    with pytest.raises(RuntimeError, match='p = 1'):
        lib.layer(x, None, P, 1, (1, 1.0, 0))
    lg, W, b = torch.zeros(1, 14).cuda(), torch.zeros(32, 3).cuda(), torch.zeros(32).cuda()
    with pytest.raises(RuntimeError, match='multiple of'):
        lib.refine_in(lg, None, W, b, 6)
    with pytest.raises(RuntimeError, match='L = 17'):
        lib.refine_in(lg, None, torch.zeros(32, 17).cuda(), b, 1 << 16)
