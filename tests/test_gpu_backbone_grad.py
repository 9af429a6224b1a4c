"""GPU checks of the k = 5 / stride-2 MaskedConv1D (csrc/conv_grad.hip: dcf_op_conv5s2_split, dcf_op_conv5s2_bwd_data,
dcf_op_conv5s2_bwd_weight), of autograd.masked_conv1d(stride=2) over them, of the stride-0 blocks of autograd.transformer_encoder and
of autograd.video_transformer / text_transformer.

The yardstick is the project's gradient rule (tests/test_gpu_dec_grad.py), per tensor:

    e_gpu <= max(4 * e_ref, 2^-21 * max |g_64|),   e = max |g - g_64|

with g_64 fp64 autograd on the CPU through the oracle (the reference's own fp64 `backward()` for the fixture cases) and e_ref the error
of the same computation in fp32 on the CPU (the reference's fp32 `backward()` for the fixtures).  Forward values go by the same
expression.  Every check prints a `BGERR` line; the figures are in profiles/backbone_grad.md.

Operator inputs: x ~ N(0, 1), w ~ N(0, 1) / sqrt(5 Cin), dY ~ 1e-3 N(0, 1), masks with holes and a padded tail.

key.bias of every block and k_norm.bias of the video blocks: a constant added to every key moves all scores of a row alike, so these
gradients are 0 in exact arithmetic and g_64, g_32 and the GPU's result are three roundings of 0; the rule is applied to them with
max |g_64| of the same layer's key.weight / k_norm.weight, the terms that cancel (backbone_grad_ref.Fixture.top).
"""
import pytest
import torch

from conftest import load_pkg
import backbone_grad_ref as R

pytestmark = pytest.mark.gpu
FLOOR = 2.0 ** -21
F16X3 = 16


def check(tag, got, g64, g32, top=None):
    got, g64, g32 = got.detach().cpu().double(), g64.detach().double(), g32.detach().double()
    assert got.shape == g64.shape == g32.shape, (tag, got.shape, g64.shape, g32.shape)
    assert bool(torch.isfinite(got).all()), tag
    top = float(g64.abs().max()) if top is None else top
    e_ref, e_gpu = float((g32 - g64).abs().max()), float((got - g64).abs().max())
    bound = max(4 * e_ref, FLOOR * top)
    print(f'BGERR {tag}: max|g64| {top:.3e} e_ref {e_ref:.3e} e_gpu {e_gpu:.3e} bound {bound:.3e} ratio {e_gpu / bound if bound else 0.0:.3f}')
    assert e_gpu <= bound, (tag, e_gpu, bound)
    return bound


class Lib:
    def __init__(self):
        self.pkg = load_pkg()
        self.L, self.l = self.pkg._lib.lib(), self.pkg._lib

    def fwd(self, x, mask, w, rc=False):
        """Y (B, T / 2, N) of device tensors, pre-filled with NaN"""
        (B, T, Cin), N, l = x.shape, w.size(0), self.l
        y = torch.full((B, T // 2, N), float('nan'), device=x.device)
        r = self.L.dcf_op_conv5s2_split(l.ptr(x), l.ptr(mask), l.ptr(w), l.ptr(y), B, T, Cin, N, F16X3, l.current_stream())
        if rc:
            return r, y
        l.check(r, 'dcf_op_conv5s2_split')
        return y

    def bwd_data(self, dy, mask, w, T, rc=False):
        (B, _, N), Cin, l = dy.shape, w.size(1), self.l
        dx = torch.full((B, T, Cin), float('nan'), device=dy.device)
        r = self.L.dcf_op_conv5s2_bwd_data(l.ptr(dy), l.ptr(mask), l.ptr(w), l.ptr(dx), B, T, Cin, N, l.current_stream())
        if rc:
            return r, dx
        l.check(r, 'dcf_op_conv5s2_bwd_data')
        return dx

    def bwd_weight(self, x, mask, dy, rc=False, into=None, accumulate=0):
        (B, T, Cin), N, l = x.shape, dy.size(2), self.l
        dw = torch.full((N, Cin, 5), float('nan'), device=x.device) if into is None else into
        r = self.L.dcf_op_conv5s2_bwd_weight(l.ptr(x), l.ptr(mask), l.ptr(dy), l.ptr(dw), B, T, Cin, N, accumulate, l.current_stream())
        if rc:
            return r, dw
        l.check(r, 'dcf_op_conv5s2_bwd_weight')
        return dw

    def error(self):
        return self.L.dcf_last_error().decode(errors='replace')


@pytest.fixture(scope='module')
def lib():
    return Lib()


def cu(*ts):
    return [None if t is None else t.cuda() for t in ts]


def case(B, T, Cin, N, seed, lens=None, masked=True):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, Cin, generator=gen)
    w = torch.randn(N, Cin, 5, generator=gen) / (5 * Cin) ** 0.5
    dy = torch.randn(B, T // 2, N, generator=gen) * 1e-3
    if lens is None:
        lens = [T if b % 2 == 0 else T - T // 3 - (1 - (T // 3) % 2) for b in range(B)]       # odd sequences: a tail that ends on an odd row
    mask = R.holes(B, T, lens, gen) if masked else torch.ones(B, T, dtype=torch.bool)
    if masked and bool(mask.all()):
        mask[-1, -1] = False                                                       # (the shortest cases: a hole is not left to chance)
    return x, w, dy, mask


def refs(x, mask, w, dy):
    d = lambda z: z.double()
    return R.conv5s2_autograd(d(x), mask, d(w), d(dy)), R.conv5s2_autograd(x, mask, w, dy)


CASES = [(1, 2, 32, 32, None), (3, 6, 32, 64, None), (2, 40, 64, 64, [40, 27]), (1, 130, 64, 32, None), (2, 4100, 64, 64, None), (1, 64, 288, 288, None)]


@pytest.mark.parametrize('B,T,Cin,N,lens', CASES)
def test_operators_match_fp64(lib, B, T, Cin, N, lens):
    """(1, 2, 32, 32): one output row, every tap but 2 and 3 falls outside; (3, 6, 32, 64): batch seams every three output rows;
    (2, 40, 64, 64): lengths 40 / 27, a tail that ends on an odd row; (1, 130, 64, 32): To = 65, one past a 64-row GEMM tile;
    (2, 4100, 64, 64): 4100 output rows -- it relies on CG_MAX_SLICES = 64 (csrc/conv_grad.h) and WG_ROWS = 32 (csrc/conv_grad.hip):
    ceil(4100 / 64) = 65 rows rounded up to 96 per slice, 43 slices, the last of 68 rows = two 32-row chunks and one of 4 rows, added by
    k_cg_reduce; (1, 64, 288, 288): channel counts that are not a power of two (the 128 x 96 GEMM tile, partial 64-column weight-gradient
    tiles)"""
    x, w, dy, mask = case(B, T, Cin, N, seed=T * 3 + Cin + N, lens=lens)
    assert not bool(mask.all())
    (y64, gx64, gw64), (y32, gx32, gw32) = refs(x, mask, w, dy)
    xc, wc, dyc, mc = cu(x, w, dy, mask)
    tag = f'op B{B} T{T} Cin{Cin} N{N}'
    check(f'{tag} Y', lib.fwd(xc, mc, wc), y64, y32)
    dx = lib.bwd_data(dyc, mc, wc, T)
    check(f'{tag} dX', dx, gx64, gx32)
    check(f'{tag} dW', lib.bwd_weight(xc, mc, dyc), gw64, gw32)
    assert bool((dx.cpu()[~mask] == 0).all()), 'dX is exactly 0 at masked rows'


def test_taps_stay_inside_their_sequence(lib):
    """Two sequences (T = 64, Cin = N = 64) whose second starts with large values, against the same sequences run as two calls of B = 1,
    bit for bit.  Forward: x[1, :4] is 500 times larger; both batch sizes run the k-sliced GEMM, whose rows do not depend on M.  dW: the
    large rows are in x[1] and dY[1] = 0, so the call of B = 2 must give the bits of sequence 0 alone (exact zeros add nothing; the row
    slices of sequence 0 are the same 32 rows in both calls).  dX: dY[1, :2] is 2^10 times larger and one element of dY[0] is as large,
    so both calls derive the same power of two from max |dY|; both run the 64 x 64 tile."""
    B, T, C, N = 2, 64, 64, 64
    x, w, dy, _ = case(B, T, C, N, seed=7, masked=False)
    x[1, :4] *= 500.0
    xc, wc = cu(x, w)
    y = lib.fwd(xc, None, wc)
    for b in range(B):
        xb = xc[b:b + 1].contiguous()
        assert torch.equal(y[b:b + 1], lib.fwd(xb, None, wc)), f'forward, sequence {b}'
    dy0 = dy.clone()
    dy0[1] = 0.0
    dyc = dy0.cuda()
    x0, dy00 = xc[:1].contiguous(), dyc[:1].contiguous()
    assert torch.equal(lib.bwd_weight(xc, None, dyc), lib.bwd_weight(x0, None, dy00)), 'dW'
    dy1 = dy.clone()
    big = float(dy1[0].abs().max()) * 1024.0
    dy1[1, :2] = torch.sign(dy1[1, :2]) * big
    dy1[0, 9, 5] = big
    dyc = dy1.cuda()
    dx = lib.bwd_data(dyc, None, wc, T)
    for b in range(B):
        dyb = dyc[b:b + 1].contiguous()
        assert torch.equal(dx[b:b + 1], lib.bwd_data(dyb, None, wc, T)), f'dX, sequence {b}'


def test_determinism_and_power_of_two_scaling(lib):
    B, T, C, N = 2, 600, 64, 64
    x, w, dy, mask = case(B, T, C, N, seed=11)
    xc, wc, mc = cu(x, w, mask)
    outs = []
    for s in (2.0 ** -30, 1.0, 2.0 ** 10):
        dyc = (dy * s).cuda()
        outs.append((lib.bwd_data(dyc, mc, wc, T).cpu() / s, lib.bwd_weight(xc, mc, dyc).cpu() / s))
    for a, b_, c in zip(*outs):
        assert torch.equal(a, b_) and torch.equal(b_, c)
    dyc = dy.cuda()
    first = None
    for _ in range(10):
        got = (lib.bwd_data(dyc, mc, wc, T).clone(), lib.bwd_weight(xc, mc, dyc).clone())
        if first is None:
            first = got
        else:
            assert all(torch.equal(a, b_) for a, b_ in zip(first, got))
    assert bool((first[0].cpu()[~mask] == 0).all()), 'dX is exactly 0 at masked rows'
    base = torch.full((N, C, 5), 0.25, device='cuda')
    lib.bwd_weight(xc, mc, dyc, into=base, accumulate=1)
    assert torch.equal(base, 0.25 + first[1]), 'accumulate adds into dW'


def test_refusals_carry_a_message_and_launch_nothing(lib):
    A = lib.pkg.autograd
    for B, T, C, N, msg in ((1, 7, 32, 32, 'T = 7 must be even'), (1, 8, 48, 32, 'Cin = 48'), (1, 8, 32, 1, 'N = 1')):
        x, w, dy = torch.zeros(B, T, C).cuda(), torch.zeros(N, C, 5).cuda(), torch.zeros(B, T // 2, N).cuda()
        for name, call in (('split', lambda: lib.fwd(x, None, w, rc=True)), ('bwd_data', lambda: lib.bwd_data(dy, None, w, T, rc=True)),
                           ('bwd_weight', lambda: lib.bwd_weight(x, None, dy, rc=True))):
            rc, out = call()
            assert rc == -1 and msg in lib.error() and f'dcf_op_conv5s2_{name}' in lib.error(), (name, lib.error())
            torch.cuda.synchronize()
            assert bool(torch.isnan(out).all()), f'{name} wrote its output'
    x = torch.zeros(1, 8, 32).cuda()
    with pytest.raises(ValueError, match='no bias'):
        A.masked_conv1d(x, None, torch.zeros(32, 32, 5).cuda(), torch.zeros(32).cuda(), stride=2)
    with pytest.raises(ValueError, match='k = 5'):
        A.masked_conv1d(x, None, torch.zeros(32, 32, 3).cuda(), None, stride=2)
    with pytest.raises(ValueError, match='multiple of the stride'):
        A.masked_conv1d(x[:, :7], None, torch.zeros(32, 32, 5).cuda(), None, stride=2)


def test_autograd_masked_conv1d_stride_2(lib):
    B, T, C, N = 2, 40, 64, 96
    x, w, dy, mask = case(B, T, C, N, seed=31, lens=[40, 27])
    (y64, gx64, gw64), (y32, gx32, gw32) = refs(x, mask, w, dy)
    A = lib.pkg.autograd
    xd, wd, md, dyd = cu(x, w, mask, dy)                                        # named: an operand lives until the kernel has been launched
    xg, wg = xd.clone().requires_grad_(True), wd.clone().requires_grad_(True)
    y, mo = A.strided_masked_conv1d(xg, md, wg)
    assert torch.equal(mo.cpu(), mask[:, ::2])
    direct = lib.fwd(xd, md, wd)
    assert torch.equal(y.detach(), direct), 'the forward is the kernel the network runs'
    assert torch.equal(A.masked_conv1d(xd, md, wd, None, 2), direct)
    check('masked_conv1d(stride=2) out', y, y64, y32)
    (y * dyd).sum().backward()
    check('masked_conv1d(stride=2) x.grad', xg.grad, gx64, gx32)
    check('masked_conv1d(stride=2) weight.grad', wg.grad, gw64, gw32)
    x2, w2 = xd.clone().requires_grad_(True), wd.clone()
    (A.masked_conv1d(x2, md, w2, stride=2) * dyd).sum().backward()
    assert w2.grad is None and torch.equal(x2.grad, xg.grad)
    x3, w3 = xd.clone(), wd.clone().requires_grad_(True)
    (A.masked_conv1d(x3, md, w3, stride=2) * dyd).sum().backward()
    assert x3.grad is None and torch.equal(w3.grad, wg.grad)
    # the default is the k = 1 / 3 function it was
    w1 = torch.randn(N, C, 3, generator=torch.Generator().manual_seed(3)).cuda()
    assert torch.equal(A.masked_conv1d(xd, md, w1), A.masked_conv1d(xd, md, w1, None, 1))


def build_backbone(pkg, f):
    M = pkg.modeling
    kw = dict(f.kw)
    if not f.text:
        kw['arch'] = tuple(kw['arch'])
    mod = (M.TextTransformer if f.text else M.VideoTransformer)(**kw)
    mod.load_state_dict(f.sd)
    return mod.cuda()


def check_fixture(f, mod, outs, masks, x):
    for l in range(f.n_levels):
        assert torch.equal(masks[l].cpu(), f.mask_out[l]), f'mask of level {l}'
        check(f'{f.name} out/l{l}', outs[l], f.out['64'][l], f.out['32'][l])
    check(f'{f.name} d x', x.grad, f.gx['64'], f.gx['32'])
    seen = 0
    for k, p in mod.named_parameters():
        assert p.grad is not None, k
        check(f'{f.name} {k}', p.grad, f.gp['64'][k], f.gp['32'][k], top=f.top(None, k))
        seen += 1
    assert seen == len(f.gp['64']) == f.meta['n_params']


@pytest.mark.parametrize('name', R.CASES)
def test_video_transformer_matches_the_reference_backward(lib, name, monkeypatch):
    """autograd.video_transformer on the three fixture cases: every level, the masks, d x and every parameter gradient against the
    reference's own fp64 `backward()`; and the stride 1 / 2 blocks inside it give the bits transformer_encoder gives on its own"""
    pkg = lib.pkg
    A = pkg.autograd
    f = R.Fixture(name, torch.float32)
    mod = build_backbone(pkg, f)
    calls, inner = [], A.transformer_encoder

    def recording(x, mask, block):
        out = inner(x, mask, block)
        calls.append((x.detach().clone(), mask.clone(), block, out[0].detach().clone(), out[1].clone()))
        return out

    monkeypatch.setattr(A, 'transformer_encoder', recording)
    x = f.x.cuda().requires_grad_(True)
    fpn, masks = A.video_transformer(x, f.mask.cuda(), mod)
    monkeypatch.setattr(A, 'transformer_encoder', inner)
    assert len(fpn) == len(masks) == 3 and [y.size(1) for y in fpn] == f.meta['level_lengths']
    sum((y * u.cuda()).sum() for y, u in zip(fpn, f.up)).backward()
    check_fixture(f, mod, fpn, masks, x)
    assert len(calls) == (1 if f.kw['pool_only'] else 4)
    for xin, min_, block, yout, mout in calls:
        y2, m2 = A.transformer_encoder(xin, min_, block)
        assert block.stride in (1, 2) and torch.equal(y2.detach(), yout) and torch.equal(m2, mout)
    if f.kw['use_abs_pe']:
        with pytest.raises(ValueError, match='max_seq_len'):
            A.video_transformer(torch.zeros(1, 4 * f.meta['T'], 32).cuda(), None, mod)


def test_text_transformer_matches_the_reference_backward(lib):
    pkg = lib.pkg
    A = pkg.autograd
    f = R.Fixture('text', torch.float32)
    mod = build_backbone(pkg, f)
    x = f.x.cuda().requires_grad_(True)
    y, mask = A.text_transformer(x, f.mask.cuda(), mod)
    assert y.shape == (3, 10, 32)
    (y * f.up[0].cuda()).sum().backward()
    check_fixture(f, mod, (y,), (mask,), x)
    # freezing one parameter leaves the bits of the others unchanged
    mod2 = build_backbone(pkg, f)
    frozen = 'transformer.1.attn.attn.key.weight'
    dict(mod2.named_parameters())[frozen].requires_grad_(False)
    x2 = f.x.cuda().requires_grad_(True)
    (A.text_transformer(x2, f.mask.cuda(), mod2)[0] * f.up[0].cuda()).sum().backward()
    assert torch.equal(x2.grad, x.grad)
    for (k, p), (_, p2) in zip(mod.named_parameters(), mod2.named_parameters()):
        assert (p2.grad is None) if k == frozen else torch.equal(p2.grad, p.grad), k
    # cross_attention's own limit: 64 tokens and the background token are 65 keys
    long = pkg.modeling.TextTransformer(32, 32, 2, 64, n_layers=1, use_abs_pe=False).cuda()
    with pytest.raises(ValueError, match='Lk = 65'):
        A.text_transformer(torch.zeros(1, 64, 32).cuda(), None, long)
    with pytest.raises(ValueError, match='TextIdentity is not differentiable yet'):
        A.text_transformer(torch.zeros(1, 8, 32).cuda(), None, pkg.modeling.TextIdentity(32, 32, 8).cuda())


def test_objective_backward_reaches_both_backbones(lib):
    """A stride-2 VideoTransformer -> xattn_fusion against text_transformer's output (inside fuse_and_predict of a model with
    second_fusion) -> loss.PointObjective -> backward(): a finite gradient on every parameter of vid_net, text_net, fusion, the heads and
    the refinement, none identically zero save the key.bias / k_norm.bias ones (zero in exact arithmetic).  The Scale of level l takes a
    gradient from the positive points of level l alone: the targets of tests/test_gpu_refine_grad.py put positive points on every level."""
    pkg = lib.pkg
    A = pkg.autograd
    kw = dict(D=32, E=32, TE=32, text_in=32, n_levels=3, win=3, n_heads=2, sn=8, sratio=0.5, msf=True, norm=True, max_seq_len=64,
              text_layers=2, text_max_len=24, n_stem=1, vid_stride=2)
    opt = pkg.config.make_opt(**kw)
    model = pkg.modeling.PtTransformerEarlyFusionIterative(opt, second_fusion=True)
    gen = torch.Generator().manual_seed(5)
    for part in (model.vid_net, model.text_net):
        R.set_backbone_parameters(part, gen)
    import dec_grad_ref
    dec_grad_ref.set_fusion_parameters(model.fusion, gen)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if k.startswith(('cls_head', 'cls_head2', 'reg_head', 'refine')) and k.endswith('bias'):
                p.add_(0.1 * torch.randn(p.shape, generator=gen))
    model = model.cuda()
    T = 80
    vid = torch.randn(2, T, 32, generator=gen).cuda()
    vmask = (torch.arange(T)[None, :] < torch.tensor([80, 55])[:, None]).cuda()
    tokens = torch.randn(3, 9, 32, generator=gen).cuda()
    tmask = (torch.arange(9)[None, :] < torch.tensor([9, 5, 7])[:, None]).cuda()
    fpn, fpn_masks = A.video_transformer(vid, vmask, model.vid_net)
    assert [y.size(1) for y in fpn] == [40, 20, 10]
    text, text_mask = A.text_transformer(tokens, tmask, model.text_net)
    outputs = A.fuse_and_predict(fpn, fpn_masks, model, text=text, text_mask=text_mask, kv_size=torch.tensor([2, 1]).cuda())
    targets = torch.tensor([[4.0, 21.0], [3.0, 8.5], [20.0, 25.5]], device='cuda')
    total = pkg.loss.PointObjective(opt)(outputs, targets)['total']
    assert bool(torch.isfinite(total))
    total.backward()
    seen = 0
    for k, p in model.named_parameters():
        if not k.startswith(('vid_net.', 'text_net.', 'fusion.', 'cls_head.', 'refine.', 'cls_head2.', 'reg_head.')):
            continue
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        if not k.endswith(('key.bias', 'k_norm.bias')):
            assert float(p.grad.abs().max()) > 0, k
        seen += 1
    assert seen == sum(1 for k, _ in model.named_parameters() if not k.startswith('vid_map.'))
