"""GPU checks of the backward of the cross-attention core (csrc/xattn_grad.hip: dcf_op_xattn_bwd), of the AdaLN pair (dcf_op_adaln,
dcf_op_adaln_bwd) and of the autograd functions over them, up to autograd.transformer_decoder and autograd.xattn_fusion.

The yardstick is the project's gradient rule (tests/test_gpu_attn_grad.py, test_gpu_enc_grad.py), per gradient tensor:

    e_gpu <= max(4 * e_ref, 2^-21 * max |g_64|),   e = max |g - g_64|

with g_64 fp64 autograd on the CPU through the oracle (the reference's own fp64 `backward()` for the fixture cases) and e_ref the error
of the same computation in fp32 on the CPU (the reference's fp32 `backward()` for the fixture).  Forward values go by the same
expression (the forward rule of tests/forward_parity.py).  Every check prints a `DGERR` line; the figures are in profiles/dec_grad.md.

Operator inputs: q, k, v ~ N(0, 1), dO ~ 1e-3 N(0, 1), key masks with holes; every sequence keeps at least one valid key.

key.bias of the fixture: a constant added to every key moves all scores of a row alike, so this gradient is 0 in exact arithmetic and
g_64, g_32 and the GPU's result are three roundings of 0.  The rule is applied to it as to every other tensor.
"""
import pytest
import torch

from conftest import load_pkg
import dec_grad_ref as R

pytestmark = pytest.mark.gpu
FLOOR = 2.0 ** -21


def check(tag, got, g64, g32):
    got, g64, g32 = got.detach().cpu().double(), g64.detach().double(), g32.detach().double()
    assert got.shape == g64.shape == g32.shape, (tag, got.shape, g64.shape, g32.shape)
    assert bool(torch.isfinite(got).all()), tag
    e_ref, e_gpu, top = float((g32 - g64).abs().max()), float((got - g64).abs().max()), float(g64.abs().max())
    bound = max(4 * e_ref, FLOOR * top)
    print(f'DGERR {tag}: max|g64| {top:.3e} e_ref {e_ref:.3e} e_gpu {e_gpu:.3e} bound {bound:.3e} ratio {e_gpu / bound if bound else 0.0:.3f}')
    assert e_gpu <= bound, (tag, e_gpu, bound)
    return bound


class Lib:
    def __init__(self):
        self.pkg = load_pkg()
        self.L, self.l = self.pkg._lib.lib(), self.pkg._lib

    def bwd(self, q, k, v, mask, do, heads, want=(True, True, True)):
        """(dQ, dK, dV) of device tensors; outputs pre-filled with NaN, None where not wanted"""
        (B, T, C), Lk, l = q.shape, k.size(1), self.l
        outs = [torch.full_like(z, float('nan')) if w else None for z, w in zip((q, k, v), want)]
        l.check(self.L.dcf_op_xattn_bwd(l.ptr(q), l.ptr(k), l.ptr(v), l.ptr(mask), l.ptr(do), l.ptr(outs[0]), l.ptr(outs[1]), l.ptr(outs[2]),
                                        B, T, Lk, C, heads, l.current_stream()), 'dcf_op_xattn_bwd')
        return outs

    def adaln(self, x, mask, h, norm):
        (B, T, C), l = x.shape, self.l
        y = torch.full_like(x, float('nan'))
        l.check(self.L.dcf_op_adaln(l.ptr(x), l.ptr(mask), l.ptr(h), l.ptr(y), B * T, C, norm, l.current_stream()), 'dcf_op_adaln')
        return y

    def adaln_bwd(self, x, mask, h, dy, norm, want=(True, True)):
        (B, T, C), l = x.shape, self.l
        dx = torch.full_like(x, float('nan')) if want[0] else None
        dh = torch.full_like(h, float('nan')) if want[1] else None
        l.check(self.L.dcf_op_adaln_bwd(l.ptr(x), l.ptr(mask), l.ptr(h), l.ptr(dy), l.ptr(dx), l.ptr(dh), B * T, C, norm, l.current_stream()),
                'dcf_op_adaln_bwd')
        return dx, dh


@pytest.fixture(scope='module')
def lib():
    return Lib()


def case(B, T, Lk, C, seed, masked=True):
    gen = torch.Generator().manual_seed(seed)
    q = torch.randn(B, T, C, generator=gen)
    k, v = (torch.randn(B, Lk, C, generator=gen) for _ in range(2))
    do = torch.randn(B, T, C, generator=gen) * 1e-3
    mask = R.holes(B, Lk, gen) if masked else torch.ones(B, Lk, dtype=torch.bool)
    return q, k, v, do, mask


def autograd_grads(q, k, v, mask, do, heads):
    q, k, v = (z.clone().requires_grad_(True) for z in (q, k, v))
    return torch.autograd.grad((R.oracle_cross_attention(q, k, v, mask, heads) * do).sum(), (q, k, v))


def refs(q, k, v, mask, do, heads):
    """((dQ, dK, dV) by fp64 autograd through the oracle's _mha_global_qkv, the same in fp32)"""
    return autograd_grads(q.double(), k.double(), v.double(), mask, do.double(), heads), autograd_grads(q, k, v, mask, do, heads)


def cu(*ts):
    return [None if t is None else t.cuda() for t in ts]


CASES = [(2, 72, 33, 256, 4), (1, 63, 16, 64, 4), (3, 7, 5, 128, 4), (1, 130, 64, 512, 4), (2, 45, 17, 1024, 16), (1, 1, 9, 64, 2), (2, 4100, 33, 64, 2)]


@pytest.mark.parametrize('B,T,Lk,C,heads', CASES)
def test_gradients_match_fp64(lib, B, T, Lk, C, heads):
    """(2, 72, 33, 256, 4): the model's own Lk and d; (1, 63, 16, 64, 4): d = 16, T no multiple of 64; (1, 130, 64, 512, 4): d = 128, the
    largest Lk; (2, 45, 17, 1024, 16): four 256-channel chunks per row; (1, 1, 9, 64, 2): one query row; (2, 4100, 33, 64, 2): more rows
    than one slice -- it relies on XG_SLICE_ROWS = 512 (csrc/xattn_grad.h): 9 slices per sequence, the last of 4 rows, added by k_xg_reduce"""
    q, k, v, do, mask = case(B, T, Lk, C, seed=T * 3 + C + Lk)
    g64, g32 = refs(q, k, v, mask, do, heads)
    got = lib.bwd(*cu(q, k, v, mask, do), heads)
    tag = f'op B{B} T{T} Lk{Lk} C{C} h{heads}'
    for name, a, b, c in zip(('dQ', 'dK', 'dV'), got, g64, g32):
        check(f'{tag} {name}', a, b, c)
    for a, b in zip(got[1:], g64[1:]):
        assert bool((b[~mask] == 0).all()), 'the fp64 gradient at a masked key is an exact zero'
        assert bool((a.cpu()[~mask] == 0).all()), 'dK / dV at a masked key are exactly 0'


def test_one_key_sequences(lib):
    """Lk = 1: the softmax is over one key, dS = 0, so dQ = dK = 0 exactly; dV = sum_t dO goes by the rule"""
    B, T, Lk, C, heads = 2, 70, 1, 128, 4
    q, k, v, do, mask = case(B, T, Lk, C, seed=17, masked=False)
    g64, g32 = refs(q, k, v, mask, do, heads)
    assert float(g64[0].abs().max()) == 0.0 and float(g64[1].abs().max()) == 0.0
    dq, dk, dv = lib.bwd(*cu(q, k, v, mask, do), heads)
    assert bool((dq == 0).all()) and bool((dk == 0).all())
    check('one-key dV', dv, g64[2], g32[2])


def test_null_mask_equals_an_all_ones_mask(lib):
    B, T, Lk, C, heads = 2, 72, 33, 256, 4
    q, k, v, do, mask = case(B, T, Lk, C, seed=19, masked=False)
    a = lib.bwd(*cu(q, k, v, mask, do), heads)
    b = lib.bwd(*cu(q, k, v, None, do), heads)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('B,T,Lk,C,heads', [(2, 72, 33, 256, 4), (1, 600, 17, 64, 4), (1, 40, 64, 512, 4)])
def test_null_outputs_leave_the_others_bit_identical(lib, B, T, Lk, C, heads):
    q, k, v, do, mask = case(B, T, Lk, C, seed=23)
    args = cu(q, k, v, mask, do)
    full = lib.bwd(*args, heads)
    for want in ((False, True, True), (True, False, True), (True, True, False), (True, False, False), (False, True, False), (False, False, True)):
        part = lib.bwd(*args, heads, want=want)
        for i in range(3):
            assert (part[i] is None) if not want[i] else torch.equal(part[i], full[i]), (want, i)


def test_power_of_two_scaling_of_dO_commutes_bit_for_bit(lib):
    B, T, Lk, C, heads = 2, 600, 33, 256, 4
    q, k, v, do, mask = case(B, T, Lk, C, seed=11)
    outs = []
    for s in (2.0 ** -30, 1.0, 2.0 ** 10):
        outs.append([g.cpu() / s for g in lib.bwd(*cu(q, k, v, mask, do * s), heads)])
    for a, b_, c in zip(*outs):
        assert torch.equal(a, b_) and torch.equal(b_, c)


def test_ten_repeats_are_bit_identical(lib):
    B, T, Lk, C, heads = 3, 1100, 33, 256, 4
    q, k, v, do, mask = case(B, T, Lk, C, seed=21)
    args = cu(q, k, v, mask, do)
    first = None
    for _ in range(10):
        got = [g.clone() for g in lib.bwd(*args, heads)]
        if first is None:
            first = got
        else:
            assert all(torch.equal(a, b_) for a, b_ in zip(first, got))


def test_keys_stay_inside_their_sequence_and_masked_keys_are_ignored(lib):
    """the keys of sequence 1 are 100 times those of sequence 0, and one masked key of sequence 0 is 100 times its neighbours: a kernel that
    indexed K by the wrong b, or ignored kvmask at the large key, would move the gradients by far more than the bound"""
    B, T, Lk, C, heads = 2, 64, 17, 64, 4
    q, k, v, do, _ = case(B, T, Lk, C, seed=5, masked=False)
    mask = torch.ones(B, Lk, dtype=torch.bool)
    mask[0, 6] = False
    k[1] *= 100
    k[0, 6] *= 100
    g64, g32 = refs(q, k, v, mask, do, heads)
    got = lib.bwd(*cu(q, k, v, mask, do), heads)
    bounds = [check(f'seam {n}', a, b, c) for n, a, b, c in zip(('dQ', 'dK', 'dV'), got, g64, g32)]
    d = lambda z: z.double()
    wrong_b = R.cross_attention_grads(d(q), d(k).flip(0), d(v).flip(0), mask.flip(0), d(do), heads)
    wrong_b = (wrong_b[0], wrong_b[1].flip(0), wrong_b[2].flip(0))
    wrong_mask = R.cross_attention_grads(d(q), d(k), d(v), None, d(do), heads)
    for wrong in (wrong_b, wrong_mask):
        for w_, g_, bound in zip(wrong, g64, bounds):
            assert float((w_ - g_).abs().max()) > 100 * bound


ADALN_CASES = [(70, 64), (33, 256), (9, 1024)]


@pytest.mark.parametrize('norm', [1, 0])
@pytest.mark.parametrize('masked', [True, False])
@pytest.mark.parametrize('rows,C', ADALN_CASES)
def test_adaln_pair(lib, rows, C, masked, norm):
    gen = torch.Generator().manual_seed(rows + C + norm)
    x, dy = torch.randn(1, rows, C, generator=gen), torch.randn(1, rows, C, generator=gen) * 1e-3
    h = torch.randn(1, rows, 2 * C, generator=gen)
    mask = (torch.rand(1, rows, generator=gen) > 0.3) if masked else None
    tag = f'adaln rows{rows} C{C} norm{norm} mask{int(masked)}'

    def ref(dt):
        xr, hr = x.to(dt).requires_grad_(True), h.to(dt).requires_grad_(True)
        y = R.oracle_adaln(xr, mask, hr, bool(norm))
        return (y.detach(),) + torch.autograd.grad((y * dy.to(dt)).sum(), (xr, hr))

    r64, r32 = ref(torch.float64), ref(torch.float32)
    xc, mc, hc, dyc = cu(x, mask, h, dy)
    y = lib.adaln(xc, mc, hc, norm)
    dx, dh = lib.adaln_bwd(xc, mc, hc, dyc, norm)
    for name, a, b, c in zip(('Y', 'dX', 'dH'), (y, dx, dh), r64, r32):
        check(f'{tag} {name}', a, b, c)
    if masked:
        assert bool((dx.cpu()[~mask] == 0).all()), 'dX is exactly 0 at a masked row'
        assert torch.equal(y.cpu()[~mask], h[..., C:][~mask]), 'a masked row holds the shift'
    only_x, none = lib.adaln_bwd(xc, mc, hc, dyc, norm, want=(True, False))
    none2, only_h = lib.adaln_bwd(xc, mc, hc, dyc, norm, want=(False, True))
    assert none is None and none2 is None and torch.equal(only_x, dx) and torch.equal(only_h, dh)


def test_autograd_functions_over_the_operators(lib):
    B, T, Lk, C, heads = 2, 72, 33, 256, 4
    q, k, v, do, mask = case(B, T, Lk, C, seed=31)
    g64, g32 = refs(q, k, v, mask, do, heads)
    A, l = lib.pkg.autograd, lib.l
    qc, kc, vc = (z.cuda().requires_grad_(True) for z in (q, k, v))
    out = A.cross_attention(qc, kc, vc, mask.cuda(), heads)
    o = torch.full_like(qc, float('nan')).detach()
    qd, kd, vd, md = cu(q, k, v, mask)                                        # named: an operand lives until the kernel has been launched
    l.check(lib.L.dcf_op_xattn(l.ptr(qd), l.ptr(kd), l.ptr(vd), l.ptr(md), l.ptr(o), B, T, Lk, C, heads, l.current_stream()), 'dcf_op_xattn')
    assert torch.equal(out.detach(), o), 'the forward is the kernel the network runs'
    o64, o32 = R.oracle_cross_attention(q.double(), k.double(), v.double(), mask, heads), R.oracle_cross_attention(q, k, v, mask, heads)
    check('cross_attention out', out, o64, o32)
    (out * do.cuda()).sum().backward()
    for name, z, b, c in zip(('q', 'k', 'v'), (qc, kc, vc), g64, g32):
        check(f'cross_attention {name}.grad', z.grad, b, c)
    q2, k2, v2 = q.cuda().requires_grad_(True), k.cuda(), v.cuda().requires_grad_(True)
    (A.cross_attention(q2, k2, v2, mask.cuda(), heads) * do.cuda()).sum().backward()
    assert k2.grad is None and torch.equal(q2.grad, qc.grad) and torch.equal(v2.grad, vc.grad)
    # adaln_modulate
    gen = torch.Generator().manual_seed(2)
    x, h, dy = torch.randn(2, 40, 64, generator=gen), torch.randn(2, 40, 128, generator=gen), torch.randn(2, 40, 64, generator=gen)
    m = torch.rand(2, 40, generator=gen) > 0.3
    xg, hg = x.cuda().requires_grad_(True), h.cuda().requires_grad_(True)
    y = A.adaln_modulate(xg, m.cuda(), hg, norm=True)
    (y * dy.cuda()).sum().backward()
    for dt, store in ((torch.float64, {}), (torch.float32, {})):
        xr, hr = x.to(dt).requires_grad_(True), h.to(dt).requires_grad_(True)
        yr = R.oracle_adaln(xr, m, hr, True)
        store['y'], (store['gx'], store['gh']) = yr.detach(), torch.autograd.grad((yr * dy.to(dt)).sum(), (xr, hr))
        if dt == torch.float64:
            s64 = store
        else:
            s32 = store
    check('adaln_modulate out', y, s64['y'], s32['y'])
    check('adaln_modulate x.grad', xg.grad, s64['gx'], s32['gx'])
    check('adaln_modulate h.grad', hg.grad, s64['gh'], s32['gh'])


def build_module(pkg, f):
    M = pkg.modeling
    meta = f.meta
    mode = 'adaln' if f.adaln else 'affine'
    mod = (M.TransformerDecoder(meta['vid_dim'], meta['text_dim'], meta['heads'], mode) if f.single else
           M.XAttNFusion(meta['vid_dim'], meta['text_dim'], meta['layers'], meta['heads'], mode))
    mod.load_state_dict(f.sd)
    return mod.cuda()


def run_module(pkg, f, mod, vid, text):
    A = pkg.autograd
    kv = None if f.kv_size is None else f.kv_size.cuda()
    fn = A.transformer_decoder if f.single else A.xattn_fusion
    return fn(vid, f.vid_mask.cuda(), text, f.text_mask.cuda(), mod, kv)


@pytest.mark.parametrize('name', ['single', 'adaln', 'affine'])
def test_composed_blocks_match_the_reference_backward(lib, name):
    """`single`: autograd.transformer_decoder on one layer; `adaln` / `affine`: autograd.xattn_fusion on the two-layer stack with
    kv_size = [2, 1]; the forward output, d vid, d text and every parameter gradient against the reference's own fp64 backward"""
    pkg = lib.pkg
    f = R.Fixture(name, torch.float32)
    mod = build_module(pkg, f)
    vid, text = f.vid.cuda().requires_grad_(True), f.text.cuda().requires_grad_(True)
    out, mask = run_module(pkg, f, mod, vid, text)
    assert torch.equal(mask.cpu(), f.mask_out)
    (out * f.up.cuda()).sum().backward()
    check(f'{name} out', out, f.out['64'], f.out['32'])
    check(f'{name} d vid', vid.grad, f.gvid['64'], f.gvid['32'])
    check(f'{name} d text', text.grad, f.gtext['64'], f.gtext['32'])
    seen = 0
    for k, p in mod.named_parameters():
        check(f'{name} {k}', p.grad, f.gp['64'][k], f.gp['32'][k])
        seen += 1
    assert seen == len(f.gp['64']) == (22 if f.single else 46)
    # freezing one parameter leaves the bits of the others unchanged
    mod2 = build_module(pkg, f)
    frozen = 'xattn.xattn.key.weight' if f.single else 'layers.1.xattn.xattn.key.weight'
    dict(mod2.named_parameters())[frozen].requires_grad_(False)
    vid2, text2 = f.vid.cuda().requires_grad_(True), f.text.cuda().requires_grad_(True)
    (run_module(pkg, f, mod2, vid2, text2)[0] * f.up.cuda()).sum().backward()
    assert torch.equal(vid2.grad, vid.grad) and torch.equal(text2.grad, text.grad)
    for (k, p), (_, p2) in zip(mod.named_parameters(), mod2.named_parameters()):
        assert (p2.grad is None) if k == frozen else torch.equal(p2.grad, p.grad), k


def test_refusals_carry_a_message(lib):
    A = lib.pkg.autograd
    q, k = torch.zeros(1, 4, 64).cuda(), torch.zeros(1, 3, 64).cuda()
    with pytest.raises(RuntimeError, match='GPU'):
        A.cross_attention(q.cpu(), k, k, None, 4)
    with pytest.raises(ValueError, match='head dimension'):
        A.cross_attention(q, k, k, None, 8)                                   # d = 8
    with pytest.raises(ValueError, match='Lk = 0'):
        A.cross_attention(q, k[:, :0], k[:, :0], None, 4)
    with pytest.raises(RuntimeError, match='head dimension 8'):
        lib.bwd(q, k, k, None, q, 8)
    with pytest.raises(RuntimeError, match='Lk = 0'):
        lib.bwd(q, k[:, :0], k[:, :0], None, q, 4)
    with pytest.raises(RuntimeError, match='Lk = 65'):
        k65 = torch.zeros(1, 65, 64).cuda()
        lib.bwd(q, k65, k65, None, q, 4)
