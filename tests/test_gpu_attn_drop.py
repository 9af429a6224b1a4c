"""GPU checks of dropout on the attention map inside the sliding-window core (csrc/attn_drop.hip: dcf_op_local_attn_drop,
dcf_op_local_attn_drop_bwd), of channel dropout (dcf_op_channel_dropout) and of the autograd functions over them.

Inputs are those of tests/test_gpu_attn_grad.py: q, k, v ~ N(0, 1), dO ~ 1e-3 N(0, 1) on EVERY row, padded ones included, masks with
holes; p in {0.1, 0.5}, b0 in {0, 3}.  The restatement is tests/attn_drop_ref.py on the keep bits of tests/philox_ref.py.

 * Keep bits, exactly: with q = k = 0 the map is uniform over the valid keys of the window; the v rows are unit vectors (channel
   key mod d of each head), so every output channel of a row names one key.  The set of non-zero output channels must equal the
   Philox keep set, bit for bit.
 * p = 0 gives the bits of the released dropout-free exports, forward and all three gradients, one case per launch variant (the
   exports run the dropout-free kernels themselves at p = 0: profiles/attn_drop.md).
 * The forward against fp64: rtol = atol = 1e-5 / (1 - p) (tests/test_gpu_ops.py holds the same core to 1e-5 on these inputs, and the
   kept terms are multiplied by 1 / (1 - p)).  The project rule's ratio e_gpu / max(4 e_ref, 2^-21 max|y_64|) is printed (`AFERR`),
   not asserted.
 * The gradients by the project's rule, per tensor: e_gpu <= max(4 e_ref, 2^-21 max|g_64|), g_64 and e_ref from the restatement in
   fp64 and fp32 on the CPU (`AGERR` lines).  dK and dV are exactly 0 at padded keys.
 * NULL outputs leave the others bit-identical, ten repeats are bit-identical, the b0 rule bit for bit, a fully dropped (row, head)
   gives exact zeros.

The kernels choose their path by the window (<= 9, <= 19: unrolled; wider: a loop; <= 32: keep bits packed into a word per (row, head)
and handed to the key side in the statistics; wider: drawn per element) and, in the backward, by C (<= 256 or not); never by row count."""
import pytest
import torch

import attn_drop_ref as R
import philox_ref as P
from conftest import load_pkg
from test_attn_grad_cpu import holes
from test_gpu_attn_grad import check, case, cu

pytestmark = pytest.mark.gpu
SEED = 0x9E3779B97F4A7C15
SITE = P.site(2, 1, R.DROP_ATTN)
FLOOR = 2.0 ** -21
RATES = [(0.1, 0), (0.5, 3)]


class Lib:
    def __init__(self):
        self.pkg = load_pkg()
        self.L, self.l = self.pkg._lib.lib(), self.pkg._lib

    @staticmethod
    def key(seed):
        return seed - (1 << 64) if seed >= 1 << 63 else seed

    def fwd(self, q, k, v, mask, heads, window, p, b0=0, seed=SEED, site=SITE):
        B, T, C = q.shape
        l = self.l
        o = torch.full_like(q, float('nan'))
        l.check(self.L.dcf_op_local_attn_drop(l.ptr(q), l.ptr(k), l.ptr(v), l.ptr(mask), l.ptr(o), B, T, C, heads, window, b0, self.key(seed), site,
                                              p, l.current_stream()), 'dcf_op_local_attn_drop')
        return o

    def bwd(self, q, k, v, mask, do, heads, window, p, b0=0, want=(True, True, True), seed=SEED, site=SITE):
        B, T, C = q.shape
        l = self.l
        outs = [torch.full_like(q, float('nan')) if w else None for w in want]
        l.check(self.L.dcf_op_local_attn_drop_bwd(l.ptr(q), l.ptr(k), l.ptr(v), l.ptr(mask), l.ptr(do), l.ptr(outs[0]), l.ptr(outs[1]),
                                                  l.ptr(outs[2]), B, T, C, heads, window, b0, self.key(seed), site, p, l.current_stream()),
                'dcf_op_local_attn_drop_bwd')
        return outs

    def fwd0(self, q, k, v, mask, heads, window):
        B, T, C = q.shape
        l = self.l
        o = torch.full_like(q, float('nan'))
        l.check(self.L.dcf_op_local_attn(l.ptr(q), l.ptr(k), l.ptr(v), l.ptr(mask), l.ptr(o), B, T, C, heads, window, l.current_stream()),
                'dcf_op_local_attn')
        return o

    def bwd0(self, q, k, v, mask, do, heads, window):
        B, T, C = q.shape
        l = self.l
        outs = [torch.full_like(q, float('nan')) for _ in range(3)]
        l.check(self.L.dcf_op_local_attn_bwd(l.ptr(q), l.ptr(k), l.ptr(v), l.ptr(mask), l.ptr(do), l.ptr(outs[0]), l.ptr(outs[1]), l.ptr(outs[2]),
                                             B, T, C, heads, window, l.current_stream()), 'dcf_op_local_attn_bwd')
        return outs


@pytest.fixture(scope='module')
def lib():
    return Lib()


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# the smallest shapes that reach each variant and each seam: (B, T, C, heads, window)
SHAPES = [(2, 37, 64, 2, 5), (3, 7, 256, 4, 9), (2, 1, 256, 4, 9), (2, 33, 64, 2, 19),
          (1, 90, 128, 2, 31),         # wider than the unrolled variants, and the last widths whose keep bits are packed
          (1, 70, 128, 2, 35),         # keep bits drawn per element, on both sides
          (2, 45, 1024, 16, 9)]        # several channel chunks
REFS = {}


def refs(shape, p, b0):
    """the inputs and the fp64 / fp32 restatement of one case, computed once"""
    key = (shape, p, b0)
    if key not in REFS:
        B, T, C, heads, window = shape
        q, k, v, do, mask = case(B, T, C, seed=T * 3 + C + window)
        keep = R.window_keep(SEED, SITE, B, heads, T, window, p, b0)
        d = lambda z: z.double()
        y64 = R.window_attention_drop(d(q), d(k), d(v), mask, heads, window, keep, p)
        y32 = R.window_attention_drop(q, k, v, mask, heads, window, keep, p)
        g64 = R.window_attention_drop_grads(d(q), d(k), d(v), mask, d(do), heads, window, keep, p)
        g32 = R.window_attention_drop_grads(q, k, v, mask, do, heads, window, keep, p)
        REFS[key] = (q, k, v, do, mask, keep, y64, y32, g64, g32)
    return REFS[key]


# ---------------------------------------------------------------------------------------------- keep bits
@pytest.mark.parametrize('B,T,C,heads,window', [(2, 37, 64, 2, 5), (2, 33, 64, 2, 19), (1, 50, 128, 2, 35)])
@pytest.mark.parametrize('p,b0', RATES)
def test_keep_bits_are_the_philox_stream(lib, B, T, C, heads, window, p, b0):
    d = C // heads
    assert window <= d
    gen = torch.Generator().manual_seed(T + window)
    mask = holes(B, T, gen)
    q = torch.zeros(B, T, C)
    v = torch.zeros(B, T, heads, d)
    v[:, torch.arange(T), :, torch.arange(T) % d] = 1.0                         # key u: channel u mod d of every head
    v = v.reshape(B, T, C)
    out = lib.fwd(*cu(q, q, v, mask), heads, window, p, b0).cpu().reshape(B, T, heads, d)
    keep = R.window_keep(SEED, SITE, B, heads, T, window, p, b0)               # (B, h, T, W)
    live = R.valid_slots(mask, window)[:, None] & keep                          # (B, h, T, W)
    want = torch.zeros(B, heads, T, d, dtype=torch.bool)
    half = window // 2
    for j in range(window):
        ch = (torch.arange(T) - half + j) % d
        want[:, :, torch.arange(T), ch] |= live[..., j]
    got = (out != 0).permute(0, 2, 1, 3)
    assert torch.equal(got, want), f'{int((got != want).sum())} of {want.numel()} keep decisions differ'
    assert 0 < int(live.sum()) < int(R.valid_slots(mask, window).sum()) * heads, 'the case both drops and keeps'
    # the kept values: scale / (number of valid keys of the row), to rounding
    n = R.valid_slots(mask, window).sum(-1).clamp(min=1).float()[:, None, :, None]
    val = torch.where(want, float(P.scale(p)) / n, torch.zeros(()))
    torch.testing.assert_close(out.permute(0, 2, 1, 3), val.expand(B, heads, T, d), rtol=1e-6, atol=0)


# ---------------------------------------------------------------------------------------------- p = 0
@pytest.mark.parametrize('B,T,C,heads,window', [(2, 37, 64, 2, 5), (2, 33, 64, 2, 19), (1, 90, 128, 2, 31), (1, 70, 128, 2, 35),
                                                (2, 45, 1024, 16, 9), (2, 30, 512, 8, 19)])
def test_p_zero_gives_the_bits_of_the_released_exports(lib, B, T, C, heads, window):
    q, k, v, do, mask = case(B, T, C, seed=T + C + window)
    args = cu(q, k, v, mask)
    assert same_bits(lib.fwd(*args, heads, window, 0.0, b0=3), lib.fwd0(*args, heads, window))
    args = cu(q, k, v, mask, do)
    for name, a, b in zip(('dQ', 'dK', 'dV'), lib.bwd(*args, heads, window, 0.0, b0=3), lib.bwd0(*args, heads, window)):
        assert same_bits(a, b), name


# ---------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'B%d-T%d-C%d-h%d-w%d' % s)
@pytest.mark.parametrize('p,b0', RATES)
def test_forward_matches_fp64(lib, shape, p, b0):
    B, T, C, heads, window = shape
    q, k, v, do, mask, keep, y64, y32, _, _ = refs(shape, p, b0)
    got = lib.fwd(*cu(q, k, v, mask), heads, window, p, b0).cpu()
    e_ref, e_gpu, top = float((y32.double() - y64).abs().max()), float((got.double() - y64).abs().max()), float(y64.abs().max())
    bound = max(4 * e_ref, FLOOR * top)
    print(f'AFERR fwd {shape} p{p} b0 {b0}: max|y64| {top:.3e} e_ref {e_ref:.3e} e_gpu {e_gpu:.3e} rule ratio {e_gpu / bound if bound else 0.0:.3f}')
    tol = 1e-5 / (1 - p)
    torch.testing.assert_close(got.double(), y64, rtol=tol, atol=tol)
    assert bool((got[~mask] == 0).all()), 'a padded query row is exactly 0'


# ---------------------------------------------------------------------------------------------- gradients
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'B%d-T%d-C%d-h%d-w%d' % s)
@pytest.mark.parametrize('p,b0', RATES)
def test_gradients_match_fp64(lib, shape, p, b0):
    B, T, C, heads, window = shape
    q, k, v, do, mask, keep, _, _, g64, g32 = refs(shape, p, b0)
    got = lib.bwd(*cu(q, k, v, mask, do), heads, window, p, b0)
    for name, a, b, c in zip(('dQ', 'dK', 'dV'), got, g64, g32):
        check(f'drop op {shape} p{p} b0 {b0} {name}', a, b, c)
        assert bool((b[~mask] == 0).all()), 'the fp64 gradient at a padded row is an exact zero'
        assert bool((a.cpu()[~mask] == 0).all()), f'{name} at a padded row is exactly 0'


# ---------------------------------------------------------------------------------------------- properties
@pytest.mark.parametrize('B,T,C,heads,window', [(2, 37, 64, 2, 5), (2, 40, 512, 8, 19), (1, 50, 64, 2, 31), (1, 50, 64, 2, 35)])
def test_null_outputs_leave_the_others_bit_identical(lib, B, T, C, heads, window):
    q, k, v, do, mask = case(B, T, C, seed=23)
    args = cu(q, k, v, mask, do)
    full = lib.bwd(*args, heads, window, 0.5, 3)
    for skip in range(3):
        want = tuple(i != skip for i in range(3))
        part = lib.bwd(*args, heads, window, 0.5, 3, want=want)
        for i in range(3):
            assert (part[i] is None) if i == skip else same_bits(part[i], full[i]), (skip, i)
    only_q = lib.bwd(*args, heads, window, 0.5, 3, want=(True, False, False))
    assert same_bits(only_q[0], full[0])
    none = lib.bwd(*args, heads, window, 0.5, 3, want=(False, False, False))
    assert none == [None, None, None]


@pytest.mark.parametrize('B,T,C,heads,window', [(3, 130, 256, 4, 9), (2, 70, 128, 2, 35)])
def test_ten_repeats_are_bit_identical(lib, B, T, C, heads, window):
    q, k, v, do, mask = case(B, T, C, seed=21)
    args = cu(q, k, v, mask, do)
    first = None
    for _ in range(10):
        got = [lib.fwd(*args[:4], heads, window, 0.1)] + lib.bwd(*args, heads, window, 0.1)
        if first is None:
            first = got
        else:
            assert all(same_bits(a, b_) for a, b_ in zip(first, got))


@pytest.mark.parametrize('B,T,C,heads,window', [(5, 37, 64, 2, 5), (5, 33, 64, 2, 19), (5, 40, 128, 2, 35), (5, 21, 512, 8, 9)])
def test_b0_rule_bit_for_bit(lib, B, T, C, heads, window):
    """sequence b of a call with b0 = n has the bits of sequence b + n of a call on the larger batch with b0 = 0"""
    q, k, v, do, mask = case(B, T, C, seed=7)
    n = 3
    whole = [lib.fwd(*cu(q, k, v, mask), heads, window, 0.5)] + lib.bwd(*cu(q, k, v, mask, do), heads, window, 0.5)
    tail = [z[n:].contiguous() for z in (q, k, v, mask, do)]
    part = [lib.fwd(*cu(*tail[:4]), heads, window, 0.5, b0=n)] + lib.bwd(*cu(*tail), heads, window, 0.5, b0=n)
    for name, a, b in zip(('O', 'dQ', 'dK', 'dV'), whole, part):
        assert same_bits(a[n:], b), name
    shifted = lib.fwd(*cu(*tail[:4]), heads, window, 0.5, b0=0)
    assert not same_bits(shifted, part[0]), 'b0 moves the stream'


def test_a_fully_dropped_row_and_head_gives_exact_zeros(lib):
    B, T, C, heads, window, p = 2, 37, 64, 2, 5, 0.5
    d = C // heads
    q, k, v, do, mask = case(B, T, C, seed=3)
    keep = R.window_keep(SEED, SITE, B, heads, T, window, p)
    valid = R.valid_slots(mask, window)[:, None].expand_as(keep)
    dead = (valid.any(-1) & ~(valid & keep).any(-1)).permute(0, 2, 1)           # (B, T, h): a live row with every valid key dropped
    assert int(dead.sum()) >= 2, 'the key of this test must produce such rows'
    out = lib.fwd(*cu(q, k, v, mask), heads, window, p).cpu().reshape(B, T, heads, d)
    dq, dk, dv = lib.bwd(*cu(q, k, v, mask, do), heads, window, p)
    assert bool((out[dead].view(torch.int32) == 0).all()), 'O = +0 exactly (the sign bit included)'
    assert bool((dq.cpu().reshape(B, T, heads, d)[dead] == 0).all())
    # it contributes exact zeros: with dO zeroed at every other (row, head) nothing is left of dK and dV
    only = torch.where(dead[..., None], do.reshape(B, T, heads, d), torch.zeros(())).reshape(B, T, C)
    _, dk, dv = lib.bwd(*cu(q, k, v, mask, only), heads, window, p)
    assert bool((dk == 0).all()) and bool((dv == 0).all())
    g64 = R.window_attention_drop_grads(q.double(), k.double(), v.double(), mask, only.double(), heads, window, keep, p)
    assert all(float(g.abs().max()) == 0.0 for g in g64)


def test_refusals_come_before_any_launch(lib):
    q, k, v, do, mask = cu(*case(1, 8, 64, seed=1))
    with pytest.raises(RuntimeError, match='window = 0'):                       # the global form has a backward export of its own
        lib.bwd(q, k, v, mask, do, 2, 0, 0.1, 0)
    with pytest.raises(RuntimeError, match='head dimension'):                   # window = 0 in the forward: the limits of the global core
        lib.fwd(q, k, v, mask, 4, 0, 0.1, 0)
    for kw, word in ((dict(window=4), 'odd'), (dict(p=1.0), 'outside [0, 1)'), (dict(p=-0.1), 'outside [0, 1)'),
                     (dict(b0=-1), 'b0'), (dict(heads=3), 'divisible')):
        a = dict(heads=2, window=9, p=0.1, b0=0)
        a.update(kw)
        with pytest.raises(RuntimeError, match=word.replace('[', r'\[').replace(')', r'\)')):
            lib.fwd(q, k, v, mask, a['heads'], a['window'], a['p'], a['b0'])
        with pytest.raises(RuntimeError, match=word.replace('[', r'\[').replace(')', r'\)')):
            lib.bwd(q, k, v, mask, do, a['heads'], a['window'], a['p'], a['b0'])
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- autograd
def test_window_attention_function_with_map_dropout(lib):
    shape, (p, b0) = SHAPES[0], RATES[1]
    B, T, C, heads, window = shape
    q, k, v, do, mask, keep, y64, _, g64, g32 = refs(shape, p, b0)
    A = lib.pkg.autograd
    drop = A.DropSpec(SEED, b0, group=2, layer=1, attn_p=p)
    assert drop.site(A.DROP_ATTN) == SITE and drop.active
    qc, kc, vc = (z.cuda().requires_grad_(True) for z in (q, k, v))
    out = A.window_attention(qc, kc, vc, mask.cuda(), heads, window, drop=drop)
    assert same_bits(out.detach(), lib.fwd(*cu(q, k, v, mask), heads, window, p, b0))
    (out * do.cuda()).sum().backward()
    want = lib.bwd(*cu(q, k, v, mask, do), heads, window, p, b0)
    for name, z, w_, b, c in zip(('q', 'k', 'v'), (qc, kc, vc), want, g64, g32):
        assert same_bits(z.grad, w_), name
        check(f'window_attention drop {name}.grad', z.grad, b, c)
    # attn_p = 0 launches what it launches without a DropSpec
    plain = A.window_attention(q.cuda(), k.cuda(), v.cuda(), mask.cuda(), heads, window)
    for spec in (A.DropSpec(SEED, b0, proj_p=0.3, group=2, layer=1), A.DropSpec(SEED), None):
        assert same_bits(A.window_attention(q.cuda(), k.cuda(), v.cuda(), mask.cuda(), heads, window, drop=spec), plain)
    # needs_input_grad: an input that does not require grad gets None, the others keep their bits
    q2, v2 = q.cuda().requires_grad_(True), v.cuda().requires_grad_(True)
    (A.window_attention(q2, k.cuda(), v2, mask.cuda(), heads, window, drop=drop) * do.cuda()).sum().backward()
    assert same_bits(q2.grad, qc.grad) and same_bits(v2.grad, vc.grad)


@pytest.mark.parametrize('window', [9, 19])
def test_masked_mha_with_map_dropout_matches_the_restatement(lib, window):
    pkg = lib.pkg
    A = pkg.autograd
    B, T, E, heads, p, b0 = 2, 40, 64, 2, 0.25, 1
    gen = torch.Generator().manual_seed(window)
    torch.manual_seed(window)
    mha = pkg.modeling.MaskedMHA(E, n_heads=heads, window_size=window)
    sd = {n: t.detach().clone() for n, t in mha.state_dict().items()}
    x = torch.randn(B, T, E, generator=gen)
    up = torch.randn(B, T, E, generator=gen) * 1e-3
    mask = torch.ones(B, T, dtype=torch.bool)
    mask[1, 29:] = False
    drop = A.DropSpec(SEED, b0, group=3, layer=2, attn_p=p)
    keep = R.window_keep(SEED, drop.site(A.DROP_ATTN), B, heads, T, window, p, b0)

    def ref(dtype):
        xs = x.to(dtype).clone().requires_grad_(True)
        ps = {n: t.to(dtype).requires_grad_(True) for n, t in sd.items()}
        y = R.masked_mha_drop(xs, xs, xs, mask, ps, heads, window, keep, p)
        grads = torch.autograd.grad((y * up.to(dtype)).sum(), [xs] + list(ps.values()))
        return y.detach(), grads[0], dict(zip(ps, grads[1:]))

    y64, gx64, gp64 = ref(torch.float64)
    _, gx32, gp32 = ref(torch.float32)
    mha = mha.cuda()
    xc = x.cuda().requires_grad_(True)
    out = A.masked_mha(xc, xc, xc, mask.cuda(), mha, drop=drop)
    (out * up.cuda()).sum().backward()
    tol = 1e-5 / (1 - p)
    torch.testing.assert_close(out.detach().cpu().double(), y64, rtol=tol, atol=tol)
    check(f'mha drop w{window} dX', xc.grad, gx64, gx32)
    seen = 0
    for n, par in mha.named_parameters():
        check(f'mha drop w{window} {n}', par.grad, gp64[n], gp32[n])
        seen += 1
    assert seen == 8


# ---------------------------------------------------------------------------------------------- channel dropout
@pytest.mark.parametrize('B,T,C', [(3, 1, 4), (2, 17, 36), (5, 40, 512)])
@pytest.mark.parametrize('p,b0', RATES)
def test_channel_dropout_is_the_philox_stream_bit_for_bit(lib, B, T, C, p, b0):
    l, L = lib.l, lib.L
    site = P.site(R.DROP_G_INPUT, 0, R.DROP_CHANNEL)
    gen = torch.Generator().manual_seed(B + T + C)
    x = torch.randn(B, T, C, generator=gen)
    x[0, 0, 0] = float('inf')                                                   # a dropped element is +0 whatever X holds
    keep = R.channel_keep(SEED, site, B, C, p, b0)
    want = R.channel_dropout(x, keep, p)
    xc = x.cuda()
    y = torch.full_like(xc, float('nan'))
    l.check(L.dcf_op_channel_dropout(l.ptr(xc), l.ptr(y), B, T, C, b0, Lib.key(SEED), site, p, l.current_stream()), 'dcf_op_channel_dropout')
    assert same_bits(y.cpu(), want)
    if B * C >= 64:
        assert bool(keep.any()) and not bool(keep.all())
    l.check(L.dcf_op_channel_dropout(l.ptr(xc), l.ptr(xc), B, T, C, b0, Lib.key(SEED), site, p, l.current_stream()), 'dcf_op_channel_dropout')
    assert same_bits(xc.cpu(), want), 'Y may alias X'
    # the autograd function: the same bits, and the backward is the same operator on the gradient
    A = lib.pkg.autograd
    drop = A.DropSpec(SEED, b0, proj_p=p, group=A.DROP_G_INPUT)
    xs = torch.randn(B, T, C, generator=gen)
    xg = xs.cuda().requires_grad_(True)
    out = A.channel_dropout(xg, drop)
    assert same_bits(out.detach().cpu(), R.channel_dropout(xs, keep, p))
    up = torch.randn(B, T, C, generator=gen)
    (out * up.cuda()).sum().backward()
    assert same_bits(xg.grad.cpu(), R.channel_dropout(up, keep, p))
    assert A.channel_dropout(xg, A.DropSpec(SEED, b0, group=A.DROP_G_INPUT)) is xg


# ---------------------------------------------------------------------------------------------- against the reference
@pytest.mark.parametrize('name', ['w9', 'w19'])
def test_masked_mha_with_map_dropout_matches_the_reference_backward(lib, name):
    """tests/golden/attn_drop_ops.npz: the reference's own MaskedMHA with attn_pdrop 0.25 under the stated stream, its fp64 `backward()`
    as g_64 and its fp32 `backward()` for e_ref; the output to the forward tolerance"""
    from test_attn_drop_cpu import ops_case
    pkg = lib.pkg
    A = pkg.autograd
    x, mask, sd, up, heads, window, p, key, site, keep, g = ops_case(name, torch.float32)
    meta = g.js('meta')
    mha = pkg.modeling.MaskedMHA(x.size(-1), n_heads=heads, window_size=window)
    mha.load_state_dict(sd)
    mha = mha.cuda()
    drop = A.DropSpec(key, 0, group=meta['group'], layer=meta['layer'], attn_p=p)
    assert drop.site(A.DROP_ATTN) == site
    xc = x.cuda().requires_grad_(True)
    out = A.masked_mha(xc, xc, xc, mask.cuda(), mha, drop=drop)
    (out * up.cuda()).sum().backward()
    tol = 1e-5 / (1 - p)
    torch.testing.assert_close(out.detach().cpu().transpose(1, 2).double(), g.t(f'{name}/out64'), rtol=tol, atol=tol)
    check(f'ref mha drop {name} dX', xc.grad.transpose(1, 2), g.t(f'{name}/gx64'), g.t(f'{name}/gx32'))
    seen = 0
    for k, par in mha.named_parameters():
        check(f'ref mha drop {name} {k}', par.grad, g.t(f'{name}/gp64/{k}'), g.t(f'{name}/gp32/{k}'))
        seen += 1
    assert seen == 8
