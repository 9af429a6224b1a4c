"""GPU checks of the backward of the sliding-window attention core (csrc/attn_grad.hip: dcf_op_local_attn_bwd) and of the autograd
functions over it (autograd.window_attention, autograd.masked_mha).

The yardstick is the project's gradient rule (tests/test_gpu_objective_grad.py, test_gpu_conv_grad.py), per gradient tensor:

    e_gpu <= max(4 * e_ref, 2^-21 * max |g_64|),   e = max |g - g_64|

with g_64 fp64 autograd through the oracle's banded attention (the reference's fp64 `backward()` for the fixture) and e_ref the error
of the same in fp32 on the CPU (the reference's fp32 `backward()` for the fixture).  Every check prints an `AGERR` line; the worst per
case are in profiles/attn_grad.md.

In the operator cases q, k, v ~ N(0, 1), dO ~ 1e-3 N(0, 1) on EVERY row, padded ones included, and masks have holes.

key.bias of the fixture: a constant added to every key moves all scores of a row alike, so this gradient is 0 in exact arithmetic
and g_64, g_32 and the GPU's result are three different roundings of 0 (1e-16, 1e-7, 1e-7 of key.weight's gradient).  The rule is
applied to it as to every other tensor.

Measured on an MI355X (profiles/attn_grad.md): operator cases at most 0.45 of the bound (dQ at B 4, T 63, window 19), the seam case
0.47 (dK), the composed MaskedMHA at most 0.31 (key.bias, window 19); one-row sequences give exact zeros in dQ and dK.
"""
import pytest
import torch

from conftest import load_pkg
import attn_grad_ref as R
from test_attn_grad_cpu import banded, banded_grads, holes, mha_fixture

pytestmark = pytest.mark.gpu
FLOOR = 2.0 ** -21
E2E_TOL = dict(rtol=2e-4, atol=2e-4)          # what tests/test_gpu_e2e.py used before its gates moved to the rule


def check(tag, got, g64, g32):
    got, g64, g32 = got.detach().cpu().double(), g64.detach().double(), g32.detach().double()
    assert got.shape == g64.shape == g32.shape, (tag, got.shape, g64.shape, g32.shape)
    assert bool(torch.isfinite(got).all()), tag
    e_ref, e_gpu, top = float((g32 - g64).abs().max()), float((got - g64).abs().max()), float(g64.abs().max())
    bound = max(4 * e_ref, FLOOR * top)
    print(f'AGERR {tag}: max|g64| {top:.3e} e_ref {e_ref:.3e} e_gpu {e_gpu:.3e} bound {bound:.3e} ratio {e_gpu / bound if bound else 0.0:.3f}')
    assert e_gpu <= bound, (tag, e_gpu, bound)
    return bound


class Lib:
    def __init__(self):
        self.pkg = load_pkg()
        self.L, self.l = self.pkg._lib.lib(), self.pkg._lib

    def bwd(self, q, k, v, mask, do, heads, window, want=(True, True, True)):
        """(dQ, dK, dV) of device tensors; outputs pre-filled with NaN, None where not wanted"""
        B, T, C = q.shape
        l = self.l
        outs = [torch.full_like(q, float('nan')) if w else None for w in want]
        l.check(self.L.dcf_op_local_attn_bwd(l.ptr(q), l.ptr(k), l.ptr(v), l.ptr(mask), l.ptr(do), l.ptr(outs[0]), l.ptr(outs[1]), l.ptr(outs[2]),
                                             B, T, C, heads, window, l.current_stream()), 'dcf_op_local_attn_bwd')
        return outs

    def fwd(self, q, k, v, mask, heads, window):
        B, T, C = q.shape
        l = self.l
        o = torch.full_like(q, float('nan'))
        l.check(self.L.dcf_op_local_attn(l.ptr(q), l.ptr(k), l.ptr(v), l.ptr(mask), l.ptr(o), B, T, C, heads, window, l.current_stream()),
                'dcf_op_local_attn')
        return o


@pytest.fixture(scope='module')
def lib():
    return Lib()


def case(B, T, C, seed, masked=True):
    gen = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(B, T, C, generator=gen) for _ in range(3))
    do = torch.randn(B, T, C, generator=gen) * 1e-3           # every row, padded ones too
    mask = holes(B, T, gen) if masked else torch.ones(B, T, dtype=torch.bool)
    return q, k, v, do, mask


def refs(q, k, v, mask, do, heads, window):
    """((dQ, dK, dV) by fp64 autograd through the banded oracle, the same in fp32)"""
    return banded_grads(q.double(), k.double(), v.double(), mask, do.double(), heads, window), banded_grads(q, k, v, mask, do, heads, window)


def cu(*ts):
    return [t.cuda() for t in ts]


# the forward's own list (tests/test_gpu_ops.py::test_local_attn_core), then an odd length (63) at window 19 and many
# workgroups at window 9.  The launcher picks its variant by window (<= 9, <= 19, wider) and by C (<= 256 or not), never by row count.
CASES = [(2, 72, 32, 4, 9), (1, 256, 256, 4, 9), (2, 64, 128, 4, 5), (1, 90, 64, 2, 19), (1, 8, 256, 4, 9), (1, 4, 128, 4, 5), (3, 7, 256, 4, 9),
         (2, 33, 64, 2, 19), (1, 150, 256, 4, 71), (2, 45, 1024, 16, 9), (4, 63, 256, 4, 19), (3, 1100, 256, 4, 9)]


@pytest.mark.parametrize('B,T,C,heads,window', CASES)
def test_gradients_match_fp64(lib, B, T, C, heads, window):
    q, k, v, do, mask = case(B, T, C, seed=T * 3 + C + window)
    g64, g32 = refs(q, k, v, mask, do, heads, window)
    got = lib.bwd(*cu(q, k, v, mask, do), heads, window)
    tag = f'op B{B} T{T} C{C} h{heads} w{window}'
    for name, a, b, c in zip(('dQ', 'dK', 'dV'), got, g64, g32):
        check(f'{tag} {name}', a, b, c)
        assert bool((b[~mask] == 0).all()), 'the fp64 gradient at a padded row is an exact zero'
        assert bool((a.cpu()[~mask] == 0).all()), f'{name} at a padded row is exactly 0'


def test_one_row_sequences(lib):
    """T = 1: the softmax is over one key, dS = 0, so dQ = dK = 0 exactly (the bound is 0); dV = dO goes by the rule"""
    B, T, C, heads, window = 2, 1, 256, 4, 9
    q, k, v, do, mask = case(B, T, C, seed=17, masked=False)
    g64, g32 = refs(q, k, v, mask, do, heads, window)
    assert float(g64[0].abs().max()) == 0.0 and float(g64[1].abs().max()) == 0.0
    dq, dk, dv = lib.bwd(*cu(q, k, v, mask, do), heads, window)
    assert bool((dq == 0).all()) and bool((dk == 0).all())
    check('one-row dV', dv, g64[2], g32[2])
    dq, dk, dv = lib.bwd(*cu(q, k, v), None, do.cuda(), heads, window)          # NULL mask = every row valid
    assert bool((dq == 0).all()) and bool((dk == 0).all())
    check('one-row dV (NULL mask)', dv, g64[2], g32[2])


@pytest.mark.parametrize('B,T,C,heads,window', [(2, 72, 64, 4, 9), (2, 40, 512, 8, 19), (1, 50, 64, 2, 31)])
def test_null_outputs_leave_the_others_bit_identical(lib, B, T, C, heads, window):
    q, k, v, do, mask = case(B, T, C, seed=23)
    args = cu(q, k, v, mask, do)
    full = lib.bwd(*args, heads, window)
    for skip in range(3):
        want = tuple(i != skip for i in range(3))
        part = lib.bwd(*args, heads, window, want=want)
        for i in range(3):
            assert (part[i] is None) if i == skip else torch.equal(part[i], full[i]), (skip, i)
    only_q = lib.bwd(*args, heads, window, want=(True, False, False))
    assert torch.equal(only_q[0], full[0])


def test_windows_stop_at_sequence_seams_and_masked_rows(lib):
    """rows next to a seam and one masked row hold values 100 times the rest in q, k and v: a window that crossed the seam, or a
    kernel that ignored the mask, would move the gradients by far more than the bound"""
    B, T, C, heads, window = 2, 64, 64, 4, 9
    q, k, v, do, _ = case(B, T, C, seed=5, masked=False)
    mask = torch.ones(B, T, dtype=torch.bool)
    mask[0, 30] = False
    for z in (q, k, v):
        z[0, T - 1] *= 100
        z[1, 0] *= 100
        z[0, 30] *= 100
    g64, g32 = refs(q, k, v, mask, do, heads, window)
    got = lib.bwd(*cu(q, k, v, mask, do), heads, window)
    bounds = [check(f'seam {n}', a, b, c) for n, a, b, c in zip(('dQ', 'dK', 'dV'), got, g64, g32)]
    one = lambda z: z.double().reshape(1, B * T, C)
    wrong_seam = R.window_attention_grads(one(q), one(k), one(v), mask.reshape(1, B * T), one(do), heads, window)
    wrong_mask = R.window_attention_grads(q.double(), k.double(), v.double(), None, do.double(), heads, window)
    for wrong in (wrong_seam, wrong_mask):
        for w_, g_, bound in zip(wrong, g64, bounds):
            assert float((w_.reshape(B, T, C) - g_).abs().max()) > 100 * bound


def test_power_of_two_scaling_of_dO_commutes_bit_for_bit(lib):
    B, T, C, heads, window = 2, 200, 256, 4, 9
    q, k, v, do, mask = case(B, T, C, seed=11)
    outs = []
    for s in (2.0 ** -30, 1.0, 2.0 ** 10):
        outs.append([g.cpu() / s for g in lib.bwd(*cu(q, k, v, mask, do * s), heads, window)])
    for a, b_, c in zip(*outs):
        assert torch.equal(a, b_) and torch.equal(b_, c)


def test_ten_repeats_are_bit_identical(lib):
    B, T, C, heads, window = 3, 1100, 256, 4, 9
    q, k, v, do, mask = case(B, T, C, seed=21)
    args = cu(q, k, v, mask, do)
    first = None
    for _ in range(10):
        got = [g.clone() for g in lib.bwd(*args, heads, window)]
        if first is None:
            first = got
        else:
            assert all(torch.equal(a, b_) for a, b_ in zip(first, got))


def test_window_attention_function(lib):
    B, T, C, heads, window = 2, 72, 128, 4, 9
    q, k, v, do, mask = case(B, T, C, seed=31)
    g64, g32 = refs(q, k, v, mask, do, heads, window)
    A = lib.pkg.autograd
    qc, kc, vc = (z.cuda().requires_grad_(True) for z in (q, k, v))
    out = A.window_attention(qc, kc, vc, mask.cuda(), heads, window)
    assert torch.equal(out.detach(), lib.fwd(*cu(q, k, v, mask), heads, window))
    torch.testing.assert_close(out.detach().cpu(), banded(q, k, v, mask, heads, window), rtol=1e-5, atol=1e-5)
    (out * do.cuda()).sum().backward()
    for name, z, b, c in zip(('q', 'k', 'v'), (qc, kc, vc), g64, g32):
        check(f'window_attention {name}.grad', z.grad, b, c)
    # needs_input_grad: an input that does not require grad gets None (its output is not computed), the others keep their bits
    q2, k2, v2 = q.cuda().requires_grad_(True), k.cuda(), v.cuda().requires_grad_(True)
    out2 = A.window_attention(q2, k2, v2, mask.cuda(), heads, window)
    (out2 * do.cuda()).sum().backward()
    assert k2.grad is None and torch.equal(q2.grad, qc.grad) and torch.equal(v2.grad, vc.grad)
    k3 = k.cuda().requires_grad_(True)
    out3 = A.window_attention(q.cuda(), k3, v.cuda(), mask.cuda(), heads, window)
    (out3 * do.cuda()).sum().backward()
    assert torch.equal(k3.grad, kc.grad)


@pytest.mark.parametrize('name', ['w9', 'w19'])
def test_masked_mha_matches_the_reference_backward(lib, name):
    pkg = lib.pkg
    x, mask, sd, up, heads, window, g = mha_fixture(name, torch.float32)
    mha = pkg.modeling.MaskedMHA(x.size(-1), n_heads=heads, window_size=window)
    mha.load_state_dict(sd)
    mha = mha.cuda()
    xc = x.cuda().requires_grad_(True)
    out = pkg.autograd.masked_mha(xc, xc, xc, mask.cuda(), mha)
    (out * up.cuda()).sum().backward()
    torch.testing.assert_close(out.detach().cpu().transpose(1, 2), g.t(f'{name}/out32'), **E2E_TOL)
    check(f'mha {name} dX', xc.grad.transpose(1, 2), g.t(f'{name}/gx64'), g.t(f'{name}/gx32'))
    seen = 0
    for k, p in mha.named_parameters():
        check(f'mha {name} {k}', p.grad, g.t(f'{name}/gp64/{k}'), g.t(f'{name}/gp32/{k}'))
        seen += 1
    assert seen == 8


def test_attention_trains_through_heads_and_the_point_objective(lib):
    from test_conv_grad_cpu import fixture_case
    from test_gpu_conv_grad import make_head
    pkg = lib.pkg
    B, T, L, E = 2, 64, 3, 64
    gen = torch.Generator().manual_seed(3)
    torch.manual_seed(4)
    mha = pkg.modeling.MaskedMHA(E, n_heads=4, window_size=9).cuda()
    cls1, cls2 = (make_head(pkg, 'cls', fixture_case('cls', torch.float32)[2]) for _ in range(2))
    reg = make_head(pkg, 'reg', fixture_case('reg', torch.float32)[2])
    masks = [(torch.arange(T >> l)[None] < torch.tensor([T >> l, (T * 3 // 4) >> l])[:, None]).cuda() for l in range(L)]
    A = pkg.autograd
    xs = []
    for l in range(L):
        x = torch.randn(B, T >> l, E, generator=gen).cuda()
        xs.append(x + A.masked_mha(x, x, x, masks[l], mha))
    outputs = (tuple(A.conv_head(x, m, cls1) for x, m in zip(xs, masks)), tuple(A.conv_head(x, m, cls2) for x, m in zip(xs, masks)),
               tuple(A.conv_head(x, m, reg, level=l) for l, (x, m) in enumerate(zip(xs, masks))), tuple(masks))
    obj = pkg.loss.PointObjective(pkg.config.make_opt(n_levels=L, max_seq_len=T))
    total = obj(outputs, torch.tensor([[10.0, 30.5], [3.0, 20.0]]).cuda())['total']
    assert bool(torch.isfinite(total))
    total.backward()
    for name in ('query', 'key', 'value', 'proj'):
        gr = getattr(mha, name).weight.grad
        assert gr is not None and bool(torch.isfinite(gr).all()) and float(gr.abs().max()) > 0, name
