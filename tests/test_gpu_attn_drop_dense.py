"""GPU checks of dropout on the map of global self attention (dcf_op_local_attn_drop with window = 0, dcf_op_global_attn_drop_bwd)
and of cross attention (dcf_op_xattn_drop, dcf_op_xattn_drop_bwd), csrc/attn_drop.hip, and of the autograd functions over them.  The
checks, inputs, rates and bounds are those of tests/test_gpu_attn_drop.py; the restatement is ``attn_drop_ref.dense_attention_drop``.

Shapes: global (B, T, C, heads) (2, 1, 64, 2), (2, 63, 64, 2), (1, 70, 256, 4), (2, 130, 64, 1), and a sequence without a valid key,
which gives zeros; cross (B, T, Lk, C, heads) (2, 50, 1, 64, 4), (3, 70, 24, 128, 4), (2, 33, 5, 256, 2), (1, 520, 64, 256, 4).  The
kernels take one path at p > 0 (blocks of 32 keys: Lk 1, 5, 24, 63 / 64, 70 and 130 are below, at and above one and several blocks)."""
import pytest
import torch

import attn_drop_ref as R
import philox_ref as P
from conftest import load_pkg
from test_gpu_attn_drop import FLOOR, RATES, SEED, Lib, same_bits
from test_gpu_attn_grad import check, cu

pytestmark = pytest.mark.gpu
SITE = P.site(1, 1, R.DROP_ATTN)
GLOBAL = [(2, 1, 64, 2), (2, 63, 64, 2), (1, 70, 256, 4), (2, 130, 64, 1)]
CROSS = [(2, 50, 1, 64, 4), (3, 70, 24, 128, 4), (2, 33, 5, 256, 2), (1, 520, 64, 256, 4)]
CASES = [('global',) + s[:2] + (s[1],) + s[2:] for s in GLOBAL] + [('cross',) + s for s in CROSS]     # (kind, B, T, Lk, C, heads)
IDS = ['%s-B%d-T%d-Lk%d-C%d-h%d' % c for c in CASES]


class Dense(Lib):
    def fwd(self, kind, q, k, v, mask, heads, p, b0=0):
        B, T, C = q.shape
        l, tail = self.l, (b0, self.key(SEED), SITE, p, self.l.current_stream())
        o = torch.full_like(q, float('nan'))
        if kind == 'global':
            l.check(self.L.dcf_op_local_attn_drop(l.ptr(q), l.ptr(k), l.ptr(v), l.ptr(mask), l.ptr(o), B, T, C, heads, 0, *tail), 'global fwd')
        else:
            l.check(self.L.dcf_op_xattn_drop(l.ptr(q), l.ptr(k), l.ptr(v), l.ptr(mask), l.ptr(o), B, T, k.size(1), C, heads, *tail), 'xattn fwd')
        return o

    def bwd(self, kind, q, k, v, mask, do, heads, p, b0=0, want=(True, True, True)):
        B, T, C = q.shape
        l, tail = self.l, (b0, self.key(SEED), SITE, p, self.l.current_stream())
        outs = [torch.full_like(z, float('nan')) if w else None for z, w in zip((q, k, v), want)]
        ptrs = (l.ptr(q), l.ptr(k), l.ptr(v), l.ptr(mask), l.ptr(do), l.ptr(outs[0]), l.ptr(outs[1]), l.ptr(outs[2]))
        if kind == 'global':
            l.check(self.L.dcf_op_global_attn_drop_bwd(*ptrs, B, T, C, heads, *tail), 'global bwd')
        else:
            l.check(self.L.dcf_op_xattn_drop_bwd(*ptrs, B, T, k.size(1), C, heads, *tail), 'xattn bwd')
        return outs

    def released(self, kind, q, k, v, mask, do, heads):
        B, T, C = q.shape
        l, st = self.l, self.l.current_stream()
        o = torch.full_like(q, float('nan'))
        g = [torch.full_like(z, float('nan')) for z in (q, k, v)]
        if kind == 'global':
            l.check(self.L.dcf_op_local_attn(l.ptr(q), l.ptr(k), l.ptr(v), l.ptr(mask), l.ptr(o), B, T, C, heads, 0, st), 'fwd0')
            l.check(self.L.dcf_op_global_attn_bwd(l.ptr(q), l.ptr(k), l.ptr(v), l.ptr(mask), l.ptr(do), l.ptr(g[0]), l.ptr(g[1]), l.ptr(g[2]), B, T, C,
                                                  heads, st), 'bwd0')
        else:
            Lk = k.size(1)
            l.check(self.L.dcf_op_xattn(l.ptr(q), l.ptr(k), l.ptr(v), l.ptr(mask), l.ptr(o), B, T, Lk, C, heads, st), 'fwd0')
            l.check(self.L.dcf_op_xattn_bwd(l.ptr(q), l.ptr(k), l.ptr(v), l.ptr(mask), l.ptr(do), l.ptr(g[0]), l.ptr(g[1]), l.ptr(g[2]), B, T, Lk, C,
                                            heads, st), 'bwd0')
        return [o] + g


@pytest.fixture(scope='module')
def lib():
    return Dense()


def key_mask(B, Lk, gen):
    """a hole in every sequence that can spare one, a padded tail in the odd ones; every sequence keeps a valid key"""
    m = torch.ones(B, Lk, dtype=torch.bool)
    if Lk > 2:
        m[:, int(torch.randint(1, Lk - 1, (1,), generator=gen))] = False
    for b in range(1, B, 2):
        m[b, Lk - Lk // 4:] = False
    return m


def inputs(kind, B, T, Lk, C, seed):
    gen = torch.Generator().manual_seed(seed)
    q = torch.randn(B, T, C, generator=gen)
    k, v = (torch.randn(B, Lk, C, generator=gen) for _ in range(2))
    do = torch.randn(B, T, C, generator=gen) * 1e-3
    return q, k, v, do, key_mask(B, Lk, gen)


REFS = {}


def refs(case, p, b0):
    if (case, p, b0) not in REFS:
        kind, B, T, Lk, C, heads = case
        q, k, v, do, mask = inputs(kind, B, T, Lk, C, T * 3 + C + Lk)
        keep = R.dense_keep(SEED, SITE, B, heads, T, Lk, p, b0)
        d = lambda z: z.double()
        REFS[(case, p, b0)] = (q, k, v, do, mask, keep, R.dense_attention_drop(d(q), d(k), d(v), mask, heads, keep, p),
                               R.dense_attention_drop(q, k, v, mask, heads, keep, p),
                               R.dense_attention_drop_grads(d(q), d(k), d(v), mask, d(do), heads, keep, p),
                               R.dense_attention_drop_grads(q, k, v, mask, do, heads, keep, p))
    return REFS[(case, p, b0)]


@pytest.mark.parametrize('kind,B,T,Lk,C,heads', [('global', 2, 30, 30, 64, 2), ('cross', 2, 40, 24, 128, 4)])
@pytest.mark.parametrize('p,b0', RATES)
def test_keep_bits_are_the_philox_stream(lib, kind, B, T, Lk, C, heads, p, b0):
    """q = k = 0: the map is uniform over the valid keys; v row j is the unit vector of channel j of each head (Lk <= d)"""
    d = C // heads
    assert Lk <= d
    mask = key_mask(B, Lk, torch.Generator().manual_seed(Lk))
    q, kz = torch.zeros(B, T, C), torch.zeros(B, Lk, C)
    v = torch.zeros(B, Lk, heads, d)
    v[:, torch.arange(Lk), :, torch.arange(Lk)] = 1.0
    out = lib.fwd(kind, *cu(q, kz, v.reshape(B, Lk, C), mask), heads, p, b0).cpu().reshape(B, T, heads, d)
    keep = R.dense_keep(SEED, SITE, B, heads, T, Lk, p, b0) & mask[:, None, None, :]
    want = torch.zeros(B, heads, T, d, dtype=torch.bool)
    want[..., :Lk] = keep
    got = (out != 0).permute(0, 2, 1, 3)
    assert torch.equal(got, want), f'{int((got != want).sum())} of {want.numel()} keep decisions differ'
    assert 0 < int(keep.sum()) < int(mask.sum()) * heads * T


@pytest.mark.parametrize('case', [CASES[1], CASES[3], CASES[5], CASES[7]], ids=[IDS[1], IDS[3], IDS[5], IDS[7]])
def test_p_zero_gives_the_bits_of_the_released_exports(lib, case):
    kind, B, T, Lk, C, heads = case
    q, k, v, do, mask = cu(*inputs(kind, B, T, Lk, C, 9))
    got = [lib.fwd(kind, q, k, v, mask, heads, 0.0, 3)] + lib.bwd(kind, q, k, v, mask, do, heads, 0.0, 3)
    for name, a, b in zip(('O', 'dQ', 'dK', 'dV'), got, lib.released(kind, q, k, v, mask, do, heads)):
        assert same_bits(a, b), name


@pytest.mark.parametrize('case', CASES, ids=IDS)
@pytest.mark.parametrize('p,b0', RATES)
def test_forward_and_gradients_match_fp64(lib, case, p, b0):
    kind, B, T, Lk, C, heads = case
    q, k, v, do, mask, keep, y64, y32, g64, g32 = refs(case, p, b0)
    got = lib.fwd(kind, *cu(q, k, v, mask), heads, p, b0).cpu()
    e_ref, e_gpu, top = float((y32.double() - y64).abs().max()), float((got.double() - y64).abs().max()), float(y64.abs().max())
    bound = max(4 * e_ref, FLOOR * top)
    print(f'AFERR {kind} fwd {case[1:]} p{p} b0 {b0}: max|y64| {top:.3e} e_ref {e_ref:.3e} e_gpu {e_gpu:.3e} rule ratio {e_gpu / bound if bound else 0.0:.3f}')
    tol = 1e-5 / (1 - p)
    torch.testing.assert_close(got.double(), y64, rtol=tol, atol=tol)
    grads = lib.bwd(kind, *cu(q, k, v, mask, do), heads, p, b0)
    for name, a, b, c in zip(('dQ', 'dK', 'dV'), grads, g64, g32):
        check(f'drop {kind} {case[1:]} p{p} b0 {b0} {name}', a, b, c)
    for a in grads[1:]:
        assert bool((a.cpu()[~mask] == 0).all()), 'dK and dV are exactly 0 at masked keys'


@pytest.mark.parametrize('kind', ['global', 'cross'])
def test_a_sequence_without_a_valid_key_gives_zeros(lib, kind):
    B, T, Lk, C, heads = (2, 20, 20, 64, 2) if kind == 'global' else (2, 20, 7, 64, 2)
    q, k, v, do, mask = inputs(kind, B, T, Lk, C, 4)
    mask[1] = False
    out = lib.fwd(kind, *cu(q, k, v, mask), heads, 0.5)
    grads = lib.bwd(kind, *cu(q, k, v, mask, do), heads, 0.5)
    assert bool((out[1] == 0).all()) and all(bool((g[1] == 0).all()) for g in grads)
    assert bool(out[0].any()) and all(bool(torch.isfinite(g).all()) and bool(g[0].any()) for g in grads)


@pytest.mark.parametrize('case', [CASES[2], CASES[5]], ids=[IDS[2], IDS[5]])
def test_null_outputs_repeats_and_the_b0_rule(lib, case):
    kind, _, T, Lk, C, heads = case
    B, n = 4, 3
    q, k, v, do, mask = inputs(kind, B, T, Lk, C, 23)
    args = cu(q, k, v, mask, do)
    full = lib.bwd(kind, *args, heads, 0.5)
    for skip in range(3):
        part = lib.bwd(kind, *args, heads, 0.5, want=tuple(i != skip for i in range(3)))
        for i in range(3):
            assert (part[i] is None) if i == skip else same_bits(part[i], full[i]), (skip, i)
    assert lib.bwd(kind, *args, heads, 0.5, want=(False, False, False)) == [None, None, None]
    first = [lib.fwd(kind, *args[:4], heads, 0.5)] + full
    for _ in range(9):
        again = [lib.fwd(kind, *args[:4], heads, 0.5)] + lib.bwd(kind, *args, heads, 0.5)
        assert all(same_bits(a, b) for a, b in zip(first, again))
    tail = cu(*[z[n:].contiguous() for z in (q, k, v, mask, do)])
    part = [lib.fwd(kind, *tail[:4], heads, 0.5, b0=n)] + lib.bwd(kind, *tail, heads, 0.5, b0=n)
    for name, a, b in zip(('O', 'dQ', 'dK', 'dV'), first, part):
        assert same_bits(a[n:], b), name


def test_a_fully_dropped_row_and_head_gives_exact_zeros(lib):
    kind, B, T, Lk, C, heads, p = 'cross', 3, 70, 5, 64, 4, 0.5
    q, k, v, do, mask = inputs(kind, B, T, Lk, C, 3)
    keep = R.dense_keep(SEED, SITE, B, heads, T, Lk, p) & mask[:, None, None, :]
    dead = (~keep.any(-1)).permute(0, 2, 1)                                      # (B, T, h)
    assert int(dead.sum()) >= 2
    d = C // heads
    out = lib.fwd(kind, *cu(q, k, v, mask), heads, p).cpu().reshape(B, T, heads, d)
    assert bool((out[dead].view(torch.int32) == 0).all()), 'O = +0 exactly'
    only = torch.where(dead[..., None], do.reshape(B, T, heads, d), torch.zeros(())).reshape(B, T, C)
    dq, dk, dv = lib.bwd(kind, *cu(q, k, v, mask, only), heads, p)
    assert bool((dq == 0).all()) and bool((dk == 0).all()) and bool((dv == 0).all())


def test_autograd_functions_with_map_dropout(lib):
    A = lib.pkg.autograd
    for case in (CASES[1], CASES[5]):
        kind, B, T, Lk, C, heads = case
        p, b0 = RATES[1]
        q, k, v, do, mask, keep, y64, _, g64, g32 = refs(case, p, b0)
        drop = A.DropSpec(SEED, b0, group=1, layer=1, attn_p=p)
        assert drop.site(A.DROP_ATTN) == SITE
        leaves = [z.cuda().requires_grad_(True) for z in (q, k, v)]
        fn = A.global_attention if kind == 'global' else A.cross_attention
        out = fn(*leaves, mask.cuda(), heads, drop=drop)
        assert same_bits(out.detach(), lib.fwd(kind, *cu(q, k, v, mask), heads, p, b0))
        (out * do.cuda()).sum().backward()
        for z, w in zip(leaves, lib.bwd(kind, *cu(q, k, v, mask, do), heads, p, b0)):
            assert same_bits(z.grad, w)
        plain = fn(*cu(q, k, v, mask), heads)
        assert same_bits(fn(*cu(q, k, v, mask), heads, drop=A.DropSpec(SEED, b0, proj_p=0.3)), plain)


@pytest.mark.parametrize('name', ['global', 'cross'])
def test_mha_with_map_dropout_matches_the_reference_backward(lib, name):
    """tests/golden/attn_drop_ops_dense.npz: the global branch of the reference's own MaskedMHA with attn_pdrop 0.25 under the stated
    stream -- self attention over 70 positions with a hole in the key mask, and cross attention on 24 padded keys with kv_size (2, 1) --
    its fp64 `backward()` as g_64, its fp32 `backward()` for e_ref; the output to the forward tolerance"""
    from conftest import Golden
    pkg = lib.pkg
    A = pkg.autograd
    g = Golden('attn_drop_ops_dense.npz')
    meta = g.js('meta')
    p, kv_size = meta['p'], meta['cases'][name]['kv_size']
    tm = lambda z: z.transpose(1, 2).contiguous()
    mha = pkg.modeling.MaskedMHA(meta['E'], n_heads=meta['heads'], window_size=0)
    mha.load_state_dict(g.sub('param/'))
    mha = mha.cuda()
    drop = A.DropSpec(int(meta['key']), 0, group=meta['group'], layer=meta['layer'], attn_p=p)
    assert drop.site(A.DROP_ATTN) == meta['site']
    qc = tm(g.t(f'{name}/q')).cuda().requires_grad_(True)
    mask, up = g.t(f'{name}/mask').cuda(), tm(g.t(f'{name}/up')).cuda()
    if name == 'global':
        kc, out = None, A.masked_mha(qc, qc, qc, mask, mha, drop=drop)
    else:
        kc = tm(g.t(f'{name}/kv')).cuda().requires_grad_(True)
        out = A.xattn_mha(qc, kc, mask, mha, torch.tensor(kv_size).cuda(), drop=drop)
    (out * up).sum().backward()
    tol = 1e-5 / (1 - p)
    torch.testing.assert_close(out.detach().cpu().transpose(1, 2).double(), g.t(f'{name}/out64'), rtol=tol, atol=tol)
    check(f'ref mha drop {name} dq', qc.grad.transpose(1, 2), g.t(f'{name}/gq64'), g.t(f'{name}/gq32'))
    if kc is not None:
        check(f'ref mha drop {name} dkv', kc.grad.transpose(1, 2), g.t(f'{name}/gkv64'), g.t(f'{name}/gkv32'))
    seen = 0
    for k, par in mha.named_parameters():
        check(f'ref mha drop {name} {k}', par.grad, g.t(f'{name}/gp64/{k}'), g.t(f'{name}/gp32/{k}'))
        seen += 1
    assert seen == 8
