"""GPU checks of the training extension's operators (include/decafnet_hip_train.h, csrc/drop_grad.hip): dropout, the fused
GELU + dropout pair and the residual with dropout and drop-path, forward and backward, against tests/philox_ref.py's keep bits and
the restatements of tests/step_grad_drop_ref.py.

What is exact is compared bit for bit: masks, kept values x * float32(scale), dropped values +0, the fused pair against the
two-operator chains it replaces, the residual's forward against its stated fp32 evaluation, dR, the rows of a dropped sample, and
everything at p = 0 against dcf_op_layerscale_residual(_bwd).  dH and dls meet the project's gradient rule (one `DGERR` line each):

    e_gpu <= max(4 e_ref, 2^-21 max |g_64|),   e = max |g - g_64|,   e_ref the fp32 restatement's error

Every call runs twice and must give equal bits.  Shapes (B, T, C, b0): T % 4 == 0 and != 0, C no multiple of the 256-channel chunk,
a tiny one, rows that span several reduction slices (B T = 1032: 258 workgroup partials, more than one group of 64 in k_eg_reduce), an
element index past 2^32, and the FFN's widest hidden tensor for the fused pair."""
import numpy as np
import pytest
import torch

from conftest import load_pkg
import philox_ref as P
import step_grad_drop_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(2, 8, 8, 0), (3, 10, 36, 5), (1, 3, 4, 2), (2, 516, 64, 1), (2, 68, 64, 2 ** 20 + 1)]
GELU_SHAPES = SHAPES + [(2, 12, 4096, 0)]
RATES = [0.1, 0.5]
SITE_DROP, SITE_PATH = P.site(P.G_BRANCH, 1, P.FFN_OUT), P.site(P.G_BRANCH, 1, P.PATH_FFN)
ids = lambda s: 'x'.join(str(v) for v in s)


@pytest.fixture(scope='module')
def pkg():
    return load_pkg()


def i64(seed):
    """the 64-bit key as the int64 the ABI takes"""
    return seed - (1 << 64) if seed >= 1 << 63 else seed


def pick_seed(B, b0, p_path, start=0x9E3779B97F4A7C15):
    """a key under which the drop-path site drops a sample and, where B > 1, keeps one"""
    seed = start
    for _ in range(256):
        k = R.keep_paths(seed, SITE_PATH, B, b0, p_path)
        if not bool(k.all()) and (B == 1 or bool(k.any())):
            return seed
        seed = (seed * 6364136223846793005 + 1442695040888963407) & ((1 << 64) - 1)
    raise AssertionError('no key found')


def rows_mask(B, T):
    """(B, T) uint8: sequence 0 full, the others with a padded tail"""
    m = torch.ones(B, T, dtype=torch.uint8)
    for b in range(1, B):
        m[b, T - (T // 3 + b):] = 0
    if B == 1 and T > 2:
        m[0, T - 1:] = 0
    return m


def bits(t):
    return t.detach().cpu().contiguous().view(-1).view(torch.int32)


def same(a, b):
    return torch.equal(bits(a), bits(b))


class Ops:
    def __init__(self, pkg):
        self.L, self.lib = pkg._lib, pkg._lib.lib()

    def _run(self, name, fn):
        """twice: equal bits from run to run"""
        a = fn()
        b = fn()
        torch.cuda.synchronize()
        for x, y in zip(a, b):
            assert (x is None) == (y is None) and (x is None or same(x, y)), f'{name}: two runs differ'
        return a

    def dropout(self, x, geom, seed, site, p, inplace=False):
        def fn():
            src = x.clone()
            y = src if inplace else torch.full_like(x, float('nan'))
            self.L.check(self.lib.dcf_op_dropout(self.L.ptr(src), self.L.ptr(y), *geom, i64(seed), site, p, self.L.current_stream()), 'dcf_op_dropout')
            return (y,)
        return self._run('dcf_op_dropout', fn)[0]

    def gelu(self, x):
        y = torch.empty_like(x)
        self.L.check(self.lib.dcf_op_gelu(self.L.ptr(x), self.L.ptr(y), x.numel(), self.L.current_stream()), 'dcf_op_gelu')
        return y

    def gelu_bwd(self, x, gy):
        gx = torch.empty_like(x)
        self.L.check(self.lib.dcf_op_gelu_bwd(self.L.ptr(x), self.L.ptr(gy), self.L.ptr(gx), x.numel(), self.L.current_stream()), 'dcf_op_gelu_bwd')
        return gx

    def gelu_dropout(self, x, geom, seed, site, p):
        def fn():
            y = torch.full_like(x, float('nan'))
            self.L.check(self.lib.dcf_op_gelu_dropout(self.L.ptr(x), self.L.ptr(y), *geom, i64(seed), site, p, self.L.current_stream()),
                         'dcf_op_gelu_dropout')
            return (y,)
        return self._run('dcf_op_gelu_dropout', fn)[0]

    def gelu_dropout_bwd(self, x, gy, geom, seed, site, p):
        def fn():
            gx = torch.full_like(x, float('nan'))
            self.L.check(self.lib.dcf_op_gelu_dropout_bwd(self.L.ptr(x), self.L.ptr(gy), self.L.ptr(gx), *geom, i64(seed), site, p,
                                                          self.L.current_stream()), 'dcf_op_gelu_dropout_bwd')
            return (gx,)
        return self._run('dcf_op_gelu_dropout_bwd', fn)[0]

    def residual(self, r, m_r, h, m_h, ls, geom, seed, pd, pp):
        def fn():
            y = torch.full_like(r, float('nan'))
            self.L.check(self.lib.dcf_op_drop_residual(self.L.ptr(r), self.L.ptr(m_r), self.L.ptr(h), self.L.ptr(m_h), self.L.ptr(ls), self.L.ptr(y), *geom,
                                                       i64(seed), SITE_DROP, pd, SITE_PATH, pp, self.L.current_stream()), 'dcf_op_drop_residual')
            return (y,)
        return self._run('dcf_op_drop_residual', fn)[0]

    def residual_bwd(self, gy, h, m_r, m_h, ls, geom, seed, pd, pp, dls0=None):
        def fn():
            dr, dh = torch.full_like(gy, float('nan')), torch.full_like(gy, float('nan'))
            dls = torch.full_like(ls, float('nan')) if dls0 is None else dls0.clone()
            self.L.check(self.lib.dcf_op_drop_residual_bwd(self.L.ptr(gy), self.L.ptr(h), self.L.ptr(m_r), self.L.ptr(m_h), self.L.ptr(ls), self.L.ptr(dr),
                                                           self.L.ptr(dh), self.L.ptr(dls), *geom, i64(seed), SITE_DROP, pd, SITE_PATH, pp,
                                                           int(dls0 is not None), self.L.current_stream()), 'dcf_op_drop_residual_bwd')
            return dr, dh, dls
        return self._run('dcf_op_drop_residual_bwd', fn)

    def ls_residual(self, r, m_r, h, m_h, ls):
        y = torch.empty_like(r)
        self.L.check(self.lib.dcf_op_layerscale_residual(self.L.ptr(r), self.L.ptr(m_r), self.L.ptr(h), self.L.ptr(m_h), self.L.ptr(ls), self.L.ptr(y),
                                                         r.size(0) * r.size(1), r.size(2), self.L.current_stream()), 'dcf_op_layerscale_residual')
        return y

    def ls_residual_bwd(self, gy, h, m_r, m_h, ls):
        dr, dh, dls = torch.empty_like(gy), torch.empty_like(gy), torch.empty_like(ls)
        self.L.check(self.lib.dcf_op_layerscale_residual_bwd(self.L.ptr(gy), self.L.ptr(h), self.L.ptr(m_r), self.L.ptr(m_h), self.L.ptr(ls), self.L.ptr(dr),
                                                             self.L.ptr(dh), self.L.ptr(dls), gy.size(0) * gy.size(1), gy.size(2), 0,
                                                             self.L.current_stream()), 'dcf_op_layerscale_residual_bwd')
        return dr, dh, dls


@pytest.fixture(scope='module')
def ops(pkg):
    return Ops(pkg)


def randn(seed, *shape, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


@pytest.mark.parametrize('p', RATES)
@pytest.mark.parametrize('shape', SHAPES, ids=ids)
def test_dropout_is_the_stated_mask_and_scale(ops, shape, p):
    B, T, C, b0 = shape
    seed = 0xC0FFEE1234567890 + B
    x = randn(1, B, T, C)
    x[x == 0] = 1.0
    keep = R.keep_rows(seed, SITE_DROP, B, T, C, b0, p)
    assert 0 < int(keep.sum()) < keep.numel() or keep.numel() < 16
    want = torch.where(keep, x * torch.tensor(P.scale(p)), torch.zeros(()))             # fp32 product, rounded once; dropped: +0
    for inplace in (False, True):
        y = ops.dropout(x.cuda(), shape, seed, SITE_DROP, p, inplace)
        assert torch.equal((bits(y) != 0).view(B, T, C), keep), 'kept / dropped positions'
        assert same(y, want)
    # its own backward: the same call on dY is dY k, the gradient of sum(dY * drop(x)) with respect to x
    gy = randn(2, B, T, C)
    k = R.factor(keep, p, torch.float64)
    xd = x.double().requires_grad_()
    (R.dropout(xd, k) * gy.double()).sum().backward()
    got = ops.dropout(gy.cuda(), shape, seed, SITE_DROP, p)
    assert torch.equal(got.cpu(), xd.grad.float()), 'not the gradient'                  # as values: autograd's dropped entries are dY * 0 = -0 for dY < 0
    assert same(got, torch.where(keep, gy * torch.tensor(P.scale(p)), torch.zeros(())))
    # p = 0 is the identity
    assert same(ops.dropout(x.cuda(), shape, seed, SITE_DROP, 0.0), x)


@pytest.mark.parametrize('p', RATES)
@pytest.mark.parametrize('shape', GELU_SHAPES, ids=ids)
def test_gelu_dropout_has_the_bits_of_the_two_operator_chains(ops, shape, p):
    B, T, C, b0 = shape
    seed = 0x0123456789ABCDEF
    site = P.site(P.G_STEM, 0, P.FFN_HID)
    x, gy = randn(3, B, T, C, scale=2.0).cuda(), randn(4, B, T, C).cuda()
    y = ops.gelu_dropout(x, shape, seed, site, p)
    assert same(y, ops.dropout(ops.gelu(x), shape, seed, site, p))
    gx = ops.gelu_dropout_bwd(x, gy, shape, seed, site, p)
    assert same(gx, ops.gelu_bwd(x, ops.dropout(gy, shape, seed, site, p)))
    keep = R.keep_rows(seed, site, B, T, C, b0, p)
    assert torch.equal((y.cpu() != 0) | (x.cpu() == 0), keep | (x.cpu() == 0))
    # p = 0: the plain pair
    assert same(ops.gelu_dropout(x, shape, seed, site, 0.0), ops.gelu(x))
    assert same(ops.gelu_dropout_bwd(x, gy, shape, seed, site, 0.0), ops.gelu_bwd(x, gy))


def residual_operands(B, T, C):
    r, h, gy = randn(5, B, T, C), randn(6, B, T, C), randn(7, B, T, C)
    ls = randn(8, C, scale=0.5)
    return r, h, gy, ls, rows_mask(B, T)


@pytest.mark.parametrize('masks', ['mR', 'mH', 'both', 'none'])
@pytest.mark.parametrize('p', RATES)
@pytest.mark.parametrize('shape', SHAPES, ids=ids)
def test_drop_residual_forward_bits_and_backward_rule(ops, shape, p, masks):
    B, T, C, b0 = shape
    p_path = 0.5 if p == 0.1 else 0.3
    seed = pick_seed(B, b0, p_path)
    r, h, gy, ls, m = residual_operands(B, T, C)
    m_r, m_h = (m if masks in ('mR', 'both') else None), (m if masks in ('mH', 'both') else None)
    keep, pk = R.keep_rows(seed, SITE_DROP, B, T, C, b0, p), R.keep_paths(seed, SITE_PATH, B, b0, p_path)
    assert not bool(pk.all()), 'the key was picked to drop a sample'
    md = m.cuda()                                                  # one array: a block has one mask
    dev = lambda t: None if t is None else md
    npy = lambda t: None if t is None else t.numpy()

    y = ops.residual(r.cuda(), dev(m_r), h.cuda(), dev(m_h), ls.cuda(), shape, seed, p, p_path)
    want = R.drop_residual_bits(r.numpy(), npy(m_r), h.numpy(), npy(m_h), ls.numpy(), keep.numpy(), p, pk.numpy(), p_path)
    assert same(y, torch.from_numpy(want)), 'Y differs from the stated fp32 evaluation'

    dr, dh, dls = ops.residual_bwd(gy.cuda(), h.cuda(), dev(m_r), dev(m_h), ls.cuda(), shape, seed, p, p_path)
    ref = {}
    for name, dt in (('64', torch.float64), ('32', torch.float32)):
        cast = lambda t: None if t is None else t.to(dt)
        ref[name] = R.drop_residual_bwd(gy.to(dt), h.to(dt), cast(m_r), cast(m_h), ls.to(dt), R.factor(keep, p, dt), R.factor(pk, p_path, dt))
    assert same(dr, gy if m_r is None else torch.where(m_r[..., None] != 0, gy, torch.zeros(()))), 'dR = dY m_R is exact (a masked row: +0)'
    tag = f'{ids(shape)} p{p} {masks}'
    missed = [R.check('DGERR', f'{tag} dH', dh, ref['64'][1], ref['32'][1]), R.check('DGERR', f'{tag} dls', dls, ref['64'][2], ref['32'][2])]
    assert not [x for x in missed if x], missed
    for b in range(B):
        if not bool(pk[b]):
            assert bool((bits(dh).view(B, T, C)[b] == 0).all()), f'dH of the dropped sample {b} is not +0 everywhere'
    # accumulate: dls is added to what is there, in one rounding
    dls0 = randn(9, C)
    _, _, acc = ops.residual_bwd(gy.cuda(), h.cuda(), dev(m_r), dev(m_h), ls.cuda(), shape, seed, p, p_path, dls0=dls0.cuda())
    assert same(acc, dls0 + dls.cpu())


@pytest.mark.parametrize('masks', ['mR', 'mH', 'both', 'none'])
@pytest.mark.parametrize('shape', SHAPES, ids=ids)
def test_zero_rates_are_the_layerscale_residual(ops, shape, masks):
    B, T, C, b0 = shape
    r, h, gy, ls, m = (t.cuda() for t in residual_operands(B, T, C))
    m_r, m_h = (m if masks in ('mR', 'both') else None), (m if masks in ('mH', 'both') else None)
    assert same(ops.residual(r, m_r, h, m_h, ls, shape, 77, 0.0, 0.0), ops.ls_residual(r, m_r, h, m_h, ls))
    for got, want in zip(ops.residual_bwd(gy, h, m_r, m_h, ls, shape, 77, 0.0, 0.0), ops.ls_residual_bwd(gy, h, m_r, m_h, ls)):
        assert same(got, want)


def test_bad_arguments_are_errors(pkg, ops):
    x = torch.zeros(2, 8, 8, device='cuda')
    L = pkg._lib
    for p in (1.0, -0.1):
        assert ops.lib.dcf_op_dropout(L.ptr(x), L.ptr(x), 2, 8, 8, 0, 1, 0, p, L.current_stream()) != 0
    assert ops.lib.dcf_op_dropout(L.ptr(x), L.ptr(x), 2, 8, 6, 0, 1, 0, 0.5, L.current_stream()) != 0          # C % 4
    assert ops.lib.dcf_op_dropout(L.ptr(x), L.ptr(x), 2, 8, 8, -1, 1, 0, 0.5, L.current_stream()) != 0         # b0 < 0
    assert b'b0' in ops.lib.dcf_last_error()


# ---------------------------------------------------------------------------------------------- whole blocks through autograd
import step_grad_ref as SR  # noqa: E402
from conftest import Golden  # noqa: E402

BLOCK_SITES = {'enc1': (P.G_STEM, 0), 'enc2': (P.G_BRANCH, 1), 'dec': (P.G_FUSION, 1)}


@pytest.mark.parametrize('tag', list(BLOCK_SITES))
def test_block_with_dropout_matches_the_reference_block(pkg, tag):
    """a TransformerEncoder block of stride 1 (enc1, T = 40) and of stride 2 (enc2, T = 40 -> 20) and a TransformerDecoder layer (dec), E = 32,
    three rows, with a DropSpec, against the reference's block inside its step with the stated masks injected (group blk/ of
    tests/golden/step_grad_drop_s1d.npz): output, input gradient and every parameter gradient of the block under the gradient rule.
    The block is used once in that step, so its parameter gradients are the step's."""
    f = SR.Fixture('drop_s1d')
    g = Golden('step_grad_drop_s1d.npz')
    name = f.meta['blocks'][tag]
    rec = lambda k: (g.t(f'blk/{tag}/{k}_32'), g.t(f'blk/{tag}/{k}_32').double() + g.t(f'blk/{tag}/{k}_d').double())
    opt = f.opt(pkg)
    for part in ('vid_net', 'fusion'):
        opt.model[part]['proj_pdrop'], opt.model[part]['path_pdrop'] = f.meta['proj_pdrop'], f.meta['path_pdrop']
    model = pkg.modeling.PtTransformerEarlyFusionIterative(opt, second_fusion=False)
    model.load_state_dict(f.sd)
    block = model.cuda().get_submodule(name)
    A = pkg.autograd
    drop = A.DropSpec(f.meta['seed'], 0, f.meta['proj_pdrop'], f.meta['path_pdrop']).at(*BLOCK_SITES[tag])
    (x32, x64), (y32, y64), (gx32, gx64), (gy32, gy64) = rec('x'), rec('y'), rec('gx'), rec('gy')
    x = SR.tm(x32).cuda().requires_grad_()
    mask = g.t(f'blk/{tag}/mask')[:, 0].cuda()
    if tag == 'dec':
        kv = SR.tm(g.t(f'blk/{tag}/kv_32')).cuda()
        y, mo = A.transformer_decoder(x, mask, kv, g.t(f'blk/{tag}/kv_mask').reshape(kv.size(0), -1).cuda(), block, drop=drop)
    else:
        y, mo = A.transformer_encoder(x, mask, block, drop=drop)
    assert torch.equal(mo.cpu(), g.t(f'blk/{tag}/mask_out')[:, 0])
    y.backward(SR.tm(gy32).cuda())
    missed = [R.check('DGERR', f'{tag} y', y, SR.tm(y64), SR.tm(y32)), R.check('DGERR', f'{tag} dx', x.grad, SR.tm(gx64), SR.tm(gx32))]
    n = 0
    for k, p in block.named_parameters():
        full = f'{name}.{k}'
        assert p.grad is not None, full
        missed.append(R.check('DGERR', f'{tag} {k}', p.grad, f.gp['64'][full], f.gp['32'][full], top=f.top(full)))
        n += 1
    assert n == sum(1 for k in f.gp['64'] if k.startswith(name + '.')) > 10
    assert not [m for m in missed if m], missed
