"""GPU checks of global self-attention (mha_win_size = 0) composed: autograd.masked_mha and autograd.transformer_encoder (stride 1 / 2)
with window_size = 0 against the reference's own `backward()` (tests/golden/global_attn_grad.npz), the stride-0 blocks of the text
encoder beyond 64 positions, and the whole training step of case g1 (tests/golden/step_grad_global*.npz) up to TrainStep.step.

The yardstick is the project's gradient rule, unchanged, per tensor: e_gpu <= max(4 e_ref, 2^-21 max |g_64|), with g_64 the reference's
fp64 run and e_ref the error of its fp32 run.  For key.bias / k_norm.bias, zero in exact arithmetic, max |g_64| is that of the same
layer's weight.  Every check prints a `GAERR` line (`SGERR` for the step, as tests/test_gpu_step_grad.py does); the figures are in
profiles/global_attn_grad.md."""
import pytest
import torch

from conftest import Golden, load_pkg
import global_attn_grad_ref as R
import global_step_fixture as G
import step_grad_ref as S
from test_gpu_step_grad import check as step_check
from test_gpu_train_step import batch_of

pytestmark = pytest.mark.gpu
ZERO = ('key.bias', 'k_norm.bias')


@pytest.fixture(scope='module')
def pkg():
    return load_pkg()


def rule(tag, got, g64, e_ref, top, missed):
    got, g64 = got.detach().cpu().double(), g64.double()
    assert got.shape == g64.shape and bool(torch.isfinite(got).all()), (tag, got.shape, g64.shape)
    e_gpu = float((got - g64).abs().max())
    bound = max(4 * e_ref, R.FLOOR * top)
    ok = e_gpu <= bound
    print(f'GAERR {tag}: max|g64| {top:.3e} e_ref {e_ref:.3e} e_gpu {e_gpu:.3e} bound {bound:.3e} ratio {e_gpu / bound:.3f}{"" if ok else "  MISSED"}')
    if not ok:
        missed.append((tag, e_gpu, bound))


def pair_rule(tag, got, g32, g64, missed, top=None):
    rule(tag, got, g64, float((g32.double() - g64).abs().max()), float(g64.abs().max()) if top is None else top, missed)


# ---------------------------------------------------------------------------------------------- MaskedMHA, window_size = 0
@pytest.mark.parametrize('name', [s[0] for s in R.SHAPES if s[7]])
def test_masked_mha_matches_the_reference_backward(pkg, name):
    """the gradient of every recorded parameter (all eight at below_tile; the biases at the larger shapes, where key.bias, zero in exact
    arithmetic, has no recorded weight gradient to take its scale from and is left to below_tile) and, at below_tile, of the input"""
    f = R.OpFixture(name)
    mha = pkg.modeling.MaskedMHA(f.C, n_heads=f.heads, window_size=0)
    mha.load_state_dict(f.sd)
    mha = mha.cuda()
    x = f.x.cuda().requires_grad_(True)
    y = pkg.autograd.masked_mha(x, x, x, f.mask.cuda(), mha)
    (y * f.up.cuda()).sum().backward()
    missed = []
    if 'gx' in f.g64:
        rule(f'mha {name} dx', f.at_rows(x.grad), f.g64['gx'], f.e_ref['gx'], f.top['gx'], missed)
    seen = 0
    for k, p in mha.named_parameters():
        if k not in f.gp64 or (k.endswith(ZERO) and 'key.weight' not in f.gp64):
            continue
        top = float(f.gp64['key.weight'].abs().max()) if k.endswith(ZERO) else None
        pair_rule(f'mha {name} {k}', p.grad, f.gp32[k], f.gp64[k], missed, top)
        seen += 1
    assert seen == (8 if name == 'below_tile' else 3)
    assert not missed, missed


# ---------------------------------------------------------------------------------------------- TransformerEncoder, window_size = 0
def enc_block(pkg, g, stride, enc):
    blk = pkg.modeling.TransformerEncoder(enc['E'], stride, enc['heads'], 0)
    blk.load_state_dict(g.sub('enc/param/'))
    return blk.cuda()


@pytest.mark.parametrize('name', ['s1', 's2'])
def test_transformer_encoder_matches_the_reference_backward(pkg, name):
    g = Golden('global_attn_grad.npz')
    meta = g.js('meta')
    enc, stride = meta['enc'], meta['enc_cases'][name]
    pre = f'enc/{name}/'
    blk = enc_block(pkg, g, stride, enc)
    x = S.tm(g.t(pre + 'x')).cuda().requires_grad_(True)
    mask = g.t(pre + 'mask').cuda()
    y, mo = pkg.autograd.transformer_encoder(x, mask, blk)
    assert torch.equal(mo.cpu(), g.t(pre + 'mask_out'))
    (y * S.tm(g.t(pre + 'up')).cuda()).sum().backward()
    two = lambda key: (g.t(f'{pre}{key}/32'), g.t(f'{pre}{key}/32').double() + g.t(f'{pre}{key}/d').double())
    missed = []
    o32, o64 = two('out')
    pair_rule(f'enc {name} out', y, S.tm(o32), S.tm(o64), missed)
    x32, x64 = two('gx')
    pair_rule(f'enc {name} dx', x.grad, S.tm(x32), S.tm(x64), missed)
    seen = 0
    for k, p in blk.named_parameters():
        g32, g64 = two(f'gp/{k}')
        top = float(two(f'gp/{k[:-len("bias")]}weight')[1].abs().max()) if k.endswith(ZERO) else None
        pair_rule(f'enc {name} {k}', p.grad, g32, g64, missed, top)
        seen += 1
    assert seen == 27
    assert not missed, missed


def test_transformer_encoder_with_dropout_repeats_its_bits(pkg):
    A = pkg.autograd
    g = Golden('global_attn_grad.npz')
    meta = g.js('meta')
    runs = []
    for _ in range(2):
        blk = enc_block(pkg, g, 2, meta['enc'])
        x = S.tm(g.t('enc/s2/x')).cuda().requires_grad_(True)
        drop = A.DropSpec(0x1234567890abcdef, 0, 0.2, 0.1, A.DROP_G_BRANCH, 1)
        y, _ = A.transformer_encoder(x, g.t('enc/s2/mask').cuda(), blk, drop=drop)
        (y * S.tm(g.t('enc/s2/up')).cuda()).sum().backward()
        runs.append([y.detach(), x.grad] + [p.grad for p in blk.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    blk = enc_block(pkg, g, 2, meta['enc'])
    plain, _ = A.transformer_encoder(S.tm(g.t('enc/s2/x')).cuda(), g.t('enc/s2/mask').cuda(), blk)
    assert not torch.equal(plain, runs[0][0]), 'the dropout dropped nothing'


# ---------------------------------------------------------------------------------------------- the stride-0 blocks of the text encoder
def text_block(pkg, C, heads, seed):
    import enc_grad_ref
    blk = pkg.modeling.TransformerEncoder(C, 0, heads, 0)
    enc_grad_ref.set_block_parameters(blk, torch.Generator().manual_seed(seed))
    return blk


def test_stride_0_block_beyond_64_positions(pkg):
    """T = 70 tokens on 2 heads of 32 channels: xattn_mha's self-attention takes global_attention.  The whole block -- output, input
    gradient and the gradient of each of its 18 parameters -- against the oracle's transformer_encoder differentiated in fp64, with
    e_ref from the same in fp32 on the CPU, and the attention core inside it against global_attn_grad_ref on the block's own q, k, v
    and upstream gradient.  Other head dimensions beyond 64 positions keep cross_attention's message."""
    import enc_grad_ref as E
    A = pkg.autograd
    B, T, C, heads = 2, 70, 64, 2
    gen = torch.Generator().manual_seed(70)
    blk = text_block(pkg, C, heads, 71)
    x0, up = torch.randn(B, T, C, generator=gen), torch.randn(B, T, C, generator=gen)
    mask = torch.arange(T)[None, :] < torch.tensor([70, 41])[:, None]
    ref = {}
    for dt in (torch.float64, torch.float32):
        sd = {k: v.detach().to(dt).clone().requires_grad_(True) for k, v in blk.state_dict().items()}
        xr = x0.to(dt).clone().requires_grad_(True)
        yr, _ = E.oracle_encoder(sd, xr, mask, 0, heads, 0)
        (yr * up.to(dt)).sum().backward()
        ref[dt] = (yr.detach(), xr.grad, {k: v.grad for k, v in sd.items()})
    blk = blk.cuda()
    x = x0.cuda().requires_grad_(True)
    tap = {}
    inner = A.global_attention

    def spy(q, k, v, m, h):
        for z in (q, k, v):
            z.retain_grad()
        o = inner(q, k, v, m, h)
        o.retain_grad()
        tap.update(q=q, k=k, v=v, o=o, h=h)
        return o

    A.global_attention = spy
    try:
        y, _ = A.transformer_encoder(x, mask.cuda(), blk, narrow_heads=True)
    finally:
        A.global_attention = inner
    assert tap and tap['h'] == heads, 'the block did not take global_attention'
    (y * up.cuda()).sum().backward()
    (y64, x64, p64), (y32, x32, p32) = ref[torch.float64], ref[torch.float32]
    missed = []
    pair_rule('text block T70 out', y, y32, y64, missed)
    pair_rule('text block T70 dx', x.grad, x32, x64, missed)
    seen = 0
    for k, p in blk.named_parameters():
        top = float(p64[k[:-len('bias')] + 'weight'].abs().max()) if k.endswith(ZERO) else None
        pair_rule(f'text block T70 {k}', p.grad, p32[k], p64[k], missed, top)
        seen += 1
    assert seen == 18 and not missed, missed
    q, k, v, do = [tap[n].detach().cpu() for n in ('q', 'k', 'v')] + [tap['o'].grad.cpu()]
    g64, g32 = R.reference_pair(q, k, v, mask, do, heads)
    for n, a, b, c in zip(('dQ', 'dK', 'dV'), (tap['q'].grad, tap['k'].grad, tap['v'].grad), g64, g32):
        R.rule(f'text block T70 core {n}', a, b, c)
    with pytest.raises(ValueError, match='cross_attention: Lk = 70'):             # other head dimensions keep today's message
        A.transformer_encoder(torch.zeros(1, 70, 32).cuda(), None, text_block(pkg, 32, 2, 3).cuda(), narrow_heads=True)


def test_stride_0_block_of_25_positions_keeps_its_path(pkg):
    """at most 64 positions: xattn_mha runs cross_attention as before -- the bits of an explicit call"""
    A = pkg.autograd
    B, T, C, heads = 2, 25, 64, 2
    gen = torch.Generator().manual_seed(25)
    blk = text_block(pkg, C, heads, 26).cuda()
    mha = blk.attn.attn
    x = torch.randn(B, T, C, generator=gen).cuda()
    mask = (torch.arange(T)[None, :] < torch.tensor([25, 14])[:, None]).cuda()
    up = torch.randn(B, T, C, generator=gen).cuda()

    def explicit(z):
        q = A.masked_conv1d(z, None, mha.query.weight, mha.query.bias)
        k = A.masked_conv1d(z, None, mha.key.weight, mha.key.bias)
        v = A.masked_conv1d(z, None, mha.value.weight, mha.value.bias)
        return A.masked_conv1d(A.cross_attention(q, k, v, mask, heads), None, mha.proj.weight, mha.proj.bias)

    outs = []
    for fn in (lambda z: A.xattn_mha(z, z, mask, mha), explicit):
        for p in mha.parameters():
            p.grad = None
        z = x.clone().requires_grad_(True)
        y = fn(z)
        (y * up).sum().backward()
        outs.append([y.detach(), z.grad] + [p.grad.clone() for p in mha.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*outs))


# ---------------------------------------------------------------------------------------------- the whole step, case g1
def test_whole_step_g1_matches_the_reference_step(pkg):
    """tests/test_gpu_step_grad.py's check of s1 / s2 on case g1: taps, outputs, the total, the gradients at the text-encoder and at the
    first-fusion output and the gradient of EVERY parameter; video_transformer, fuse_and_predict and run_step are called as they are"""
    f = G.fixture()
    model = f.model(pkg).cuda()
    s = S.run_step(pkg, model, f)
    s.total.backward()
    l1, l2, off, masks = s.outputs
    missed = []
    for l in range(f.L):
        assert torch.equal(masks[l].cpu(), f.masks[l]), f'mask of level {l}'
    for k in S.TAPS + tuple(f'fpn{l}' for l in range(f.L)):
        missed.append(step_check(f'g1 tap/{k}', s.taps[k], f.taps['64'][k], f.taps['32'][k]))
    for key, outs in (('logits1', l1), ('logits2', l2), ('offsets', off)):
        for l in range(f.L):
            missed.append(step_check(f'g1 {key}/l{l}', outs[l], f.out['64'][key][l], f.out['32'][key][l]))
    missed.append(step_check('g1 total', s.total, f.total['64'], f.total['32']))
    for k in S.GTAPS:
        missed.append(step_check(f'g1 d tap/{k}', s.taps[k].grad, f.gtaps['64'][k], f.gtaps['32'][k]))
    seen = 0
    for k, p in model.named_parameters():
        assert p.grad is not None, k
        missed.append(step_check(f'g1 {k}', p.grad, f.gp['64'][k], f.gp['32'][k], top=f.top(k)))
        seen += 1
    assert seen == f.meta['n_params'] == len(f.gp['64'])
    missed = [m for m in missed if m is not None]
    assert not missed, missed


def test_train_step_on_g1_moves_every_parameter(pkg):
    f = G.fixture()
    model = f.model(pkg).cuda()
    opt = f.opt(pkg)
    opt.train.warmup_epochs = 0
    ts = pkg.train.TrainStep(model, opt, itrs_per_epoch=1)
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    batch, targets = batch_of(f)
    for _ in range(2):                                     # (a schedule that starts from lr = 0 moves nothing in its first step)
        lr = ts.optimizer.param_groups[0]['lr']
        out = ts.step(batch, targets)
        assert set(out) >= {'cls', 'reg', 'total', 'grad_norm'} and all(bool(torch.isfinite(out[k]).all()) for k in ('cls', 'reg', 'total', 'grad_norm'))
        if lr > 0:
            break
    assert lr > 0
    still = [k for k, p in model.named_parameters() if torch.equal(p.detach(), before[k])]
    assert not still, f'parameters the step did not move: {still}'
