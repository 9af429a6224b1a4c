"""The operand-range cases of tests/test_gpu_operand_range.py, built once per process on the CPU and shared with
tests/test_operand_range_cpu.py, which checks what each case presupposes (a helper module; users leave the tensors unchanged).

A case carries its fp32 inputs, y64 (fp64 torch), y32 (fp32 torch on the CPU) and `emu`: the same operation with every matrix product
replaced by the plane emulation of tests/f16x3_ref.py (fp64 elsewhere), i.e. the representation error of the operand planes alone.
"""
import contextlib
import functools
import math
import types

import torch
import torch.nn.functional as F

import f16x3_ref as X

A_MAX = 4000.0                        # activations stay inside |a| < 4094
W_MAX = 255.9
A_SCALES = (-8, -4, 0, 6, 9)          # A * 2^s under the rule, both modes
W_SCALES = (-8, 6)                    # W * 2^t (t = 0 is s = 0)
WIDE_SCALES = (-20, 20)               # bf16x6 only: bf16 has fp32's exponent range
FLOOR_SCALES = (-12, -14)             # f16x3 below the envelope: judged against the emulation, not under the rule

# (operator, shape): the smallest shapes at which each kernel takes its tile paths (partial last row tile, K = 1024, channel-major A,
# the three taps of the k3 convolution with a ragged mask)
GEMM_SHAPES = [('linear', (200, 256, 256)), ('linear', (64, 256, 1024)), ('linear_cm', (256, 128, 64)), ('conv3', (2, 300, 64, 64))]


def variants(nterms):
    """the data variants of section (a) for one mode: (kind, exponent)"""
    v = [('a', s) for s in A_SCALES] + [('w', t) for t in W_SCALES] + [('mixed', 0)]
    return v + [('a', s) for s in WIDE_SCALES] if nterms == 6 else v


def gemm_ids():
    return [(op, shape, kind, e) for op, shape in GEMM_SHAPES for kind, e in variants(6)]


def _log_uniform(shape, lo, hi, g):
    """magnitudes log-uniform in [2^lo, 2^hi], random signs"""
    mag = torch.exp2(lo + (hi - lo) * torch.rand(shape, generator=g))
    return mag * torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)


def conv3_rows(x, mask):
    """(B, Cin, T) masked input -> the (B*T, 3*Cin) rows [x[t-1], x[t], x[t+1]] of the k3 convolution as a matrix product"""
    B, C, T = x.shape
    p = F.pad(x * mask, (1, 1))
    return torch.stack([p[:, :, k:k + T] for k in range(3)], 1).permute(0, 3, 1, 2).reshape(B * T, 3 * C)


def conv3_weight(w):
    """(N, Cin, 3) -> (N, 3*Cin) matching conv3_rows"""
    return w.permute(0, 2, 1).reshape(w.size(0), -1)


@functools.lru_cache(maxsize=None)
def gemm_case(op, shape, kind, e):
    """one case of sections (a) / (b).  A (M, K): the logical rows (linear_cm hands the kernel A^T, conv3 hands it x, w, mask); bias is
    scaled with the product so that it never hides the product's error; `emu` / `emu_flush` / `emu6`: f16x3 planes kept / flushed, bf16x6"""
    g = torch.Generator().manual_seed(sum(shape) * 31 + len(op))
    c = types.SimpleNamespace(op=op, shape=shape, kind=kind, e=e, x=None, w3=None, mask=None)
    if op == 'conv3':
        B, T, Cin, N = shape
        base = torch.randn(B, Cin, T, generator=g)
        W = torch.randn(N, Cin, 3, generator=g) / math.sqrt(3 * Cin)
        c.mask = torch.ones(B, 1, T, dtype=torch.bool)
        c.mask[0, :, int(T * 0.9):] = False
        c.mask[-1, :, T - 3:] = False
        c.mask[-1, :, 41] = False
        bias = None
    else:
        M, N, K = shape
        base = torch.randn(M, K, generator=g)
        W = torch.randn(N, K, generator=g) / math.sqrt(K)
        bias = torch.randn(N, generator=g) * 0.5
    if kind == 'mixed':
        base = _log_uniform(base.shape, -12.0, 10.0, g)
    elif kind == 'a':
        base = base * 2.0 ** e
    elif kind == 'w':
        W = W * 2.0 ** e
    if bias is not None and kind != 'mixed':
        bias = bias * 2.0 ** e
    if abs(e) < 20:
        base = base.clamp(-A_MAX, A_MAX)
    if op == 'conv3':
        c.x, c.w3 = base, W
        c.A, c.W = conv3_rows(base, c.mask), conv3_weight(W)
        c.y64 = F.conv1d((base * c.mask).double(), W.double(), padding=1).permute(0, 2, 1).reshape(B * T, N)
        c.y32 = F.conv1d(base * c.mask, W, padding=1).permute(0, 2, 1).reshape(B * T, N)
    else:
        c.A, c.W = base, W
        c.y64 = base.double() @ W.double().t() + bias.double()
        c.y32 = base @ W.t() + bias
    c.bias = bias
    b64 = bias.double() if bias is not None else 0.0
    c.e_ref = X.e_ref(c.y64, c.y32)
    c.emu6 = X.gemm_bf16x6(c.A, c.W) + b64
    if abs(e) < 20:
        c.emu = X.gemm(c.A, c.W) + b64
        c.emu_flush = X.gemm(c.A, c.W, flush=True) + b64
    return c


# ---- (c) chain kernels: restatements with the matrix product as a parameter --------------------------------------------------
CHAIN_SCALES = (-6, 4)


def mm_exact(a, w):
    return a @ w.t()


def mm_emu(a, w):
    """the plane emulation on operands rounded to fp32 (what the kernels hold in registers); operands must be in range"""
    a32, w32 = a.float(), w.float()
    assert float(a32.abs().max()) * X.SA <= X.F16_MAX and float(w32.abs().max()) * X.SW <= X.F16_MAX
    return X.gemm(a32, w32)


def _ln(v, w, b):
    mu = v.mean(1, keepdim=True)
    return (v - mu) / torch.sqrt(((v - mu) ** 2).mean(1, keepdim=True) + 1e-5) * w + b


def _conv_rows(x, w, mm, dil=1):
    """x (B, T, C) rows, w (N, C, 3): the k3 convolution (zero padding, dilation `dil`) through mm -> (B, T, N)"""
    B, T, C = x.shape
    p = F.pad(x, (0, 0, dil, dil))
    a = torch.cat([p[:, k * dil:k * dil + T] for k in range(3)], 2).reshape(B * T, 3 * C)
    return mm(a, w.permute(0, 2, 1).reshape(w.size(0), -1)).view(B, T, -1)


def head_forward(p, dt, mm):
    """ClsHead / RegHead trunk and output convolution (test_gpu_ops.test_head_chain_vs_fp64) -> (B*T, NO)"""
    t = {k: v.to(dt) for k, v in p.items() if k != 'mask'}
    B, T = p['mask'].shape
    mf = p['mask'][:, :, None].to(dt)
    x = t['X'].view(B, T, -1)
    y = torch.relu(_ln(_conv_rows(x * mf, t['W1'], mm).reshape(B * T, -1), t['l1w'], t['l1b'])).view(B, T, -1)
    y = torch.relu(_ln(_conv_rows(y * mf, t['W2'], mm).reshape(B * T, -1), t['l2w'], t['l2b'])).view(B, T, -1)
    return _conv_rows(y * mf, t['Wo'], mm).reshape(B * T, -1) + t['bo']


def ffn_forward(p, dt, mm):
    """x + ls * mask * fc2(gelu(fc1(LayerNorm(x)))) (test_gpu_ops.test_ffn_chain_vs_fp64) -> (M, E)"""
    t = {k: v.to(dt) for k, v in p.items() if k != 'mask'}
    x = t['X']
    h = F.gelu(mm(_ln(x, t['lw'], t['lb']), t['W1']) + t['b1'])
    return x + (mm(h, t['W2']) + t['b2']) * p['mask'][:, None].to(dt) * t['ls']


def tcn_forward(p, dt, mm):
    """oracle.decafnet_ref.tcn_refine on rows: w = the block's parameters, x (B, n_in, T), mask (B, 1, T) -> (B*T, n_out)"""
    w = {k: v.to(dt) for k, v in p['w'].items()}
    B, _, T = p['x'].shape
    mf = p['mask'].permute(0, 2, 1).to(dt)                         # (B, T, 1)
    x = p['x'].to(dt).permute(0, 2, 1)
    out = (mm(x.reshape(B * T, -1), w['conv_1x1.weight'][:, :, 0]) + w['conv_1x1.bias']).view(B, T, -1)
    for i in range(p['n_layers']):
        q = f'layers.{i}.'
        h = torch.relu(_conv_rows(out, w[q + 'conv_dilated.weight'], mm, 2 ** i) + w[q + 'conv_dilated.bias'])
        h = (mm(h.reshape(B * T, -1), w[q + 'conv_1x1.weight'][:, :, 0]) + w[q + 'conv_1x1.bias']).view(B, T, -1)
        out = (out + h) * mf
        out = F.layer_norm(out, (out.size(2),), w[q + 'norm.weight'], w[q + 'norm.bias'], 1e-5)
    out = (mm(out.reshape(B * T, -1), w['conv_out.weight'][:, :, 0]) + w['conv_out.bias']).view(B, T, -1)
    return (out * mf).reshape(B * T, -1)


def _chain_inputs(name, t):
    from conftest import Golden
    s = 2.0 ** t
    g = torch.Generator().manual_seed(500 + len(name))
    if name == 'head':
        B, T, C, NO = 2, 100, 256, 2
        mask = torch.ones(B, T, dtype=torch.bool)
        mask[0, 77:] = False
        mask[1, 17] = False
        return dict(X=torch.randn(B * T, C, generator=g), mask=mask,
                    W1=torch.randn(C, C, 3, generator=g) / math.sqrt(3 * C) * s, W2=torch.randn(C, C, 3, generator=g) / math.sqrt(3 * C) * s,
                    l1w=torch.rand(C, generator=g) + 0.5, l1b=torch.randn(C, generator=g) * 0.3,
                    l2w=torch.rand(C, generator=g) + 0.5, l2b=torch.randn(C, generator=g) * 0.3,
                    Wo=torch.randn(NO, C, 3, generator=g) / math.sqrt(3 * C) * s, bo=torch.randn(NO, generator=g) * s)
    if name == 'ffn':
        M, E = 200, 256
        return dict(X=torch.randn(M, E, generator=g), lw=torch.rand(E, generator=g) + 0.5, lb=torch.randn(E, generator=g) * 0.5,
                    W1=torch.randn(4 * E, E, generator=g) / math.sqrt(E) * s, b1=torch.randn(4 * E, generator=g) * 0.3 * s,
                    W2=torch.randn(E, 4 * E, generator=g) / math.sqrt(4 * E) * s, b2=torch.randn(E, generator=g) * 0.3 * s,
                    ls=torch.randn(E, generator=g), mask=torch.rand(M, generator=g) > 0.2)
    ops = Golden('ops.npz')
    w = {k: (v * s if 'norm' not in k else v) for k, v in ops.sub('tcn/w/').items()}
    return dict(w=w, x=ops.t('tcn/x'), mask=ops.t('mask'), n_layers=4)


CHAIN_FORWARD = dict(head=head_forward, ffn=ffn_forward, tcn=tcn_forward)


def chain_weights(p):
    """the tensors of a chain case that enter weight planes"""
    if 'w' in p:
        return [v for k, v in p['w'].items() if k.endswith('.weight') and 'norm' not in k]
    return [p[k] for k in ('W1', 'W2', 'Wo') if k in p]


@functools.lru_cache(maxsize=None)
def chain_case(name, t):
    p = _chain_inputs(name, t)
    fwd = CHAIN_FORWARD[name]
    with torch.no_grad():
        return types.SimpleNamespace(name=name, t=t, p=p, y64=fwd(p, torch.float64, mm_exact), y32=fwd(p, torch.float32, mm_exact),
                                     emu=fwd(p, torch.float64, mm_emu))


# ---- (f) attention cores ------------------------------------------------------------------------------------------------------
# (kernel, shape): cross attention (B, T, Lk, C, heads), sliding window (B, T, C, heads, window), window 0 = global
ATTN_SHAPES = [('xattn', (1, 70, 17, 128, 4)), ('local', (2, 72, 128, 4, 9)), ('local', (1, 37, 128, 4, 0))]
# q and k by 8: the softmax saturates (the max subtraction); by 2^-6: near-uniform; v by 2^8 and 2^-8
ATTN_VARIANTS = [('qk', 3), ('qk', -6), ('v', 8), ('v', -8)]


def attn_forward(q, k, v, kvmask, heads, window, dt, planes, vs_fixed=None):
    """MaskedMHA's core (blocks.py:339-393) on token-major (B, T, C) / (B, Lk, C): d^-1/4 on q and k, masked softmax over the keys
    (window > 0: |i - j| <= window // 2), context.  planes = True (window 0): csrc/attn.hip k_xattn_mfma -- both products on two fp16
    planes per operand for the keys of whole 16-key tiles, q, k and the probabilities unscaled, v under the kernel's plane scale: 1
    where max |v| over those keys of a (batch, head), masked ones included, is at least 2^-2, else the power of two that lifts that
    maximum into [8, 16); vs_fixed: that scale instead (1.0: unscaled planes whatever v is, which at v * 2^-8 breaks the rule 3.2x
    by representation alone).  fp64 elsewhere."""
    B, T, C = q.shape
    Lk, d = k.size(1), C // heads
    s = 1.0 / math.sqrt(math.sqrt(d))

    def sp(z):
        return z.to(dt).view(B, -1, heads, d).transpose(1, 2)

    qh, kh, vh = sp(q) * s, sp(k) * s, sp(v)
    allow = kvmask[:, None, None, :].expand(B, 1, T, Lk)
    if window > 0:
        i = torch.arange(T)
        allow = allow & ((i[:, None] - i[None, :]).abs() <= window // 2)[None, None]

    def prod(a, b, sb=1.0):                  # a (.., m, k) x b (.., n, k)^T, the planes of b under the scale sb
        if not planes:
            return a @ b.transpose(-1, -2)
        ah, am = X.split(a.float(), 1.0)
        bh, bm = X.split(b.float(), sb)
        return (ah @ bh.transpose(-1, -2) + ah @ bm.transpose(-1, -2) + am @ bh.transpose(-1, -2)) / sb

    if not planes:
        att = prod(qh, kh).masked_fill(~allow, float('-inf'))
        return prod(F.softmax(att, -1), vh.transpose(-1, -2)).transpose(1, 2).reshape(B, T, C)
    # the kernel's split of the keys (launch_xattn_mfma): whole 16-key tiles on planes, up to two trailing keys in fp32 (exact here)
    nk = Lk - Lk % 16 if Lk % 16 <= 2 else Lk
    att = torch.cat([prod(qh, kh[..., :nk, :]), qh @ kh[..., nk:, :].transpose(-1, -2)], -1).masked_fill(~allow, float('-inf'))
    p = F.softmax(att, -1)
    vmax = vh[..., :nk, :].abs().amax((-1, -2), keepdim=True).double() if nk else torch.ones(B, heads, 1, 1, dtype=torch.float64)
    vs = vs_fixed if vs_fixed is not None else torch.where(vmax < 0.25, 2.0 ** (3 - torch.floor(torch.log2(vmax))), torch.ones_like(vmax))
    out = prod(p[..., :nk], vh[..., :nk, :].transpose(-1, -2), vs) + p[..., nk:] @ vh[..., nk:, :]
    return out.transpose(1, 2).reshape(B, T, C)


@functools.lru_cache(maxsize=None)
def attn_case(kind, shape, what, e):
    if kind == 'xattn':
        B, T, Lk, C, heads = shape
        window = 0
    else:
        B, T, C, heads, window = shape
        Lk = T
    g = torch.Generator().manual_seed(T * 7 + C + Lk)
    q, k, v = torch.randn(B, T, C, generator=g), torch.randn(B, Lk, C, generator=g), torch.randn(B, Lk, C, generator=g)
    m = torch.ones(B, Lk, dtype=torch.bool)
    m[-1, int(Lk * 0.7):] = False
    if what == 'qk':
        q, k = q * 2.0 ** e, k * 2.0 ** e
    else:
        v = v * 2.0 ** e
    c = types.SimpleNamespace(kind=kind, shape=shape, q=q, k=k, v=v, mask=m, heads=heads, window=window)
    # rows whose own key is masked are undefined in the sliding-window reference (they attend to nothing they own): valid rows only
    c.rows = m.reshape(-1) if kind == 'local' else torch.ones(B * T, dtype=torch.bool)
    c.y64 = attn_forward(q, k, v, m, heads, window, torch.float64, False).reshape(B * T, C)
    c.y32 = attn_forward(q, k, v, m, heads, window, torch.float32, False).reshape(B * T, C)
    # the cross-attention core runs on fp16 planes; the sliding-window and the global core are fp32 FMA chains: nothing to emulate
    c.emu = attn_forward(q, k, v, m, heads, window, torch.float64, kind == 'xattn').reshape(B * T, C)
    return c


@functools.lru_cache(maxsize=None)
def attn_unscaled_case():
    """the `xattn v 2^-8` case with one element of 1.0 per head in a MASKED key of the MFMA tile: max |v| >= 2^-2, so the kernel must
    keep v on unscaled planes although every key that counts is small (the masked key's probability is exactly 0: y64 and y32 are the
    base case's).  emu_unscaled: what unscaled planes give; the base case's emu: what scaled planes would."""
    kind, shape = ATTN_SHAPES[0]
    base = attn_case(kind, shape, 'v', -8)
    key = 12
    assert not bool(base.mask[0, key]) and key < 16
    v = base.v.clone()
    v[0, key, ::v.size(-1) // base.heads] = 1.0
    c = types.SimpleNamespace(**vars(base))
    c.v = v
    c.emu_unscaled = attn_forward(c.q, c.k, v, c.mask, c.heads, 0, torch.float64, True).reshape(base.y64.shape)
    c.emu_scaled = base.emu
    c.e_ref = X.e_ref(c.y64, c.y32)
    return c


# ---- the oracle with its dense convolutions on planes ----------------------------------------------------------------------------
class _PlaneF:
    """torch.nn.functional with conv1d on emulated planes: every dense convolution (groups == 1: the 1x1 projections, embd_fc, vid_map,
    the k3 convolutions of the heads, the TCN) is hi*hi + hi*mid + mid*hi of the fp16 planes of its operands rounded to fp32, summed
    in fp64 and un-scaled; activations under 2^4, weights under 2^8, a convolution of `unit_cin` input channels (vid_map) under an
    activation scale of 1 as its launches have.  Depthwise convolutions and everything else are torch's."""

    def __init__(self, unit_cin):
        self.unit_cin = unit_cin

    def __getattr__(self, name):
        return getattr(F, name)

    def conv1d(self, x, w, bias=None, stride=1, padding=0, dilation=1, groups=1):
        if groups != 1:
            return F.conv1d(x, w, bias, stride, padding, dilation, groups)
        sa = 1.0 if w.size(1) == self.unit_cin else X.SA
        assert float(x.abs().max()) * sa <= X.F16_MAX and float(w.abs().max()) * X.SW <= X.F16_MAX
        (xh, xm), (wh, wm) = X.split(x.float(), sa), X.split(w.float(), X.SW)
        y = sum(F.conv1d(a, b, None, stride, padding, dilation) for a, b in ((xh, wh), (xh, wm), (xm, wh))) / (sa * X.SW)
        return y if bias is None else y + bias.double()[:, None]


@contextlib.contextmanager
def oracle_on_planes(unit_cin=None):
    """inside, oracle.decafnet_ref computes its dense convolutions as _PlaneF does (call it through forward_parity.oracle64: fp64
    elsewhere).  The attention products stay exact: section (f) has their cases."""
    from oracle import decafnet_ref as R
    keep, R.F = R.F, _PlaneF(unit_cin)
    try:
        yield
    finally:
        R.F = keep


# ---- (d) front end on reference-shaped features, (e) text path ------------------------------------------------------------------
# the small model of test_gpu_e2e.test_f16x3_range_guards, but E = 128: the vid_map product of a narrower model does not run on
# fp16 planes at all (channel-major A on the split path needs N % 128 == 0; E = 64 takes the fp32 GEMM)
FRONT_KW = dict(E=128, TE=32, text_in=32, n_levels=3, win=5, n_heads=2, sn=8, sratio=0.4, msf=True, norm=True, max_seq_len=128,
                text_layers=1, text_max_len=24)
FRONT_T, FRONT_LEN = 128, 120
FRONT_DIMS = (1024, 4096)
# unit-length clips (the reference's normalize_vid, libs/data/dataset.py:401-403), the same from non-negative heavy-tailed features,
# features stored at 2^-10 and at 2^10
FRONT_KINDS = ('unit', 'unit_relu', 'small', 'large')

def _features(kind, D, T, g):
    if kind == 'unit':
        return F.normalize(torch.randn(1, D, T, generator=g), dim=1)
    if kind == 'unit_relu':
        return F.normalize(torch.relu(torch.randn(1, D, T, generator=g)) * torch.rand(1, D, T, generator=g) ** 4, dim=1)
    return torch.randn(1, D, T, generator=g) * 2.0 ** (-10 if kind == 'small' else 10)


@functools.lru_cache(maxsize=None)
def front_case(D, kind):
    """the model, its inputs and the CPU side of the front end: scores, gate and vid_map of query 0 in fp64 / fp32 / on planes"""
    from conftest import load_pkg
    from oracle import decafnet_ref as R
    pkg = load_pkg()
    kw = dict(FRONT_KW, D=D)
    opt = pkg.config.make_opt(**kw)
    shapes = {k: list(v.shape) for k, v in pkg.modeling.create_model(opt).state_dict().items()}
    sd = pkg.synth.make_state_dict(shapes, 77)
    inp = pkg.synth.make_inputs(D, FRONT_T, FRONT_LEN, 1, kw['text_in'], 6, 7)
    g = torch.Generator().manual_seed(D + len(kind))
    inp['vid'], inp['shallow_vid'] = _features(kind, D, FRONT_T, g), _features(kind, D, FRONT_T, g)
    cfg = opt.model
    c = types.SimpleNamespace(D=D, kind=kind, kw=kw, opt=opt, sd=sd, inp=inp)
    vid, sh, vm, tc = inp['vid'], inp['shallow_vid'], inp['vid_masks'], inp['text_cls']
    c.correl64 = R.sidekick_scores(sh.double(), tc.double(), cfg['norm'])
    c.correl32 = R.sidekick_scores(sh, tc, cfg['norm'])
    n = int(vm.sum())
    c.pooled64 = F.avg_pool1d(c.correl64[0][None, None, :n], cfg['sn'], cfg['sn'], ceil_mode=True)[0, 0]
    c.pooled32 = F.avg_pool1d(c.correl32[0][None, None, :n], cfg['sn'], cfg['sn'], ceil_mode=True)[0, 0]
    c.gate64 = torch.zeros(FRONT_T)
    c.gate64[:n] = R.topk_block_gate(c.correl64[0], n, cfg['sn'], cfg['sratio']).float()
    W = sd['vid_map.conv.weight'][:, :, 0]
    a1, a2 = (vid[0] * c.gate64).t().contiguous(), sh[0].t().contiguous()            # (T, D) rows of the two halves of vid_map
    w1, w2, b = W[:, :D], W[:, D:], sd['vid_map.conv.bias']
    valid = vm[0]
    c.vidmap64 = (a1.double() @ w1.double().t() + a2.double() @ w2.double().t() + b.double())[valid]
    c.vidmap32 = (torch.cat([a1, a2], 1) @ W.t() + b)[valid]

    c.vidmap_emu = (X.gemm(a1, w1, 1.0) + X.gemm(a2, w2, 1.0) + b.double())[valid]       # the vid_map launches: a_scale = 1
    return c


@functools.lru_cache(maxsize=None)
def front_forward_case(D, kind):
    """the whole forward of front_case(D, kind) on the CPU, query 0, on the fp32 oracle's text encoding (the GPU test hands all three
    sides the GPU's encoding instead: the same tokens): `fused` over valid clips and the logits pooled over the levels, each as
    (emu, y64, y32) with emu = the fp64 oracle inside oracle_on_planes"""
    import forward_parity as P
    from oracle import decafnet_ref as R
    c = front_case(D, kind)
    inp, cfg = c.inp, c.opt.model
    tok = inp['tokens'][0][None]
    with torch.no_grad():
        text, tmask = R.encode_text(c.sd, cfg, tok, torch.ones(1, 1, tok.size(-1), dtype=torch.bool))
        args = (inp['vid'], inp['shallow_vid'], inp['vid_masks'], [text], inp['text_cls'], [tmask])
        y32 = R.forward_eval(c.sd, cfg, *args, return_intermediates=True)
    y64 = P.oracle64.forward_eval(c.sd, cfg, *args, return_intermediates=True)
    with oracle_on_planes(unit_cin=2 * D):
        emu = P.oracle64.forward_eval(c.sd, cfg, *args, return_intermediates=True)
    valid = inp['vid_masks'][0]
    out = types.SimpleNamespace()
    out.fused = tuple(y[3]['per_query'][0]['fused'][0][:, valid] for y in (emu, y64, y32))
    out.logits = tuple(P.pool(y[0]) for y in (emu, y64, y32))
    return out


TEXT_KINDS = ('unit', 'small', 'large')       # unit-length tokens (the reference's normalize_text), tokens * 2^-8, tokens * 2^8


@functools.lru_cache(maxsize=None)
def text_case(kind, lq=11):
    """tokens (1, text_in, lq) for the text encoder of front_case's model, y64 / y32 from the oracle, emu: the fp64 oracle with
    embd_fc and every projection of the encoder on planes (oracle_on_planes)"""
    import forward_parity as P
    from oracle import decafnet_ref as R
    c0 = front_case(FRONT_DIMS[0], 'unit')
    g = torch.Generator().manual_seed(900 + len(kind))
    tok = torch.randn(1, FRONT_KW['text_in'], lq, generator=g)
    tok = F.normalize(tok, dim=1) if kind == 'unit' else tok * 2.0 ** (-8 if kind == 'small' else 8)
    mask = torch.ones(1, 1, lq, dtype=torch.bool)
    mask[..., lq - 2:] = False
    y64, m64 = P.oracle64.encode_text(c0.sd, c0.opt.model, tok, mask)
    with torch.no_grad():
        y32, m32 = R.encode_text(c0.sd, c0.opt.model, tok, mask)
    assert torch.equal(m64, m32)
    with oracle_on_planes():
        emu, _ = P.oracle64.encode_text(c0.sd, c0.opt.model, tok, mask)
    return types.SimpleNamespace(kind=kind, tok=tok, mask=mask, y64=y64, y32=y32, emu=emu, out_mask=m64, model=c0)
