"""The global self-attention core of MaskedMHA (blocks.py:374-389 with q, k and v of one sequence) and its gradient, restated in torch
in the dtype of its operands -- fp64 for the yardstick, fp32 on the CPU for e_ref -- with the conventions of
include/decafnet_hip_attn.h: the mask masks keys only, a padded key takes exactly 0, a sequence without a valid key gives zeros.
The backward is written out (dP, delta, dS), not taken from autograd, so that it can be checked against finite differences and
against the reference's own `backward()` (tests/golden/global_attn_grad.npz).  A helper module of tests/test_global_attn_grad_cpu.py
and tests/test_gpu_global_attn_grad.py.

Tensors are token-major (B, T, C), heads concatenated along C; mask (B, T) bool or None."""
import torch

FLOOR = 2.0 ** -21

# (name, B, T, C, heads, lengths or None, holes of the second sequence inside its valid part, F = in the reference fixture)
SHAPES = [
    ('one_row', 1, 1, 64, 2, None, (), False),
    ('below_tile', 2, 37, 64, 2, (37, 20), (), True),
    ('tile', 1, 64, 64, 1, None, (), False),
    ('past_tile', 2, 65, 128, 2, (65, 64), (), True),
    ('two_tiles_tail', 2, 130, 256, 4, (130, 71), (3, 17, 18, 40, 63, 64, 70), True),
    ('last_tile_padded', 1, 130, 64, 2, (60,), (), False),
    ('no_valid_key', 2, 40, 64, 2, (40, 0), (), False),
]


def shape_mask(B, T, lens, holes):
    """None for an unmasked shape, else (B, T) bool: lengths, and `holes` cleared in the last sequence"""
    if lens is None:
        return None
    mask = torch.arange(T)[None, :] < torch.tensor(lens)[:, None]
    for h in holes:
        mask[-1, h] = False
    return mask


def shape_case(name, dtype=torch.float32):
    """(q, k, v, do, mask, heads) of a row of SHAPES: q, k, v ~ N(0, 1), dO ~ N(0, 1) on EVERY row, padded ones included"""
    i = [s[0] for s in SHAPES].index(name)
    _, B, T, C, heads, lens, holes, _ = SHAPES[i]
    gen = torch.Generator().manual_seed(4100 + i)
    q, k, v, do = (torch.randn(B, T, C, generator=gen).to(dtype) for _ in range(4))
    return q, k, v, do, shape_mask(B, T, lens, holes), heads


def _split(x, heads):
    B, T, C = x.shape
    return x.reshape(B, T, heads, C // heads).transpose(1, 2)            # (B, h, T, d)


def _join(x):
    B, h, T, d = x.shape
    return x.transpose(1, 2).reshape(B, T, h * d)


def probabilities(q, k, mask, heads):
    """p (B, h, T, T): softmax over the valid keys; rows of a sequence without a valid key are 0"""
    d = q.size(2) // heads
    scale = d ** -0.25
    s = (_split(q, heads) * scale) @ (_split(k, heads) * scale).transpose(-1, -2)
    if mask is None:
        return torch.softmax(s, dim=-1)
    key = mask[:, None, None, :]
    s = s.masked_fill(~key, float('-inf'))
    m = s.max(dim=-1, keepdim=True).values
    e = torch.where(key, torch.exp(s - torch.where(torch.isfinite(m), m, torch.zeros_like(m))), torch.zeros_like(s))
    l = e.sum(dim=-1, keepdim=True)
    return torch.where(l > 0, e / torch.where(l > 0, l, torch.ones_like(l)), torch.zeros_like(e))


def forward(q, k, v, mask, heads):
    return _join(probabilities(q, k, mask, heads) @ _split(v, heads))


def grads(q, k, v, mask, do, heads):
    """(dQ, dK, dV) by the formulas of the header, in the operands' dtype"""
    d = q.size(2) // heads
    s2 = d ** -0.5
    p = probabilities(q, k, mask, heads)
    g = _split(do, heads)
    dp = g @ _split(v, heads).transpose(-1, -2)
    delta = (p * dp).sum(dim=-1, keepdim=True)
    ds = p * (dp - delta)
    dv = p.transpose(-1, -2) @ g
    dq = s2 * (ds @ _split(k, heads))
    dk = s2 * (ds.transpose(-1, -2) @ _split(q, heads))
    return _join(dq), _join(dk), _join(dv)


def reference_pair(q, k, v, mask, do, heads):
    """((dQ, dK, dV) in fp64, the same in fp32 on the CPU): the yardstick and the e_ref of the gradient rule"""
    g64 = grads(q.double(), k.double(), v.double(), mask, do.double(), heads)
    g32 = grads(q.float(), k.float(), v.float(), mask, do.float(), heads)
    return g64, g32


def rule(tag, got, g64, g32, label='GAERR'):
    """the project's gradient rule on one tensor: e_gpu <= max(4 e_ref, 2^-21 max|g64|); prints one line, returns (e_gpu, bound)"""
    got, g64, g32 = got.detach().cpu().double(), g64.detach().double(), g32.detach().double()
    assert got.shape == g64.shape == g32.shape, (tag, got.shape, g64.shape, g32.shape)
    assert bool(torch.isfinite(got).all()), tag
    e_ref, e_gpu, top = float((g32 - g64).abs().max()), float((got - g64).abs().max()), float(g64.abs().max())
    bound = max(4 * e_ref, FLOOR * top)
    print(f'{label} {tag}: max|g64| {top:.3e} e_ref {e_ref:.3e} e_gpu {e_gpu:.3e} bound {bound:.3e} ratio {e_gpu / bound if bound else 0.0:.3f}')
    assert e_gpu <= bound, (tag, e_gpu, bound)
    return e_gpu, bound


# ---------------------------------------------------------------------------------------------- the reference fixture
class OpFixture:
    """case op/<name> of tests/golden/global_attn_grad.npz (make_golden_global_attn_grad.py): the reference's MaskedMHA(window_size=0)
    at a shape marked F.  x, up (B, T, C) token-major, mask (B, T), sd (the state dict), heads; q, k, v and do, the operands of the
    attention core, recomputed here -- inputs and parameters lie on a grid that makes the projections exact in fp32, in any summation
    order (the generator asserts that the reference's fp32 and fp64 runs hold the same numbers); rows, and by tensor name g32[name] /
    g64[name] at those rows of the flattened (B * T, C) tensor ('dq', 'dk', 'dv', for below_tile 'gx' too), gp32 / gp64 by parameter,
    e_ref[name] = max |g32 - g64| and top[name] = max |g64| over ALL rows."""

    def __init__(self, name):
        from conftest import Golden
        g = Golden('global_attn_grad.npz')
        pre = f'op/{name}/'
        i = [s[0] for s in SHAPES].index(name)
        _, self.B, self.T, self.C, self.heads, lens, holes, _ = SHAPES[i]
        self.name, step = name, float(g.t(pre + 'step'))
        self.x, self.up = (g.t(pre + k).float().mul(0.25).transpose(1, 2).contiguous() for k in ('x', 'up'))
        self.mask = g.t(pre + 'mask')
        assert torch.equal(self.mask, shape_mask(self.B, self.T, lens, holes))
        self.sd = {k: v.float() * step for k, v in g.sub(pre + 'param/').items()}
        self.rows = g.t(pre + 'rows')
        self.e_ref, self.top = g.js(pre + 'e_ref'), g.js(pre + 'top')
        self.g32, self.g64, self.gp32, self.gp64 = {}, {}, {}, {}
        for k in g.keys():
            if k.startswith(pre) and k.endswith('/32'):
                key = k[len(pre):-3]
                a, d = g.t(k), g.t(k[:-2] + 'd')
                (self.gp32 if key.startswith('gp/') else self.g32)[key[3:] if key.startswith('gp/') else key] = a
                (self.gp64 if key.startswith('gp/') else self.g64)[key[3:] if key.startswith('gp/') else key] = a.double() + d.double()
        lin = lambda z, n: z @ self.sd[f'{n}.weight'][:, :, 0].t() + self.sd[f'{n}.bias']
        self.q, self.k, self.v = lin(self.x, 'query'), lin(self.x, 'key'), lin(self.x, 'value')
        self.do = self.up @ self.sd['proj.weight'][:, :, 0]

    def at_rows(self, t):
        return t.reshape(-1, t.size(-1))[self.rows.to(t.device)]


def fixture_rule(tag, got_rows, f, key, label='GAERR'):
    """the gradient rule on the stored rows of fixture tensor `key`, with e_ref and max |g64| of the whole tensor as recorded"""
    got, g64 = got_rows.detach().cpu().double(), f.g64[key]
    assert got.shape == g64.shape and bool(torch.isfinite(got).all()), (tag, got.shape, g64.shape)
    e_ref, top, e_gpu = f.e_ref[key], f.top[key], float((got - g64).abs().max())
    bound = max(4 * e_ref, FLOOR * top)
    print(f'{label} {tag}: max|g64| {top:.3e} e_ref {e_ref:.3e} e_gpu {e_gpu:.3e} bound {bound:.3e} ratio {e_gpu / bound:.3f}')
    assert e_gpu <= bound, (tag, e_gpu, bound)
    return e_gpu, bound
