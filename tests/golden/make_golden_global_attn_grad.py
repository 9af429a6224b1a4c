"""Generate tests/golden/global_attn_grad.npz: forward values and `backward()` results of the reference's own MaskedMHA and
TransformerEncoder (libs/modeling/blocks.py) with window_size = 0 -- global self-attention -- in fp32 and, from the same module cast to
fp64, in fp64.

Run where the reference is importable (not on the GPU machine):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_global_attn_grad.py

Operator cases `op/<shape>` -- the rows marked F of global_attn_grad_ref.SHAPES: below_tile (B 2, T 37, C 64, 2 heads, lengths 37 / 20),
past_tile (2 x 65, C 128, 2 heads, lengths 65 / 64) and two_tiles_tail (2 x 130, C 256, 4 heads, lengths 130 / 71, the second with holes
inside its valid part).  Each is MaskedMHA(C, heads, window_size=0) as self attention on one input x with a random upstream gradient
`up` on EVERY position (the global branch has no query mask); the scalar differentiated is sum(out * up).  The input, `up` and the
parameters lie on a coarse grid (x, up: multiples of 1/4 in [-2, 2]; weights and biases: multiples of `step` = 1/32, query and key
weights doubled so that the softmax is not flat; all three are stored as int8 multiples of their step), so the three projections and
the gradient that reaches the attention core are EXACT in fp32: q, k, v and dO are the same numbers in both precisions (asserted), and the difference between the two runs' dQ / dK / dV is the error
of the fp32 attention core alone.  The file holds x, up, mask and the parameters -- the core's operands follow from them exactly, in
any summation order -- and, by the project's scheme (g32 and d = fp32(g64 - g32), g64 = g32 + d in fp64):
    dq, dk, dv      at the rows `rows` (all rows of below_tile; of the two larger shapes the rows around every tile edge, every
                    length and every hole -- a committed file is limited to 1 MiB); e_ref/<tensor> is max |g32 - g64| and
                    top/<tensor> max |g64|, both over ALL rows
    gx              the gradient of x, below_tile only
    gp/<parameter>  every parameter of below_tile; the four biases of the larger shapes

Block cases `enc/s1`, `enc/s2`: TransformerEncoder(32, stride, n_heads=1, window_size=0) (one head of 32 channels: the block has
12 C^2 parameters, and two precisions of two cases have to fit the file) on B 2, attention over 37 positions with lengths 37 / 20 and
two holes (stride 2: T = 74, lengths 74 / 40), parameters perturbed as make_golden_enc_grad.py perturbs them, upstream gradient zero
at padded output positions.  Per case x, mask, up, and out, gx and the gradient of each of the 27 parameters in full, as (32, d) pairs.

The archive is written with fixed time stamps: two runs give the same bytes."""
import importlib
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402
import global_attn_grad_ref as R  # noqa: E402

LIMIT = 1 << 20
ENC = dict(E=32, heads=1, B=2, Ta=37, lens=(37, 20), holes=(5, 11))
ENC_CASES = {'s1': 1, 's2': 2}


def reference_blocks():
    """libs/modeling/blocks.py alone, without the package's __init__ (which pulls in the whole model zoo)"""
    pkg = types.ModuleType('ref_modeling')
    pkg.__path__ = [os.path.join(os.environ.get('DCF_REFERENCE', MG.REF), 'libs', 'modeling')]
    sys.modules['ref_modeling'] = pkg
    return importlib.import_module('ref_modeling.blocks')


def save_fixed(path, d):
    """np.savez_compressed with fixed time stamps (numpy stamps each member with the clock)"""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for k, v in MG.npify(d).items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print(os.path.basename(path), os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < LIMIT, path


def stored_rows(name, B, T, lens, holes):
    """flat row indices b * T + t that the fixture keeps for shape `name`"""
    if B * T <= 80:
        return list(range(B * T))
    keep = set()
    for b in range(B):
        ts = {0, 31, T - 1, lens[b] - 1, lens[b]}
        for edge in range(64, T + 1, 64):
            ts |= {edge - 1, edge}
        if b == B - 1:
            ts |= set(holes[:4])
        keep |= {b * T + t for t in ts if 0 <= t < T}
    return sorted(keep)


def pair(out, key, g32, g64, rows=None):
    """g32 and d = fp32(g64 - g32) under `key`, at `rows` of the flattened (B * T, C) tensor if given; returns e_ref over everything"""
    e = float((g32.double() - g64).abs().max())
    if rows is not None:
        g32, g64 = g32.reshape(-1, g32.size(-1))[rows], g64.reshape(-1, g64.size(-1))[rows]
    d = (g64 - g32.double()).float()
    assert float((g32.double() + d.double() - g64).abs().max()) <= 2.0 ** -23 * max(float(d.abs().max()), 1e-300), key
    out[f'{key}/32'], out[f'{key}/d'] = g32.contiguous(), d.contiguous()
    return e


def tm(x):
    return x.transpose(1, 2).contiguous()


def op_case(BL, name, B, T, C, heads, lens, holes, rs):
    grid = lambda a, step: torch.from_numpy(np.round(a / step) * step).float()
    x = grid(np.clip(rs.standard_normal((B, C, T)), -2, 2), 0.25)
    up = grid(np.clip(rs.standard_normal((B, C, T)), -2, 2), 0.25)
    step = 1.0 / 32
    small = name == 'below_tile'
    mask = R.shape_mask(B, T, lens, holes)
    torch.manual_seed(31)
    proto = BL.MaskedMHA(C, n_heads=heads, window_size=0, attn_pdrop=0.0, proj_pdrop=0.0)
    with torch.no_grad():
        for k, p in proto.named_parameters():
            if k.endswith('bias'):
                p.add_(0.1 * torch.from_numpy(rs.standard_normal(tuple(p.shape))).float())
            if k.startswith(('query.weight', 'key.weight')):
                p.mul_(2.0)
            p.copy_(torch.round(p / step) * step)
    as_i8 = lambda z, st: (lambda i: (i.to(torch.int8), bool(torch.equal(i.float() * st, z)) and float(i.abs().max()) <= 127))(torch.round(z / st))
    out = {'mask': mask, 'step': step}
    for k, z, st in [('x', x, 0.25), ('up', up, 0.25)] + [(f'param/{k}', p.detach(), step) for k, p in proto.state_dict().items()]:
        out[k], ok = as_i8(z, st)
        assert ok, (name, k)
    rows = stored_rows(name, B, T, lens, holes)
    out['rows'] = torch.tensor(rows)
    run = {}
    for tag, dt in (('32', torch.float32), ('64', torch.float64)):
        mha = BL.MaskedMHA(C, n_heads=heads, window_size=0, attn_pdrop=0.0, proj_pdrop=0.0)
        mha.load_state_dict(proto.state_dict())
        mha = mha.to(dt)
        tap = {}

        def keep(key):
            def hook(m, a, o):
                o.retain_grad()
                tap[key] = o
            return hook

        for key in ('query', 'key', 'value'):
            getattr(mha, key).register_forward_hook(keep(key))
        mha.proj.register_forward_pre_hook(lambda m, a: (a[0].retain_grad(), tap.update(ctx=a[0]))[1])
        xin = x.to(dt).clone().requires_grad_(True)
        y = mha(xin, xin, xin, mask[:, None])
        (y * up.to(dt)).sum().backward()
        run[tag] = dict(out=tm(y.detach()), gx=tm(xin.grad), q=tm(tap['query'].detach()), k=tm(tap['key'].detach()), v=tm(tap['value'].detach()),
                        do=tm(tap['ctx'].grad), dq=tm(tap['query'].grad), dk=tm(tap['key'].grad), dv=tm(tap['value'].grad),
                        gp={k: p.grad for k, p in mha.named_parameters()})
    a, b = run['32'], run['64']
    for key in ('q', 'k', 'v', 'do'):                          # the operands of the core: the same numbers in both precisions
        assert torch.equal(a[key].double(), b[key]), (name, key)
    # the restatement on the reference's operands, in fp64, against the reference's fp64 backward
    g = R.grads(b['q'], b['k'], b['v'], mask, b['do'], heads)
    for key, mine in zip(('dq', 'dk', 'dv'), g):
        err, top = float((mine - b[key]).abs().max()), float(b[key].abs().max())
        assert err <= 1e-12 * top, (name, key, err, top)
        assert bool((b[key][~mask] == 0).all()) or key == 'dq', (name, key)
    eref = {}
    for key in ('dq', 'dk', 'dv') + (('gx',) if small else ()):
        eref[key] = pair(out, key, a[key], b[key], rows)
    for k in a['gp']:
        if small or k.endswith('bias'):
            eref[f'gp/{k}'] = pair(out, f'gp/{k}', a['gp'][k], b['gp'][k])
    out['e_ref'] = eref
    out['top'] = {key: float(b[key].abs().max()) for key in ('dq', 'dk', 'dv', 'gx', 'out')}
    print(name, 'rows', len(rows), 'e_ref', {k: f'{v:.2e}' for k, v in eref.items() if '/' not in k}, 'top', {k: f'{v:.2e}' for k, v in out['top'].items()})
    return out


def enc_case(BL, proto, stride, rs):
    t = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32))
    E, B, T = ENC['E'], ENC['B'], ENC['Ta'] * stride
    mask = torch.arange(T)[None, :] < (torch.tensor(ENC['lens']) * stride)[:, None]
    for h in ENC['holes']:
        mask[-1, h * stride] = False
    x = t(B, E, T)
    up = t(B, E, T // stride) * mask[:, None, ::stride]
    out = {'x': x, 'mask': mask, 'up': up}
    run = {}
    for tag, dt in (('32', torch.float32), ('64', torch.float64)):
        blk = BL.TransformerEncoder(E, stride, n_heads=ENC['heads'], window_size=0, attn_pdrop=0.0, proj_pdrop=0.0, path_pdrop=0.0)
        blk.load_state_dict(proto.state_dict())
        blk = blk.to(dt).train()
        xin = x.to(dt).clone().requires_grad_(True)
        y, mo = blk(xin, mask[:, None])
        (y * up.to(dt)).sum().backward()
        assert torch.equal(mo[:, 0], mask[:, ::stride])
        out['mask_out'] = mo[:, 0]
        run[tag] = dict(out=y.detach(), gx=xin.grad, gp={k: p.grad for k, p in blk.named_parameters()})
        assert len(run[tag]['gp']) == 27 and all(g is not None and bool(torch.isfinite(g).all()) for g in run[tag]['gp'].values())
    pair(out, 'out', run['32']['out'], run['64']['out'])
    pair(out, 'gx', run['32']['gx'], run['64']['gx'])
    for k in run['32']['gp']:
        pair(out, f'gp/{k}', run['32']['gp'][k], run['64']['gp'][k])
    return out


# ---------------------------------------------------------------------------------------------- the whole step, case g1
G1_SEED = 20271
G1_TARGETS = [[30.25, 35.25], [8.5, 19.5], [44.5, 75.5]]
PART_CAP = 100000                                               # parameters per gradient file (8 bytes each, 1 MiB per committed file)


def step_case(seed=G1_SEED, targets=G1_TARGETS):
    """tests/golden/step_grad_global*.npz: case g1 of the whole training step, built exactly as make_golden_step_grad.py builds s1 / s2
    (its main() runs, with its conditions on the reference alone) on E = 64 with 2 heads and mha_win_size = 0: global attention over
    heads of 32 channels in the stem and in every pyramid level.  3 levels, vid_stride 1, no msf (the gate is and-ed into the mask:
    attention runs on masks with holes), T = 80 with lengths 80 / 55, two videos, three queries, text_size [2, 1].  The files are
    read by tests/global_step_fixture.py through tests/step_grad_ref.Fixture; the parameter gradients and the state dict are split over
    as many files as the size limit of a committed file asks for."""
    import make_golden_step_grad as SG
    MG.install_stubs()
    from libs.modeling.model import PtTransformerEarlyFusionIterative
    kw = dict(SG.BASE, E=64, n_heads=2, win=0, vid_stride=1, msf=False, max_seq_len=128)
    net = PtTransformerEarlyFusionIterative(MG.make_opt(**kw).clone(), second_fusion=False)
    groups = {}
    for k, p in net.named_parameters():                        # modules three names deep, packed in order into parts of at most PART_CAP
        groups['.'.join(k.split('.')[:3])] = groups.get('.'.join(k.split('.')[:3]), 0) + p.numel()
    parts, size = {}, 0
    for g, n in groups.items():
        if not parts or size + n > PART_CAP:
            parts[f'p{len(parts)}'], size = (), 0
        key = f'p{len(parts) - 1}'
        parts[key], size = parts[key] + (g + '.' if g.count('.') == 2 and not g.endswith(('weight', 'bias', 'scale')) else g,), size + n
    SG.PARTS = parts
    SG.CASES = {'global': dict(opt=kw, second_fusion=False, T=80, lens=[80, 55], center_sampling='none', reg_loss='giou', seed=seed, targets=targets)}

    def save(name, d):
        """the state dict leaves the core file for files of its own, PART_CAP values each (tests/global_step_fixture.py merges them)"""
        chunks, size = [{}], 0
        for k in [k for k in d if k.startswith('param/')]:
            v = d.pop(k)
            if size + v.numel() > 2 * PART_CAP and chunks[-1]:
                chunks.append({})
                size = 0
            chunks[-1][k], size = v, size + v.numel()
        for i, c in enumerate(c for c in chunks if c):
            save_fixed(os.path.join(HERE, name.replace('.npz', f'_params_{i}.npz')), c)
        save_fixed(os.path.join(HERE, name), d)

    SG.save = save
    SG.main()


def main():
    if '--step-only' in sys.argv:
        return step_case()
    BL = reference_blocks()
    out = {'meta': {'shapes': [s[0] for s in R.SHAPES if s[7]], 'enc': ENC, 'enc_cases': ENC_CASES}}
    for i, (name, B, T, C, heads, lens, holes, in_fixture) in enumerate(R.SHAPES):
        if in_fixture:
            for k, v in op_case(BL, name, B, T, C, heads, lens, holes, np.random.RandomState(20260 + i)).items():
                out[f'op/{name}/{k}'] = v
    rs = np.random.RandomState(20270)
    t = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32))
    torch.manual_seed(13)
    proto = BL.TransformerEncoder(ENC['E'], 1, n_heads=ENC['heads'], window_size=0, attn_pdrop=0.0, proj_pdrop=0.0, path_pdrop=0.0)
    with torch.no_grad():
        for k, p in proto.named_parameters():
            if k.endswith('drop_path_attn.scale') or k.endswith('drop_path_ffn.scale'):
                p.copy_(0.5 + 0.25 * t(*p.shape))
            elif k.endswith('bias'):
                p.add_(0.1 * t(*p.shape))
            elif 'norm' in k or k.startswith('ln_'):           # the LayerNorm weights
                p.add_(0.1 * t(*p.shape))
    for k, p in proto.state_dict().items():
        out[f'enc/param/{k}'] = p.clone()
    for name, stride in ENC_CASES.items():
        for k, v in enc_case(BL, proto, stride, rs).items():
            out[f'enc/{name}/{k}'] = v
    save_fixed(os.path.join(HERE, 'global_attn_grad.npz'), out)
    step_case()


if __name__ == '__main__':
    main()
