"""Generate tests/golden/attn_drop_ops_dense.npz: the global branch of the reference's own MaskedMHA (libs/modeling/blocks.py:374-389)
with attn_pdrop = 0.25, the draws of its ``attn_drop`` replaced by the project's stated stream, forward and `backward()` in fp32 and,
from the same module cast to fp64, in fp64 -- the cases of make_golden_attn_drop.py that do not fit its file (1 MiB per committed file).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_attn_drop_dense.py

Cases: E 64, 2 heads.  `global`: self attention on x (2, E, 70) with a key mask that has a hole in sequence 0 and a padded tail in
sequence 1.  `cross`: queries (2, E, 40) on keys / values (3, E, 24) with padded keys, ``kv_size = (2, 1)``.  A random upstream gradient
on every position; the scalar differentiated is sum(y * up).  Per case the inputs, the key / site / p, y, and the gradients at the inputs
and at every parameter in both precisions.  The element index is the flat index of the (bs, H, T, Lk) tensor handed to ``attn_drop``
(blocks.py:388); that it is key-minor is asserted by recomputing y in fp64 from tests/attn_drop_ref.py (1e-12).  Conditions asserted
here and on the committed file by tests/test_attn_drop_cpu.py: e_ref <= 2^-15 max|g_64| for every gradient tensor but key.bias, and the
key is picked by search so that the site both drops and keeps in every case."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402
import attn_drop_ref as R  # noqa: E402
import attn_grad_ref as G  # noqa: E402
import philox_ref as P  # noqa: E402
from make_golden_attn_drop import MapStream, PDROP  # noqa: E402
from make_golden_attn_grad import reference_blocks  # noqa: E402

E, HEADS = 64, 2
KEY0 = 0xD1B54A32D192ED03


def restated(q_in, kv_in, kmask, sd, kv_size, keep):
    """MaskedMHA.forward, global branch with attn_drop, on token-major fp64 inputs (the projected query repeated by kv_size, :352-355)"""
    q, k, v = G.conv1(q_in, sd, 'query'), G.conv1(kv_in, sd, 'key'), G.conv1(kv_in, sd, 'value')
    if kv_size is not None:
        q = q.repeat_interleave(torch.tensor(kv_size), dim=0)
    return G.conv1(R.dense_attention_drop(q, k, v, kmask, HEADS, keep, PDROP), sd, 'proj')


def main():
    BL = reference_blocks()
    rs = np.random.RandomState(20262)
    t = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32))
    torch.manual_seed(17)
    proto = BL.MaskedMHA(E, n_heads=HEADS, window_size=0, attn_pdrop=PDROP, proj_pdrop=0.0)
    with torch.no_grad():
        for k, p in proto.named_parameters():
            if k.endswith('bias'):
                p.add_(0.1 * t(*p.shape))
    sd = {k: p.clone() for k, p in proto.state_dict().items()}
    gmask = torch.ones(2, 70, dtype=torch.bool)
    gmask[0, 31], gmask[1, 52:] = False, False
    cmask = torch.arange(24)[None, :] < torch.tensor([24, 17, 9])[:, None]
    xg = t(2, E, 70)
    cases = {'global': dict(q=xg, kv=xg, mask=gmask, kv_size=None, up=t(2, E, 70)),
             'cross': dict(q=t(2, E, 40), kv=t(3, E, 24), mask=cmask, kv_size=[2, 1], up=t(3, E, 40))}
    key = KEY0
    out = {'meta': {'E': E, 'heads': HEADS, 'p': PDROP, 'key': str(key), 'site': P.site(P.G_FUSION, 1, R.DROP_ATTN), 'group': P.G_FUSION, 'layer': 1,
                    'cases': {n: {'kv_size': c['kv_size']} for n, c in cases.items()}}}
    for k, p in sd.items():
        out[f'param/{k}'] = p
    import make_golden_attn_drop as MA
    MA.GROUP, MA.LAYER = P.G_FUSION, 1
    for name, c in cases.items():
        self_attn = c['kv'] is c['q']
        for z in ('q', 'kv', 'mask', 'up'):
            if not (self_attn and z == 'kv'):
                out[f'{name}/{z}'] = c[z]
        res = {}
        for tag, dt in (('32', torch.float32), ('64', torch.float64)):
            mha = BL.MaskedMHA(E, n_heads=HEADS, window_size=0, attn_pdrop=PDROP, proj_pdrop=0.0)
            mha.load_state_dict(sd)
            mha = mha.to(dt).train()
            stream = MapStream(key)
            mha.attn_drop.forward = lambda z, mod=mha.attn_drop, st=stream: st.attn(mod, z)
            qin = c['q'].to(dt).clone().requires_grad_(True)
            kvin = qin if self_attn else c['kv'].to(dt).clone().requires_grad_(True)
            y = mha(qin, kvin, kvin, c['mask'][:, None], None if c['kv_size'] is None else torch.tensor(c['kv_size']))
            (y * c['up'].to(dt)).sum().backward()
            (shape, keep), = stream.log.values()
            res[tag] = dict(y=y.detach(), gq=qin.grad, gkv=None if self_attn else kvin.grad, gp={k: p.grad for k, p in mha.named_parameters()})
            out[f'{name}/out{tag}'], out[f'{name}/gq{tag}'] = y.detach(), qin.grad
            if not self_attn:
                out[f'{name}/gkv{tag}'] = kvin.grad
            for k, g in res[tag]['gp'].items():
                out[f'{name}/gp{tag}/{k}'] = g
        keep = torch.from_numpy(keep)
        Bk, Lk, T = c['kv'].size(0), c['kv'].size(2), c['q'].size(2)
        assert shape == (Bk, HEADS, T, Lk) and torch.equal(keep, R.dense_keep(key, out['meta']['site'], Bk, HEADS, T, Lk, PDROP))
        assert bool(keep.any()) and not bool(keep.all())
        sd64 = {k: v.double() for k, v in sd.items()}
        tm = lambda z: z.double().transpose(1, 2)
        y_ref = restated(tm(c['q']), tm(c['kv']), c['mask'], sd64, c['kv_size'], keep).transpose(1, 2)
        err = float((y_ref - res['64']['y']).abs().max()) / float(res['64']['y'].abs().max())
        assert err <= 1e-12, (name, err)
        pairs = [('gq', res['64']['gq'], res['32']['gq'])] + ([] if self_attn else [('gkv', res['64']['gkv'], res['32']['gkv'])])
        pairs += [(k, res['64']['gp'][k], res['32']['gp'][k]) for k in res['64']['gp']]
        for k, g64, g32 in pairs:
            e_ref, top = float((g32.double() - g64).abs().max()), float(g64.abs().max())
            assert k == 'key.bias' or e_ref <= 2.0 ** -15 * top, (name, k, e_ref, top)
        print(f'{name}: index order confirmed ({err:.1e}), kept {int(keep.sum())} of {keep.numel()}')
    path = os.path.join(HERE, 'attn_drop_ops_dense.npz')
    np.savez_compressed(path, **MG.npify(out))
    print('attn_drop_ops_dense.npz', os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < (1 << 20)


if __name__ == '__main__':
    main()
