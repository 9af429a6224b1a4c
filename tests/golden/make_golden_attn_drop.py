"""Generate tests/golden/attn_drop_ops.npz: the reference's own MaskedMHA (libs/modeling/blocks.py) with a local window and
attn_pdrop = 0.25, the draws of its ``attn_drop`` replaced by the project's stated stream (tests/philox_ref.py,
include/decafnet_hip_attn_drop.h), forward and `backward()` in fp32 and, from the same module cast to fp64, in fp64.

Run where the reference is importable (not on the GPU machine):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_attn_drop.py

Cases: E 64, 2 heads, 2 sequences, the second with a padded tail; w9 = window 9 at T 40, w19 = window 19 at T 45 (the reference's
chunked layout needs T % (window // 2) == 0, which 40 is not for window 19).  Each case is self attention on one input x (B, E, T) with
a random upstream gradient on every position; the scalar differentiated is sum(y * up).  Per case: x, mask, up, the key / site / p, the
fp32 / fp64 output and input gradient, and per parameter the fp32 / fp64 gradient.

The element index is the flat index of the (bs, H, T, W) tensor the reference hands to ``attn_drop`` (blocks.py:368).  That slot j of row
t is key t - W // 2 + j is ASSERTED here on the reference's own tensor: the fp64 output is recomputed from the banded restatement
(tests/attn_drop_ref.py) with the keep bits placed by that rule and must agree to 1e-12.

Conditions on the reference alone, asserted here and again on the committed file by tests/test_attn_drop_cpu.py:
e_ref <= 2^-15 max|g_64| for every gradient tensor but key.bias (zero by symmetry); the key is picked by search so that the site both
drops and keeps and at least one (row, head) of each case loses all of its valid keys."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402
import make_golden_dropout as MD  # noqa: E402
import attn_drop_ref as R  # noqa: E402
import philox_ref as P  # noqa: E402
from make_golden_attn_grad import reference_blocks  # noqa: E402

E, HEADS, B, PDROP = 64, 2, 2, 0.25
GROUP, LAYER = P.G_BRANCH, 2
CASES = {'w9': (9, 40, [40, 29]), 'w19': (19, 45, [45, 31])}
KEY0 = 0x9E3779B97F4A7C15


class MapStream(MD.Stream):
    """MD.Stream with the attention map: a 4-D (bs, H, T, W) tensor at sub DROP_ATTN, element index = flat index"""

    def attn(self, mod, x):
        assert mod.training and mod.p > 0 and x.ndim == 4 and x.is_contiguous(), x.shape
        s = P.site(GROUP, LAYER, R.DROP_ATTN)
        keep = P.keep(self.seed, s, np.arange(x.numel(), dtype=np.uint64).reshape(tuple(x.shape)), mod.p)
        self.log[s] = (tuple(x.shape), keep)
        return x * (torch.from_numpy(keep).to(x.dtype) * float(P.scale(mod.p)))


def dead_rows(keep, mask, window):
    """(row, head)s that are live and lose every valid key"""
    valid = R.valid_slots(mask, window)[:, None].expand_as(keep)
    return int((valid.any(-1) & ~(valid & keep).any(-1)).sum())


def pick_key(start):
    """the first key from `start` on under which every case both drops and keeps and has a fully dropped (row, head)"""
    key = start
    while True:
        ok = True
        for window, T, lens in CASES.values():
            mask = torch.arange(T)[None, :] < torch.tensor(lens)[:, None]
            keep = R.window_keep(key, P.site(GROUP, LAYER, R.DROP_ATTN), B, HEADS, T, window, PDROP)
            ok = ok and bool(keep.any()) and not bool(keep.all()) and dead_rows(keep, mask, window) >= 1
        if ok:
            return key
        key += 1


def main():
    BL = reference_blocks()
    rs = np.random.RandomState(20261)
    t = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32))
    torch.manual_seed(13)
    proto = BL.MaskedMHA(E, n_heads=HEADS, window_size=9, attn_pdrop=PDROP, proj_pdrop=0.0)
    with torch.no_grad():
        for k, p in proto.named_parameters():                  # biases away from their small initialisation
            if k.endswith('bias'):
                p.add_(0.1 * t(*p.shape))
    key = pick_key(KEY0)
    site = P.site(GROUP, LAYER, R.DROP_ATTN)
    out = {'meta': {'E': E, 'heads': HEADS, 'p': PDROP, 'key': str(key), 'site': site, 'group': GROUP, 'layer': LAYER,
                    'cases': {n: {'window': w, 'T': T, 'lens': lens} for n, (w, T, lens) in CASES.items()}}}
    sd = {k: p.clone() for k, p in proto.state_dict().items()}
    for k, p in sd.items():
        out[f'param/{k}'] = p
    for name, (window, T, lens) in CASES.items():
        x = t(B, E, T)
        mask = torch.arange(T)[None, :] < torch.tensor(lens)[:, None]
        up = t(B, E, T)
        out[f'{name}/x'], out[f'{name}/mask'], out[f'{name}/up'] = x, mask, up
        res = {}
        for tag, dt in (('32', torch.float32), ('64', torch.float64)):
            mha = BL.MaskedMHA(E, n_heads=HEADS, window_size=window, attn_pdrop=PDROP, proj_pdrop=0.0)
            mha.load_state_dict(sd)
            mha = mha.to(dt).train()
            stream = MapStream(key)
            mha.attn_drop.forward = lambda z, mod=mha.attn_drop, st=stream: st.attn(mod, z)
            xin = x.to(dt).clone().requires_grad_(True)
            y = mha(xin, xin, xin, mask[:, None])
            (y * up.to(dt)).sum().backward()
            (shape, keep), = stream.log.values()
            assert shape == (B, HEADS, T, window), shape
            res[tag] = (y.detach(), xin.grad, {k: p.grad for k, p in mha.named_parameters()})
            out[f'{name}/out{tag}'], out[f'{name}/gx{tag}'] = y.detach(), xin.grad
            for k, g in res[tag][2].items():
                out[f'{name}/gp{tag}/{k}'] = g
        # the slot order, on the reference's own tensor
        keep = torch.from_numpy(keep)
        assert torch.equal(keep, R.window_keep(key, site, B, HEADS, T, window, PDROP))
        xt = x.double().transpose(1, 2)
        y_band = R.masked_mha_drop(xt, xt, xt, mask, {k: v.double() for k, v in sd.items()}, HEADS, window, keep, PDROP).transpose(1, 2)
        err = float((y_band - res['64'][0]).abs().max()) / float(res['64'][0].abs().max())
        assert err <= 1e-12, f'{name}: slot j of row t is not key t - W // 2 + j in the reference ({err:.3e})'
        wrong = R.masked_mha_drop(xt, xt, xt, mask, {k: v.double() for k, v in sd.items()}, HEADS, window, keep.flip(-1), PDROP).transpose(1, 2)
        assert float((wrong - res['64'][0]).abs().max()) / float(res['64'][0].abs().max()) > 1e-3, 'the check tells the orders apart'
        # the conditions on the reference alone
        assert bool(keep.any()) and not bool(keep.all()) and dead_rows(keep, mask, window) >= 1
        for k in ['x'] + list(res['64'][2]):
            g64, g32 = (res[tag][1] if k == 'x' else res[tag][2][k] for tag in ('64', '32'))
            e_ref, top = float((g32.double() - g64).abs().max()), float(g64.abs().max())
            print(f'{name} {k}: max|g64| {top:.3e} e_ref {e_ref:.3e} ratio {e_ref / (2.0 ** -15 * top):.3f}')
            assert k == 'key.bias' or e_ref <= 2.0 ** -15 * top, (name, k)
        print(f'{name}: slot order confirmed ({err:.1e}), {dead_rows(keep, mask, window)} fully dropped (row, head)s, key {key:#x}')
    path = os.path.join(HERE, 'attn_drop_ops.npz')
    np.savez_compressed(path, **MG.npify(out))
    print('attn_drop_ops.npz', os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < (1 << 20)


if __name__ == '__main__':
    main()
