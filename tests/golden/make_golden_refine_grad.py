"""Generate tests/golden/refine_grad*.npz: forward values and `backward()` results of the reference's own
PtTransformerEarlyFusionIterative.fuse_and_predict (libs/modeling/model.py:442-471: cls_head, the stacking of the upsampled logits,
the refinement TCN, the pooling chain, cls_head2 and reg_head) in fp32 and, from the same model cast to fp64, in fp64.

Run where the reference is importable (not on the GPU machine):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_refine_grad.py

The model is built the way make_golden.py builds its end-to-end models (make_opt + the reference's constructor, second_fusion off) at
E = 32, L = 3 pyramid levels, and put in .eval(): that only switches the Dropouts of the refinement TCN off, autograd still works.
Inputs: three query rows of T0 = 40 with lengths [40, 27, 33]; level l has T0 >> l positions and the mask `mask0[:, ::2^l]`.  Biases
and LayerNorm weights are moved off their initial values by 0.1 N(0, 1), the Scales of the regression head set to (1, 0.7, 1.3).  The
upstream gradients are N(0, 1) on all three outputs, padded positions included; the scalar differentiated is
sum_levels sum(logits1 * up1) + sum(logits2 * up2) + sum(offsets * up3).

Files (each below the 1 MiB limit of a committed file):
    refine_grad.npz         meta, opt_kwargs, param/<name> (cls_head, refine, cls_head2, reg_head), per level fpn/l<i>, mask/l<i>,
                            up1 / up2 / up3, and logits1_<tag> / logits2_<tag> / offsets_<tag> / gfpn_<tag> for tag 32 and 64
    refine_grad_gp32.npz / refine_grad_gp64.npz    <name> -> the gradient of that parameter
Parameters, inputs and upstream gradients are rounded to multiples of 2^-10 so that the first file compresses; nothing else is rounded."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402

OPT = dict(D=32, E=32, TE=32, text_in=32, n_levels=3, win=5, n_heads=2, sn=8, sratio=0.5, msf=True, norm=True, max_seq_len=64,
           text_layers=1, text_max_len=24)
T0, LENS = 40, [40, 27, 33]
MODULES = ('cls_head.', 'refine.', 'cls_head2.', 'reg_head.')
LIMIT = 1 << 20


def coarse(x):
    return torch.round(x * 1024) / 1024


def save(name, d):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **MG.npify(d))
    print(name, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < LIMIT, name


def main():
    MG.install_stubs()
    from libs.modeling.model import PtTransformerEarlyFusionIterative
    rs = np.random.RandomState(20255)
    t = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32))
    torch.manual_seed(17)
    L, E, B = OPT['n_levels'], OPT['E'], len(LENS)
    proto = PtTransformerEarlyFusionIterative(MG.make_opt(**OPT).clone(), second_fusion=False).eval()
    with torch.no_grad():
        for k, p in proto.named_parameters():
            if not k.startswith(MODULES):
                continue
            if '.scales.' in k:
                p.fill_({'0': 1.0, '1': 0.7, '2': 1.3}[k.split('.')[2]])
            elif k.endswith('bias') or '.norm' in k:
                p.add_(0.1 * t(*p.shape))
            p.copy_(coarse(p))
    names = [k for k, _ in proto.named_parameters() if k.startswith(MODULES)]
    core = {'meta': {'T0': T0, 'lens': LENS, 'L': L, 'E': E, 'n_params': len(names)}, 'opt_kwargs': OPT}
    for k in names:
        core[f'param/{k}'] = proto.state_dict()[k].clone()
    mask0 = torch.arange(T0)[None, :] < torch.tensor(LENS)[:, None]
    fpn = [coarse(t(B, E, T0 >> l)) for l in range(L)]
    masks = [mask0[:, ::1 << l] for l in range(L)]
    ups = {'up1': [coarse(t(B, T0 >> l)) for l in range(L)], 'up2': [coarse(t(B, T0 >> l)) for l in range(L)],
           'up3': [coarse(t(B, T0 >> l, 2)) for l in range(L)]}
    for l in range(L):
        core[f'fpn/l{l}'], core[f'mask/l{l}'] = fpn[l], masks[l]
        for k, v in ups.items():
            core[f'{k}/l{l}'] = v[l]
    for tag, dt in (('32', torch.float32), ('64', torch.float64)):
        net = PtTransformerEarlyFusionIterative(MG.make_opt(**OPT).clone(), second_fusion=False)
        net.load_state_dict(proto.state_dict())
        net = net.to(dt).eval()
        xin = [x.to(dt).clone().requires_grad_(True) for x in fpn]
        l1, l2, off, mo = net.fuse_and_predict(xin, [m[:, None] for m in masks], None, None)
        total = sum((a * u.to(dt)).sum() for outs, key in ((l1, 'up1'), (l2, 'up2'), (off, 'up3')) for a, u in zip(outs, ups[key]))
        total.backward()
        for l in range(L):
            assert l1[l].shape == (B, T0 >> l) and l2[l].shape == (B, T0 >> l) and off[l].shape == (B, T0 >> l, 2)
            assert torch.equal(mo[l].reshape(B, -1), masks[l])
            core[f'logits1_{tag}/l{l}'], core[f'logits2_{tag}/l{l}'], core[f'offsets_{tag}/l{l}'] = l1[l].detach(), l2[l].detach(), off[l].detach()
            core[f'gfpn_{tag}/l{l}'] = xin[l].grad
        grads = {k: p.grad for k, p in net.named_parameters() if k.startswith(MODULES)}
        assert list(grads) == names and all(g is not None for g in grads.values())
        save(f'refine_grad_gp{tag}.npz', grads)
    save('refine_grad.npz', core)


if __name__ == '__main__':
    main()
