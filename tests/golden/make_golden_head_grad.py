"""Generate tests/golden/head_grad.npz and head_grad_reg.npz: forward values and `backward()` results of the reference's own
ClsHead and RegHead (libs/modeling/head.py, 3 levels, embd_dim = 64) in fp32 and, from the same modules cast to fp64, in fp64.

Run where the reference is importable (not on the GPU machine):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_head_grad.py

Levels: l0 = (B 2, T 200), ragged mask, sequence 1 with a fully padded tail of 80 rows; l1 = a one-row level (T 1).  Upstream
gradients are random and zero on padded positions; the scalar differentiated is sum_levels sum(out * up), so the parameter
gradients add up over the levels like `.grad +=`.  Per head: parameters, per level the fp32 / fp64 outputs and input gradients,
per parameter the fp32 / fp64 gradient.  The inputs live in head_grad.npz (with ClsHead); RegHead's results are a file of their
own so that each stays under the size of the other fixtures."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402

E, B = 64, 2
LEVELS = [(200, [173, 120]), (1, [1, 1])]


def reference_heads():
    """libs/modeling/head.py and blocks.py alone, without the package's __init__ (which pulls in the whole model zoo)"""
    pkg = types.ModuleType('ref_modeling')
    pkg.__path__ = [os.path.join(os.environ.get('DCF_REFERENCE', MG.REF), 'libs', 'modeling')]
    sys.modules['ref_modeling'] = pkg
    return importlib.import_module('ref_modeling.head')


def main():
    H = reference_heads()
    rs = np.random.RandomState(20251)
    t = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32))
    xs = [t(B, E, T) for T, _ in LEVELS]
    masks = [torch.arange(T)[None, :] < torch.tensor(lens)[:, None] for T, lens in LEVELS]
    common = {}
    for i, (x, m) in enumerate(zip(xs, masks)):
        common[f'x/l{i}'] = x
        common[f'mask/l{i}'] = m
    files = {'cls': common, 'reg': {}}
    torch.manual_seed(7)
    heads = {'cls': H.ClsHead(E, prior_prob=0.01), 'reg': H.RegHead(E, 3)}
    for name, head in heads.items():
        out = files[name]
        with torch.no_grad():
            for k, p in head.named_parameters():             # away from the constant initialisations
                if k.startswith('norms.'):
                    p.add_(0.2 * t(*p.shape) if k.endswith('weight') else 0.1 * t(*p.shape))
                if k.startswith('scales.'):
                    p.fill_({'0': 1.0, '1': 0.7, '2': 1.3}[k.split('.')[1]])
                if k.endswith('conv.bias'):
                    p.add_(0.05 * t(*p.shape))
        ups = [(t(B, T) if name == 'cls' else t(B, T, 2)) * (m if name == 'cls' else m[..., None]) for (T, _), m in zip(LEVELS, masks)]
        for k, p in head.state_dict().items():
            out[f'{name}/param/{k}'] = p.clone()
        for i, u in enumerate(ups):
            out[f'{name}/up/l{i}'] = u
        for tag, dt in (('32', torch.float32), ('64', torch.float64)):
            hd = H.ClsHead(E, prior_prob=0.01) if name == 'cls' else H.RegHead(E, 3)
            hd.load_state_dict(head.state_dict())
            hd = hd.to(dt)
            xin = [x.detach().to(dt).clone().requires_grad_(True) for x in xs]
            outs, _ = hd(xin, [m[:, None] for m in masks])
            sum((o * u.to(dt)).sum() for o, u in zip(outs, ups)).backward()
            for i, (o, xi) in enumerate(zip(outs, xin)):
                out[f'{name}/out{tag}/l{i}'] = o.detach()
                out[f'{name}/gx{tag}/l{i}'] = xi.grad
            for k, p in hd.named_parameters():
                if p.grad is not None:
                    out[f'{name}/gp{tag}/{k}'] = p.grad
    for name, fn in (('cls', 'head_grad.npz'), ('reg', 'head_grad_reg.npz')):
        path = os.path.join(HERE, fn)
        np.savez(path, **MG.npify(files[name]))
        print(fn, os.path.getsize(path), 'bytes')
        assert os.path.getsize(path) < (1 << 20)


if __name__ == '__main__':
    main()
