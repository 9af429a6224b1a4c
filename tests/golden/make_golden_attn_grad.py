"""Generate tests/golden/attn_grad.npz: forward values and `backward()` results of the reference's own MaskedMHA
(libs/modeling/blocks.py, embd_dim = 64, 4 heads, no dropout) with a local window, in fp32 and, from the same module cast to fp64,
in fp64.

Run where the reference is importable (not on the GPU machine):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_attn_grad.py

Cases: w9 = window 9 at (B 2, T 72), w19 = window 19 at (B 2, T 63) (the reference needs T % (window // 2) == 0).  Masks are prefix
masks: sequence 0 full, sequence 1 with a padded tail of about a third.  Each case is self attention on one input x (B, E, T) -- the
three projections still get gradients of their own, dQ / dK / dV of the core separately -- with a random upstream gradient that is
zero on padded positions; the scalar differentiated is sum(out * up).  The two cases share one set of parameters.  Per case: x, mask,
up, the fp32 / fp64 output and input gradient, and per parameter the fp32 / fp64 gradient."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402

E, HEADS, B = 64, 4, 2
CASES = {'w9': (9, 72, [72, 48]), 'w19': (19, 63, [63, 42])}


def reference_blocks():
    """libs/modeling/blocks.py alone, without the package's __init__ (which pulls in the whole model zoo)"""
    pkg = types.ModuleType('ref_modeling')
    pkg.__path__ = [os.path.join(os.environ.get('DCF_REFERENCE', MG.REF), 'libs', 'modeling')]
    sys.modules['ref_modeling'] = pkg
    return importlib.import_module('ref_modeling.blocks')


def main():
    BL = reference_blocks()
    rs = np.random.RandomState(20252)
    t = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32))
    torch.manual_seed(11)
    proto = BL.MaskedMHA(E, n_heads=HEADS, window_size=9, attn_pdrop=0.0, proj_pdrop=0.0)
    with torch.no_grad():
        for k, p in proto.named_parameters():                  # biases away from their small initialisation
            if k.endswith('bias'):
                p.add_(0.1 * t(*p.shape))
    out = {'meta': {'E': E, 'heads': HEADS, 'cases': {n: {'window': w, 'T': T, 'lens': lens} for n, (w, T, lens) in CASES.items()}}}
    for k, p in proto.state_dict().items():
        out[f'param/{k}'] = p.clone()
    for name, (window, T, lens) in CASES.items():
        x = t(B, E, T)
        mask = torch.arange(T)[None, :] < torch.tensor(lens)[:, None]
        up = t(B, E, T) * mask[:, None]
        out[f'{name}/x'], out[f'{name}/mask'], out[f'{name}/up'] = x, mask, up
        for tag, dt in (('32', torch.float32), ('64', torch.float64)):
            mha = BL.MaskedMHA(E, n_heads=HEADS, window_size=window, attn_pdrop=0.0, proj_pdrop=0.0)
            mha.load_state_dict(proto.state_dict())
            mha = mha.to(dt)
            xin = x.to(dt).clone().requires_grad_(True)
            y = mha(xin, xin, xin, mask[:, None])
            (y * up.to(dt)).sum().backward()
            out[f'{name}/out{tag}'] = y.detach()
            out[f'{name}/gx{tag}'] = xin.grad
            for k, p in mha.named_parameters():
                out[f'{name}/gp{tag}/{k}'] = p.grad
    path = os.path.join(HERE, 'attn_grad.npz')
    np.savez_compressed(path, **MG.npify(out))
    print('attn_grad.npz', os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < (1 << 20)


if __name__ == '__main__':
    main()
