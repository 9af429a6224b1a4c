"""Generate tests/golden/enc_grad.npz: forward values and `backward()` results of the reference's own TransformerEncoder
(libs/modeling/blocks.py; embd_dim = 32, 4 heads, window 9, every dropout probability 0) at stride 1 and stride 2, in fp32 and, from
the same module cast to fp64, in fp64; and of the reference's own masked_max_pool1d on a small hole mask with constructed ties.

Run where the reference is importable (not on the GPU machine):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_enc_grad.py

Cases s1 / s2 (stride 1 / 2): B 2, T 72, lengths [72, 47] (the reference needs (T / stride) % (window // 2) == 0).  The two cases share
one set of parameters: biases moved off zero by 0.1 N(0, 1), the LayerNorm weights moved by 0.1 N(0, 1), both LayerScales set to
0.5 + 0.25 N(0, 1) (at the initial 1e-4 the branches would not show in the gradient).  The upstream gradient is N(0, 1) on valid
output positions and zero on padded ones; the scalar differentiated is sum(out * up).  Per case: x, mask, up, the output mask, the
fp32 / fp64 output and input gradient, and the fp32 / fp64 gradient of each of the 27 parameters.

Case pool: masked_max_pool1d(x, mask, 3, 2) at B 2, C 4, T 12 with a hole mask, values drawn from {-2, ..., 2} so that equal values
meet inside windows, and in sequence 0 a padded slot in front of the row that holds the minimum of every channel; x, mask, up (on
every output position), the fp32 / fp64 output, pooled mask and input gradient.  It pins the detached fill value (blocks.py:38) and
the lowest-position tie rule."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402

E, HEADS, WINDOW, B, T, LENS = 32, 4, 9, 2, 72, [72, 47]
CASES = {'s1': 1, 's2': 2}


def reference_blocks():
    """libs/modeling/blocks.py alone, without the package's __init__ (which pulls in the whole model zoo)"""
    pkg = types.ModuleType('ref_modeling')
    pkg.__path__ = [os.path.join(os.environ.get('DCF_REFERENCE', MG.REF), 'libs', 'modeling')]
    sys.modules['ref_modeling'] = pkg
    return importlib.import_module('ref_modeling.blocks')


def main():
    BL = reference_blocks()
    rs = np.random.RandomState(20253)
    t = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32))
    torch.manual_seed(12)
    proto = BL.TransformerEncoder(E, 1, n_heads=HEADS, window_size=WINDOW, attn_pdrop=0.0, proj_pdrop=0.0, path_pdrop=0.0)
    with torch.no_grad():
        for k, p in proto.named_parameters():
            if k.endswith('drop_path_attn.scale') or k.endswith('drop_path_ffn.scale'):
                p.copy_(0.5 + 0.25 * t(*p.shape))
            elif k.endswith('bias'):
                p.add_(0.1 * t(*p.shape))
            elif 'norm' in k or k.startswith('ln_'):           # the LayerNorm weights
                p.add_(0.1 * t(*p.shape))
    assert len(list(proto.named_parameters())) == 27
    out = {'meta': {'E': E, 'heads': HEADS, 'window': WINDOW, 'B': B, 'T': T, 'lens': LENS, 'cases': CASES}}
    for k, p in proto.state_dict().items():
        out[f'param/{k}'] = p.clone()
    for name, stride in CASES.items():
        x = t(B, E, T)
        mask = torch.arange(T)[None, :] < torch.tensor(LENS)[:, None]
        up = t(B, E, T // stride) * mask[:, None, ::stride]
        out[f'{name}/x'], out[f'{name}/mask'], out[f'{name}/up'] = x, mask, up
        for tag, dt in (('32', torch.float32), ('64', torch.float64)):
            blk = BL.TransformerEncoder(E, stride, n_heads=HEADS, window_size=WINDOW, attn_pdrop=0.0, proj_pdrop=0.0, path_pdrop=0.0)
            blk.load_state_dict(proto.state_dict())
            blk = blk.to(dt).train()
            xin = x.to(dt).clone().requires_grad_(True)
            y, mo = blk(xin, mask[:, None])
            (y * up.to(dt)).sum().backward()
            assert torch.equal(mo[:, 0], mask[:, ::stride])
            out[f'{name}/mask_out'] = mo[:, 0]
            out[f'{name}/out{tag}'] = y.detach()
            out[f'{name}/gx{tag}'] = xin.grad
            n = 0
            for k, p in blk.named_parameters():
                out[f'{name}/gp{tag}/{k}'] = p.grad
                n += 1
            assert n == 27

    Bp, Cp, Tp = 2, 4, 12
    x = torch.from_numpy(rs.randint(-2, 3, size=(Bp, Cp, Tp)).astype(np.float32))
    mask = torch.ones(Bp, Tp, dtype=torch.bool)
    mask[0, [1, 2, 7]] = False
    mask[1, [0, 5, 6, 7, 10, 11]] = False                       # a whole padded window (o = 3: 5, 6, 7) and a padded tail
    x[0, :, 3] = -3.0                                           # the minimum of every channel of sequence 0, behind padded slots 1, 2
    up = t(Bp, Cp, Tp // 2)
    out['pool/x'], out['pool/mask'], out['pool/up'] = x, mask, up
    for tag, dt in (('32', torch.float32), ('64', torch.float64)):
        xin = x.to(dt).clone().requires_grad_(True)
        y, mo = BL.masked_max_pool1d(xin, mask[:, None], 3, 2)
        (y * up.to(dt)).sum().backward()
        out[f'pool/out{tag}'], out[f'pool/gx{tag}'], out['pool/mask_out'] = y.detach(), xin.grad, mo[:, 0]

    path = os.path.join(HERE, 'enc_grad.npz')
    np.savez_compressed(path, **MG.npify(out))
    print('enc_grad.npz', os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < (1 << 20)


if __name__ == '__main__':
    main()
