"""Generate tests/golden/dec_grad*.npz: forward values and `backward()` results of the reference's own XAttNFusion
(libs/modeling/fusion.py, blocks.py; vid_dim 64, text_dim 96, 4 heads, 2 layers, every dropout probability 0) and of one of its
TransformerDecoder layers, in fp32 and, from the same modules cast to fp64, in fp64.

Run where the reference is importable (not on the GPU machine):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dec_grad.py

Cases
    adaln   2 videos, T = 40, lengths [40, 27] (a padded tail on the second), kv_size = [2, 1]: 3 text queries of lengths [9, 5, 7]
            padded to 9; xattn_mode 'adaln'
    affine  the same inputs and parameters with xattn_mode 'affine'
    single  layer 0 alone (a TransformerDecoder, 'adaln') with kv_size = None: the 2 videos against the first 2 texts

All cases share one set of parameters: biases moved off zero by 0.1 N(0, 1), the LayerNorm weights moved by 0.1 N(0, 1), the LayerScales
set to 0.5 + 0.25 N(0, 1) (at the initial 1e-4 the FFN branch would not show in the gradient).  The upstream gradient is N(0, 1) on EVERY
output row, padded video rows included (the decoder does not mask its output); the scalar differentiated is sum(out * up).

Files (each below the 1 MiB limit of a committed file; the 116 800 parameters of the stack make 1.4 MB of gradients per two-layer case
in the two precisions, so the parameter gradients live in a file per case and precision):
    dec_grad.npz                     meta, param/<name>, and per case <case>/vid, vid_mask, text, text_mask, up, kv_size,
                                     out32 / out64, mask_out, gvid32 / gvid64, gtext32 / gtext64
    dec_grad_<case>_gp32.npz / _gp64.npz    <name> -> the gradient of that parameter (for `single`, names below layers.0)
Parameters and inputs are rounded to multiples of 2^-10 so that dec_grad.npz compresses; nothing else is rounded."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402

VID_DIM, TEXT_DIM, HEADS, LAYERS, T, LK = 64, 96, 4, 2, 40, 9
VID_LENS, KV_SIZE, TEXT_LENS = [40, 27], [2, 1], [9, 5, 7]
LIMIT = 1 << 20


def reference_modules():
    """libs/modeling/blocks.py and fusion.py alone, without the package's __init__ (which pulls in the whole model zoo)"""
    pkg = types.ModuleType('ref_modeling')
    pkg.__path__ = [os.path.join(os.environ.get('DCF_REFERENCE', MG.REF), 'libs', 'modeling')]
    sys.modules['ref_modeling'] = pkg
    return importlib.import_module('ref_modeling.blocks'), importlib.import_module('ref_modeling.fusion')


def coarse(x):
    return torch.round(x * 1024) / 1024


def save(name, d):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **MG.npify(d))
    print(name, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < LIMIT, name


def main():
    BL, FU = reference_modules()
    rs = np.random.RandomState(20254)
    t = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32))
    torch.manual_seed(13)
    kw = dict(n_layers=LAYERS, n_heads=HEADS, attn_pdrop=0.0, proj_pdrop=0.0, path_pdrop=0.0)
    proto = FU.XAttNFusion(VID_DIM, TEXT_DIM, xattn_mode='adaln', **kw)
    with torch.no_grad():
        for k, p in proto.named_parameters():
            if k.endswith('drop_path_ffn.scale'):
                p.copy_(0.5 + 0.25 * t(*p.shape))
            elif k.endswith('bias') or 'norm' in k or '.ln_' in k or k.startswith('ln_'):     # biases and the LayerNorm weights
                p.add_(0.1 * t(*p.shape))
            p.copy_(coarse(p))
    names = [k for k, _ in proto.named_parameters()]
    layer0 = [k[len('layers.0.'):] for k in names if k.startswith('layers.0.')]
    core = {'meta': {'vid_dim': VID_DIM, 'text_dim': TEXT_DIM, 'heads': HEADS, 'layers': LAYERS, 'T': T, 'Lk': LK, 'vid_lens': VID_LENS,
                     'kv_size': KV_SIZE, 'text_lens': TEXT_LENS, 'cases': {'adaln': 'adaln', 'affine': 'affine', 'single': 'adaln'},
                     'n_params': len(names), 'n_layer_params': len(layer0)}}
    for k, p in proto.state_dict().items():
        core[f'param/{k}'] = p.clone()

    vid = coarse(t(len(VID_LENS), VID_DIM, T))
    vid_mask = torch.arange(T)[None, :] < torch.tensor(VID_LENS)[:, None]
    text = coarse(t(len(TEXT_LENS), TEXT_DIM, LK))
    text_mask = torch.arange(LK)[None, :] < torch.tensor(TEXT_LENS)[:, None]
    for name, mode in core['meta']['cases'].items():
        single = name == 'single'
        nq = len(VID_LENS) if single else len(TEXT_LENS)
        tx, tm = text[:nq], text_mask[:nq]
        kv_size = None if single else torch.tensor(KV_SIZE)
        up = coarse(t(nq, VID_DIM, T))                             # non-zero on padded video rows too
        core[f'{name}/vid'], core[f'{name}/vid_mask'], core[f'{name}/text'], core[f'{name}/text_mask'] = vid, vid_mask, tx, tm
        core[f'{name}/up'] = up
        core[f'{name}/kv_size'] = torch.tensor(KV_SIZE if not single else [1] * nq)
        for tag, dt in (('32', torch.float32), ('64', torch.float64)):
            net = FU.XAttNFusion(VID_DIM, TEXT_DIM, xattn_mode=mode, **kw)
            net.load_state_dict(proto.state_dict())
            net = net.to(dt).train()
            mod = net.layers[0] if single else net
            vin, tin = vid.to(dt).clone().requires_grad_(True), tx.to(dt).clone().requires_grad_(True)
            y, mo = mod(vin, vid_mask[:, None], tin, tm[:, None], kv_size)
            (y * up.to(dt)).sum().backward()
            assert y.shape == (nq, VID_DIM, T)
            core[f'{name}/out{tag}'], core[f'{name}/mask_out'] = y.detach(), mo[:, 0]
            core[f'{name}/gvid{tag}'], core[f'{name}/gtext{tag}'] = vin.grad, tin.grad
            grads = {k: p.grad for k, p in mod.named_parameters()}
            assert all(g is not None for g in grads.values()) and len(grads) == (len(layer0) if single else len(names))
            save(f'dec_grad_{name}_gp{tag}.npz', grads)
    save('dec_grad.npz', core)


if __name__ == '__main__':
    main()
