"""Generate tests/golden/backbone_grad_*.npz: forward values and `backward()` results of the reference's own VideoTransformer
(libs/modeling/video_net.py) and TextTransformer (libs/modeling/text_net.py) in training mode with every dropout probability 0, in
fp32 and, from the same modules cast to fp64, in fp64.

Run where the reference is importable (not on the GPU machine):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_backbone_grad.py

Video cases: in_dim = embd_dim = 32 (the smallest width the operators admit), 4 heads, window 3, `use_abs_pe` on, two videos, the second
with a padded tail of odd length; every arch keeps two embedding convolutions
    s4    stride 4, arch (2, 1, 3): both convolutions k5 / stride 2; T = 48, lengths [48, 29] -> pyramid 12, 6, 3
    s2    stride 2, arch (2, 1, 3): one k5 / stride 2 convolution, then one k3; T = 24, lengths [24, 15] -> pyramid 12, 6, 3
    pool  stride 1, arch (2, 1, 3), `pool_only`: the branch is three depthwise convolutions; T = 12, lengths [12, 7] -> 12, 6, 3
Text case `text`: in_dim = embd_dim = 32, 2 heads (head dimension 16), two layers, background token and position encoding on, three
queries of lengths [9, 5, 7] padded to 9.

Parameters: biases and LayerNorm weights moved off their initial values by 0.1 N(0, 1), the LayerScales set to 0.5 + 0.25 N(0, 1) (at
the initial 1e-4 the branches would not show in the gradient); inputs and parameters rounded to multiples of 2^-10.  The upstream
gradient is N(0, 1) (on the same grid) on EVERY output row of every level; the scalar differentiated is sum_l sum(fpn[l] * up[l]).

Files per case (each below the 1 MiB limit of a committed file):
    backbone_grad_<case>.npz          meta, param/<name>, x, mask, up<l>, mask_out<l>, out32_<l> / out64_<l>, gx32 / gx64
    backbone_grad_<case>_gp32.npz / _gp64.npz    <name> -> the gradient of that parameter (key.bias of the stride-0 blocks like any other)
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402

LIMIT = 1 << 20
VIDEO = dict(in_dim=32, embd_dim=32, max_seq_len=12, n_heads=4, mha_win_size=3, use_abs_pe=True)
CASES = {
    's4': (dict(VIDEO, stride=4, arch=[2, 1, 3], pool_only=False), 48, [48, 29]),
    's2': (dict(VIDEO, stride=2, arch=[2, 1, 3], pool_only=False), 24, [24, 15]),
    'pool': (dict(VIDEO, stride=1, arch=[2, 1, 3], pool_only=True), 12, [12, 7]),
    'text': (dict(in_dim=32, embd_dim=32, n_heads=2, max_seq_len=9, n_layers=2, use_abs_pe=True, use_bkgd_token=True), 9, [9, 5, 7]),
}
DROP = dict(attn_pdrop=0.0, proj_pdrop=0.0, path_pdrop=0.0)


def reference_modules():
    """libs/modeling/video_net.py and text_net.py alone, without the package's __init__ (which pulls in the whole model zoo)"""
    pkg = types.ModuleType('ref_modeling')
    pkg.__path__ = [os.path.join(os.environ.get('DCF_REFERENCE', MG.REF), 'libs', 'modeling')]
    sys.modules['ref_modeling'] = pkg
    return importlib.import_module('ref_modeling.video_net'), importlib.import_module('ref_modeling.text_net')


def coarse(x):
    return torch.round(x * 1024) / 1024


def save(name, d):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **MG.npify(d))
    print(name, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < LIMIT, name


def main():
    VN, TN = reference_modules()
    rs = np.random.RandomState(20255)
    t = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32))
    torch.manual_seed(14)
    for name, (kw, T, lens) in CASES.items():
        text = name == 'text'
        make = (lambda: TN.TextTransformer(**kw, **DROP)) if text else (lambda: VN.VideoTransformer(**kw, **DROP))
        proto = make()
        with torch.no_grad():
            for k, p in proto.named_parameters():
                if k.endswith('drop_path_attn.scale') or k.endswith('drop_path_ffn.scale'):
                    p.copy_(0.5 + 0.25 * t(*p.shape))
                elif k.endswith('bias') or 'norm' in k or '.ln_' in k:                 # biases and the LayerNorm weights
                    p.add_(0.1 * t(*p.shape))
                p.copy_(coarse(p))
        names = [k for k, _ in proto.named_parameters()]
        x = coarse(t(len(lens), kw['in_dim'], T))
        mask = torch.arange(T)[None, :] < torch.tensor(lens)[:, None]
        core = {'x': x, 'mask': mask}
        for k, p in proto.state_dict().items():
            core[f'param/{k}'] = p.clone()
        ups = None
        for tag, dt in (('32', torch.float32), ('64', torch.float64)):
            net = make()
            net.load_state_dict(proto.state_dict())
            net = net.to(dt).train()
            xin = x.to(dt).clone().requires_grad_(True)
            ys, ms = net(xin, mask)
            if text:
                ys, ms = (ys,), (ms,)
            if ups is None:
                ups = [coarse(t(*y.shape)) for y in ys]                                # non-zero on padded rows too
            sum((y * u.to(dt)).sum() for y, u in zip(ys, ups)).backward()
            for l, (y, m) in enumerate(zip(ys, ms)):
                core[f'out{tag}_{l}'], core[f'mask_out{l}'], core[f'up{l}'] = y.detach(), m[:, 0], ups[l]
            core[f'gx{tag}'] = xin.grad
            grads = {k: p.grad for k, p in net.named_parameters()}
            assert all(g is not None for g in grads.values()) and list(grads) == names
            save(f'backbone_grad_{name}_gp{tag}.npz', grads)
        core['meta'] = {'kw': kw, 'T': T, 'lens': lens, 'n_levels': len(ups), 'n_params': len(names),
                        'level_lengths': [int(u.size(-1)) for u in ups]}
        save(f'backbone_grad_{name}.npz', core)


if __name__ == '__main__':
    main()
