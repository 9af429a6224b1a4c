"""Generate tests/golden/train_dropout.npz: the reference's train()-mode forward with dropout and drop-path on, its random
draws replaced by the project's stated stream (tests/philox_ref.py, include/decafnet_hip.h dcf_model_set_dropout).

Run where the reference is importable (not on the GPU machine):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dropout.py

PtTransformerEarlyFusionIterative(second_fusion=False).train() with proj_pdrop 0.2 and path_pdrop 0.3 (vid_net and fusion)
and the refinement TCN's Dropout at 0.5.  Every nn.Dropout.forward and every LayerScale's drop_path draw from the restated
stream by the site of the module that calls them.  Two cases: the train.npz shape (E = 64, T = 256) and E = 256, T = 1024.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402
import philox_ref as P  # noqa: E402

PROJ, PATH, TCN = 0.2, 0.3, 0.5
PREFIX = 4096            # keep bits stored per site (packed); the counts cover the whole site


def site_of(name):
    """module name in the reference model -> (group, layer, kind)"""
    parts = name.split('.')
    if parts[0] == 'fusion' and parts[1] == 'layers':
        g, i, rest = P.G_FUSION, int(parts[2]), parts[3:]
    elif parts[0] == 'vid_net' and parts[1] in ('stem', 'branch'):
        g, i, rest = (P.G_STEM if parts[1] == 'stem' else P.G_BRANCH), int(parts[2]), parts[3:]
    elif parts[0] == 'refine' and parts[1] == 'layers':
        g, i, rest = P.G_REFINE, int(parts[2]), parts[3:]
    else:
        return None
    return g, i, '.'.join(rest)


class Stream:
    def __init__(self, seed):
        self.seed = seed
        self.log = {}            # site -> (shape, keep bits) as drawn
        self.ffn_calls = {}

    def dropout(self, mod, x):
        if not mod.training or mod.p == 0.0:
            return x
        g, i, rest = mod._dcf_site
        if rest in ('attn.attn.proj_drop', 'xattn.xattn.proj_drop'):
            sub = P.PROJ
        elif rest == 'ffn.dropout':          # FFN.dropout is called twice per forward: after the GELU, then after proj
            k = self.ffn_calls.get((g, i), 0)
            self.ffn_calls[(g, i)] = k + 1
            sub = P.FFN_HID if k % 2 == 0 else P.FFN_OUT
        elif rest == 'dropout' and g == P.G_REFINE:
            sub = P.TCN
        else:
            raise AssertionError(f'unexpected dropout site {mod._dcf_site}')
        s = P.site(g, i, sub)
        assert x.ndim == 3 and x.is_contiguous(), (s, x.shape)
        keep = P.dropout_mask(self.seed, s, tuple(x.shape), mod.p)
        assert s not in self.log, s
        self.log[s] = (tuple(x.shape), keep)
        return x * (torch.from_numpy(keep).to(x.dtype) * float(P.scale(mod.p)))

    def drop_path(self, mod, x):
        if not mod.training or mod.pdrop == 0.0:
            return mod.scale.to(x.dtype) * x
        g, i, rest = mod._dcf_site
        s = P.site(g, i, P.PATH_ATTN if rest == 'drop_path_attn' else P.PATH_FFN)
        x = mod.scale.to(x.dtype) * x
        keep = P.drop_path_keep(self.seed, s, x.shape[0], mod.pdrop)
        assert s not in self.log, s
        self.log[s] = ((x.shape[0],), keep)
        shape = (x.shape[0],) + (1,) * (x.ndim - 1)
        return x.div(1 - mod.pdrop) * torch.from_numpy(keep).to(x.dtype).reshape(shape)     # blocks.py:685-694


def run_case(kw, wseed, iseed, seed, bs, T, lq, sizes, lens, tok_len):
    from libs.modeling import blocks
    from libs.modeling.model import PtTransformerEarlyFusionIterative
    opt = MG.make_opt(**kw)
    for part in ('vid_net', 'fusion'):
        opt.model[part]['proj_pdrop'] = PROJ
        opt.model[part]['path_pdrop'] = PATH
    model = PtTransformerEarlyFusionIterative(opt.clone(), second_fusion=False).train()
    shapes = {k: list(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(MG.synth.make_state_dict(shapes, wseed))
    for mod in model.refine.modules():
        if isinstance(mod, torch.nn.Dropout):
            assert mod.p == 0.5
            mod.p = TCN
    stream = Stream(seed)
    for name, mod in model.named_modules():
        if isinstance(mod, (torch.nn.Dropout, blocks.LayerScale)):
            mod._dcf_site = site_of(name)
            if isinstance(mod, torch.nn.Dropout) and mod.p > 0:
                assert mod._dcf_site is not None, name
    orig_do, orig_ls = torch.nn.Dropout.forward, blocks.LayerScale.forward
    torch.nn.Dropout.forward = lambda mod, x: stream.dropout(mod, x) if getattr(mod, '_dcf_site', None) else orig_do(mod, x)
    blocks.LayerScale.forward = lambda mod, x: stream.drop_path(mod, x)
    try:
        g = torch.Generator().manual_seed(iseed)
        D = kw['D']
        vid = torch.randn(bs, D, T, generator=g)
        shallow = torch.randn(bs, D, T, generator=g)
        vid_masks = torch.stack([torch.arange(T) < n for n in lens])
        vid, shallow = vid * vid_masks[:, None], shallow * vid_masks[:, None]
        tokens = torch.randn(sum(sizes), kw['text_in'], lq, generator=g)
        token_masks = torch.stack([torch.arange(lq) < n for n in tok_len])[:, None]
        tokens = tokens * token_masks
        text_cls = torch.randn(sum(sizes), D, generator=g)
        # the padded per-video layout of the training collate (model.py:617-622): (bs, max_k, C, Lq) / (bs, max_k, Lq)
        mk = max(sizes)
        text_pad = torch.zeros(bs, mk, kw['text_in'], lq)
        mask_pad = torch.zeros(bs, mk, lq, dtype=torch.bool)
        q = 0
        for b, k in enumerate(sizes):
            text_pad[b, :k], mask_pad[b, :k] = tokens[q:q + k], token_masks[q:q + k, 0]
            q += k
        with torch.no_grad():
            out4 = model(vid, shallow, vid_masks, text_pad, text_cls, mask_pad, text_size=torch.tensor(sizes), eval=False)
    finally:
        torch.nn.Dropout.forward, blocks.LayerScale.forward = orig_do, orig_ls
    out = dict(opt_kwargs=kw, meta=dict(bs=bs, T=T, lq=lq, sizes=sizes, wseed=wseed, seed=seed, proj_pdrop=PROJ, path_pdrop=PATH,
                                        refine_pdrop=TCN),
               shapes=shapes, vid=vid, shallow=shallow, vid_masks=vid_masks, tokens=tokens, token_masks=token_masks, text_cls=text_cls)
    for part, name in zip(out4, ('logits1', 'logits2', 'offsets', 'masks')):
        for l, x in enumerate(part):
            out[f'{name}/l{l}'] = x
    sites = sorted(stream.log)
    out['sites'] = [dict(site=s, shape=list(stream.log[s][0]), kept=int(stream.log[s][1].sum())) for s in sites]
    for s in sites:
        out[f'keep/{s}'] = np.packbits(stream.log[s][1].reshape(-1)[:PREFIX])
    paths = [stream.log[s][1] for s in sites if s & 15 in (P.PATH_ATTN, P.PATH_FFN)]
    out['path_fired'] = int(sum(int((~k).sum()) for k in paths))
    out['path_kept'] = int(sum(int(k.sum()) for k in paths))
    return out


def pick_seed(start, n_rows, path_sites):
    """the first seed from `start` on under which at least one drop-path fires and at least one keeps its sample"""
    seed = start
    while True:
        k = np.concatenate([P.drop_path_keep(seed, s, n_rows, PATH) for s in path_sites])
        if k.any() and not k.all():
            return seed
        seed += 1


def main():
    MG.install_stubs()
    cases = {
        'e64': dict(kw=dict(D=64, E=64, TE=32, text_in=32, n_levels=4, win=5, n_heads=4, sn=8, sratio=0.3, msf=True, norm=True,
                            max_seq_len=256, text_layers=2, text_max_len=24),
                    wseed=901, iseed=902, bs=2, T=256, lq=7, sizes=[2, 1], lens=[256, 201], tok_len=[7, 5, 6]),
        'e256': dict(kw=dict(D=32, E=256, TE=64, text_in=32, n_levels=6, win=5, n_heads=4, sn=16, sratio=0.3, msf=True, norm=True,
                             max_seq_len=1024, text_layers=1, text_max_len=24, n_stem=1),
                     wseed=941, iseed=942, bs=2, T=1024, lq=6, sizes=[1, 2], lens=[1000, 1024], tok_len=[6, 4, 5]),
    }
    out = {}
    for name, c in cases.items():
        L = c['kw']['n_levels']
        path_sites = [P.site(g, i, sub) for g, n in ((P.G_FUSION, 2), (P.G_STEM, c['kw'].get('n_stem', 0)), (P.G_BRANCH, L))
                      for i in range(n) for sub in (P.PATH_ATTN, P.PATH_FFN)]
        seed = pick_seed(0x9E3779B97F4A7C15, sum(c['sizes']), path_sites)
        res = run_case(c['kw'], c['wseed'], c['iseed'], seed, c['bs'], c['T'], c['lq'], c['sizes'], c['lens'], c['tok_len'])
        assert res['path_fired'] > 0 and res['path_kept'] > 0
        for k, v in res.items():
            out[f'{name}/{k}'] = v
    out['cases'] = list(cases)
    MG.save('train_dropout.npz', out)


if __name__ == '__main__':
    main()
