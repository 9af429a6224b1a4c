"""Generate tests/golden/step_grad_drop_<case>*.npz: make_golden_step_grad.py's whole training step of the reference -- forward in
.train(), the Trainer's objective, `total.backward()`, in fp32 and from the same model cast to fp64 -- with dropout and drop-path ON and
every random draw replaced by the project's stated stream (make_golden_dropout.py's `Stream` on tests/philox_ref.py): every
nn.Dropout.forward and LayerScale.forward of the model draws its keep bits by the site of the module that calls it, the same bits in
both precisions.

Run where the reference is importable (not on the GPU machine):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_step_grad_drop.py

proj_pdrop = 0.2 and path_pdrop = 0.3 (vid_net and fusion), the refinement TCN's Dropout at its hard-wired 0.5, channel_drop 0,
second_fusion=False (the only configuration with a dropout forward).  Cases, otherwise those of make_golden_step_grad.py:
    s1d   `s1`: stride 1, no msf, T = 40, lengths 40 / 27; levels 40 / 20 / 10, so the last has T % 4 != 0
    s2d   `s2` without its second fusion: stride 2, msf, T = 80
Files and keys are those of make_golden_step_grad.py (tests/step_grad_ref.py reads them as case `drop_<case>`); meta adds `seed`,
the rates and `sites` (site, shape, kept count per site as drawn).

Conditions on the reference alone, asserted here and again on the committed files by tests/test_step_grad_drop_cpu.py: all of
make_golden_step_grad.py's (gate, masks and labels agree between the precisions; no positive point is non-smooth; e_ref <= 2^-15 max
|g_64| for every parameter but the zero-by-symmetry pair; every parameter takes a non-zero gradient), and the key is picked by search
so that no drop-path site drops all three rows, at least one drops a row and at least one keeps all three.  If a seed trips a
condition, change the seed, not the condition."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402
import make_golden_dropout as MD  # noqa: E402
import make_golden_step_grad as SG  # noqa: E402
import objective_cases as C  # noqa: E402
import objective_grad_ref as OR  # noqa: E402
import philox_ref as P  # noqa: E402

PROJ, PATH, TCN = 0.2, 0.3, 0.5
CASES = {
    's1d': dict(SG.CASES['s1'], key0=0x9E3779B97F4A7C15),
    's2d': dict(SG.CASES['s2'], second_fusion=False, key0=0xD1B54A32D192ED03),
}


# blocks recorded on their own in the s1d file (group blk/<tag>/): input, mask, output, the gradients at both, in fp32 and fp64; each is
# used once in the step, so its parameter gradients are the step's.  enc1: stride 1, T = 40; enc2: stride 2, T = 40 -> 20; dec: the second
# decoder layer (three rows in and out), T = 40
BLOCKS = {'enc1': 'vid_net.stem.0', 'enc2': 'vid_net.branch.1', 'dec': 'fusion.layers.1'}


def path_condition(keeps):
    """keeps: the per-sample keep bits of every drop-path site"""
    return all(k.any() for k in keeps) and any(not k.all() for k in keeps) and any(k.all() for k in keeps)


def main():
    MG.install_stubs()
    from libs.modeling import blocks
    from libs.modeling.model import PtGenerator, PtTransformerEarlyFusionIterative
    from libs.worker_v2 import annotate_points_per_video, calc_focal_loss, calc_iou_loss

    def trainer_total(l1, l2, off, msk, labels, gt_off, reg_loss):
        pos = torch.logical_and(labels, msk)
        cls1 = calc_focal_loss(logits=l1[msk], labels=labels[msk], alpha=C.FC_A, smoothing=C.FC_S) / SG.LOSS_NORM * SG.WORLD_SIZE
        cls2 = calc_focal_loss(logits=l2[msk], labels=labels[msk], alpha=C.FC_A, smoothing=C.FC_S) / SG.LOSS_NORM * SG.WORLD_SIZE
        reg = calc_iou_loss(pred_offsets=off[pos], gt_offsets=gt_off[pos], reg_loss=reg_loss) / SG.LOSS_NORM * SG.WORLD_SIZE
        return (cls1 + cls2) / 2 + SG.LOSS_WEIGHT * reg

    t_coarse = SG.coarse
    for name, c in CASES.items():
        rs = np.random.RandomState(c['seed'])
        t = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32))
        torch.manual_seed(c['seed'])
        kw, T, D = c['opt'], c['T'], c['opt']['D']
        L, stride = kw['n_levels'], kw['vid_stride']
        TOK_LENS, TEXT_SIZE = SG.TOK_LENS, SG.TEXT_SIZE

        def make():
            opt = MG.make_opt(**kw)
            for part in ('vid_net', 'fusion'):
                opt.model[part]['proj_pdrop'] = PROJ
                opt.model[part]['path_pdrop'] = PATH
            net = PtTransformerEarlyFusionIterative(opt.clone(), second_fusion=False)
            for mod in net.modules():
                if isinstance(mod, torch.nn.Dropout1d):                                  # channel_drop
                    mod.p = 0.0
            for mod in net.refine.modules():
                if isinstance(mod, torch.nn.Dropout):
                    assert mod.p == TCN
            for mname, mod in net.named_modules():
                if isinstance(mod, (torch.nn.Dropout, blocks.LayerScale)):
                    mod._dcf_site = MD.site_of(mname)
                    assert mod._dcf_site is not None or not (isinstance(mod, torch.nn.Dropout) and mod.p > 0), mname
            return net

        proto = make()
        SG.perturb(proto, t)
        names = [k for k, _ in proto.named_parameters()]
        bs, nq, lq = len(c['lens']), sum(TEXT_SIZE), max(TOK_LENS)
        vid_masks = torch.arange(T)[None, :] < torch.tensor(c['lens'])[:, None]
        vid, shallow = t_coarse(t(bs, D, T)) * vid_masks[:, None], t_coarse(t(bs, D, T)) * vid_masks[:, None]
        token_masks = (torch.arange(lq)[None, :] < torch.tensor(TOK_LENS)[:, None])[:, None]
        tokens = t_coarse(t(nq, kw['text_in'], lq)) * token_masks
        text_cls = t_coarse(t(nq, D))
        text_pad = torch.zeros(bs, max(TEXT_SIZE), kw['text_in'], lq)
        mask_pad = torch.zeros(bs, max(TEXT_SIZE), lq, dtype=torch.bool)
        q = 0
        for b, k in enumerate(TEXT_SIZE):
            text_pad[b, :k], mask_pad[b, :k] = tokens[q:q + k], token_masks[q:q + k, 0]
            q += k
        targets = torch.tensor(c['targets'])
        sizes = [(T // stride) >> l for l in range(L)]
        points = torch.cat(PtGenerator(kw['max_seq_len'], L, 4, 0.5, use_offset=False)(sizes))
        ann = [annotate_points_per_video(points, tg, center_sampling=c['center_sampling'], center_sampling_radius=C.RADIUS) for tg in targets]
        labels, gt_off = torch.stack([a[0] for a in ann]), torch.stack([a[1] for a in ann])

        core = {'opt_kwargs': kw, 'vid': vid, 'shallow': shallow, 'vid_masks': vid_masks, 'tokens': tokens, 'token_masks': token_masks,
                'text_cls': text_cls, 'targets': targets, 'labels': labels, 'gt_offsets': gt_off}
        for k, p in proto.state_dict().items():
            core[f'param/{k}'] = p.clone()

        def run(dt, reference_loss, key):
            net = make()
            net.load_state_dict(proto.state_dict())
            net = net.to(dt).train()
            tap = {}
            net.vid_map.register_forward_pre_hook(lambda m, a: tap.update(vid_map_in=a[0].detach(), mask_gated=a[1][:, 0]))
            net.vid_map.register_forward_hook(lambda m, a, o: tap.update(vid_map=o[0]))

            def keep(tag):
                def hook(m, a, o):
                    o[0].retain_grad()
                    tap[tag] = o[0]
                return hook

            net.text_net.register_forward_hook(keep('text'))
            net.fusion.register_forward_hook(keep('fused'))
            net.vid_net.register_forward_hook(lambda m, a, o: tap.update(fpn=o[0]))
            blk = {}

            def block_hooks(tag):
                def pre(m, a):
                    x = a[0].clone()                               # the block's own input gradient: a pyramid level also feeds the heads
                    x.retain_grad()
                    blk[tag] = {'x': x, 'mask': a[1]}
                    if tag == 'dec':
                        assert a[0].size(0) == a[2].size(0) == nq
                        blk[tag].update(kv=a[2].detach(), kv_mask=a[3])
                    return (x,) + tuple(a[1:])

                def post(m, a, o):
                    o[0].retain_grad()
                    blk[tag].update(y=o[0], mask_out=o[1])
                return pre, post

            for tag, mname in BLOCKS.items():
                pre, post = block_hooks(tag)
                net.get_submodule(mname).register_forward_pre_hook(pre)
                net.get_submodule(mname).register_forward_hook(post)
            stream = MD.Stream(key)
            orig_do, orig_ls = torch.nn.Dropout.forward, blocks.LayerScale.forward
            torch.nn.Dropout.forward = lambda mod, x: stream.dropout(mod, x) if getattr(mod, '_dcf_site', None) else orig_do(mod, x)
            blocks.LayerScale.forward = lambda mod, x: stream.drop_path(mod, x)
            try:
                l1, l2, off, mo = net(vid.to(dt), shallow.to(dt), vid_masks, text_pad.to(dt), text_cls.to(dt), mask_pad, text_size=torch.tensor(TEXT_SIZE))
            finally:
                torch.nn.Dropout.forward, blocks.LayerScale.forward = orig_do, orig_ls
            msk = torch.cat(mo, 1).reshape(nq, -1)
            cl1, cl2, coff = torch.cat(l1, 1), torch.cat(l2, 1), torch.cat(off, 1)
            if reference_loss:
                total = trainer_total(cl1, cl2, coff, msk, labels, gt_off.to(dt), c['reg_loss'])
            else:
                total = OR.objective_value(cl1, cl2, coff, msk, labels, gt_off.to(dt), c['reg_loss'], SG.LOSS_NORM, SG.WORLD_SIZE, SG.LOSS_WEIGHT,
                                           C.FC_A, C.FC_S, dt)
            total.backward()
            x_in = tap['vid_map_in']
            rep = vid.repeat_interleave(torch.tensor(TEXT_SIZE), dim=0).to(dt)
            gate = (x_in[:, :D] != 0).any(1)
            assert torch.equal(x_in[:, :D], rep * gate[:, None].to(dt)), 'the gate could not be read off the input of vid_map'
            grads = {k: p.grad for k, p in net.named_parameters()}
            assert list(grads) == names and all(g is not None for g in grads.values()), [k for k, g in grads.items() if g is None]
            return dict(l1=l1, l2=l2, off=off, masks=[m.reshape(nq, -1) for m in mo], total=total.detach(), gate=gate,
                        mask_gated=tap['mask_gated'], msk=msk, coff=coff.detach(), grads=grads, log=stream.log,
                        blocks={tag: dict(x=b['x'].detach(), gx=b['x'].grad, y=b['y'].detach(), gy=b['y'].grad, mask=b['mask'], mask_out=b['mask_out'],
                                          **({'kv': b['kv'], 'kv_mask': b['kv_mask']} if tag == 'dec' else {})) for tag, b in blk.items()},
                        taps={'vid_map': tap['vid_map'].detach(), 'text': tap['text'].detach(), 'fused': tap['fused'].detach(),
                              **{f'fpn{l}': x.detach() for l, x in enumerate(tap['fpn'])}},
                        gtaps={'text': tap['text'].grad, 'fused': tap['fused'].grad})

        # the sites do not depend on the key: a first run lists them (and warms the scripted loss functions up), then the key is searched
        probe = run(torch.float32, True, c['key0'])
        path_sites = sorted(s for s in probe['log'] if s & 15 in (P.PATH_ATTN, P.PATH_FFN))
        assert len(path_sites) >= 3 and all(probe['log'][s][0] == (nq,) for s in path_sites)
        key = c['key0']
        while not path_condition([P.drop_path_keep(key, s, nq, PATH) for s in path_sites]):
            key += 1
        print(f'{name}: key {key:#x} ({key - c["key0"]} past the start), {len(probe["log"])} sites, {len(path_sites)} of them drop-path')
        for _ in range(SG.WARMUP):
            run(torch.float32, True, key)
        r32, again = run(torch.float32, True, key), run(torch.float32, True, key)
        assert all(torch.equal(r32['grads'][k], again['grads'][k]) for k in names), 'the fp32 gradient changed between calls'
        r64 = run(torch.float64, False, key)
        assert sorted(r32['log']) == sorted(r64['log']) and all(np.array_equal(r32['log'][s][1], r64['log'][s][1]) for s in r32['log'])
        print(f'{name}: total {float(r64["total"]):.9f} (fp32 {float(r32["total"]):.9f})')

        # ---- conditions on the reference alone
        assert path_condition([r32['log'][s][1] for s in path_sites])
        assert torch.equal(r32['gate'], r64['gate']) and torch.equal(r32['mask_gated'], r64['mask_gated']), 'gate decisions differ'
        assert all(torch.equal(a, b) for a, b in zip(r32['masks'], r64['masks']))
        pos = labels & r32['msk']
        lv = np.cumsum([0] + sizes)
        per_level = [int(pos[:, lv[l]:lv[l + 1]].sum()) for l in range(L)]
        n_ex = sum(int((OR.non_smooth(r['coff'], gt_off) & pos).sum()) for r in (r32, r64))
        assert min(per_level) >= 1 and n_ex == 0, (per_level, n_ex)
        rows, worst = [], (0.0, None)
        for k in names:
            g32, g64 = r32['grads'][k].double(), r64['grads'][k]
            top, e = float(g64.abs().max()), float((g32 - g64).abs().max())
            zero = k.endswith(SG.ZERO_BY_SYMMETRY)
            if zero:
                top = float(r64['grads'][k[:-len('bias')] + 'weight'].abs().max())
            assert top > 0, k
            rel = e / top
            rows.append(rel)
            if not zero:
                assert float(g64.abs().max()) > 0 and rel <= SG.E_REF_CAP, (k, rel)
                worst = max(worst, (rel, k))
        print(f'{name}: {len(names)} parameters, worst e_ref / max|g64| {worst[0]:.3e} ({worst[1]}), median {float(np.median(rows)):.3e}')

        core['gate'], core['mask_gated'] = r32['gate'], r32['mask_gated']
        for l in range(L):
            core[f'mask/l{l}'] = r32['masks'][l]
        for tag, r in (('32', r32), ('64', r64)):
            for l in range(L):
                core[f'logits1_{tag}/l{l}'], core[f'logits2_{tag}/l{l}'], core[f'offsets_{tag}/l{l}'] = r['l1'][l].detach(), r['l2'][l].detach(), r['off'][l].detach()
            core[f'total_{tag}'] = r['total']
            for k, v in r['taps'].items():
                core[f'tap_{tag}/{k}'] = v
            for k, v in r['gtaps'].items():
                core[f'gtap_{tag}/{k}'] = v
        if name == 's1d':
            for tag in BLOCKS:
                b32, b64 = r32['blocks'][tag], r64['blocks'][tag]
                assert torch.equal(b32['mask'], b64['mask']) and torch.equal(b32['mask_out'], b64['mask_out'])
                core[f'blk/{tag}/mask'], core[f'blk/{tag}/mask_out'] = b32['mask'], b32['mask_out']
                for k in ('x', 'gx', 'y', 'gy') + (('kv',) if tag == 'dec' else ()):
                    core[f'blk/{tag}/{k}_32'], core[f'blk/{tag}/{k}_d'] = b32[k], (b64[k] - b32[k].double()).float()
                if tag == 'dec':
                    core[f'blk/{tag}/kv_mask'] = b32['kv_mask']
        for part, prefixes in SG.PARTS.items():
            gp = {}
            for k in names:
                if k.startswith(prefixes):
                    g32, g64 = r32['grads'][k], r64['grads'][k]
                    gp[f'32/{k}'], gp[f'd/{k}'] = g32, (g64 - g32.double()).float()
            SG.save(f'step_grad_drop_{name}_gp_{part}.npz', gp)
        sites = sorted(r32['log'])
        core['meta'] = {'case': name, 'T': T, 'lens': c['lens'], 'tok_lens': TOK_LENS, 'text_size': TEXT_SIZE, 'second_fusion': False,
                        'center_sampling': c['center_sampling'], 'reg_loss': c['reg_loss'], 'n_levels': L, 'level_lengths': sizes,
                        'n_params': len(names), 'loss_norm': SG.LOSS_NORM, 'positive_per_level': per_level, 'excluded': n_ex,
                        'parts': list(SG.PARTS), 'seed': key, 'proj_pdrop': PROJ, 'path_pdrop': PATH, 'refine_pdrop': TCN,
                        'path_sites': path_sites, 'blocks': BLOCKS if name == 's1d' else {},
                        'sites': [dict(site=s, shape=list(r32['log'][s][0]), kept=int(r32['log'][s][1].sum())) for s in sites]}
        SG.save(f'step_grad_drop_{name}.npz', core)


if __name__ == '__main__':
    main()
