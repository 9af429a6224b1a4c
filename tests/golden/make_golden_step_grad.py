"""Generate tests/golden/step_grad_<case>*.npz: one whole training step of the reference -- its own
PtTransformerEarlyFusionIterative.forward(..., eval=False) (libs/modeling/model.py:567-632: the gate, the concatenation with the
shallow features, vid_map, encode_text, the first fusion, encode_video, fuse_and_predict), the Trainer's objective on its outputs
(libs/worker_v2.py:428-465, combined as make_golden_objective_grad.py::trainer_total combines it) and `total.backward()` -- in fp32
and, from the same model cast to fp64, in fp64 (the objective then by tests/objective_grad_ref.py's values, as that generator makes
its fp64 run).

Run where the reference is importable (not on the GPU machine):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_step_grad.py

Both cases: D = E = TE = text_in = 32, 3 pyramid levels, 2 heads, window 3, sn = 8, sratio = 0.5, `norm` on, n_stem = 1, a two-layer
text encoder with background token and position encoding; two videos, three queries of lengths [9, 5, 7], text_size = [2, 1]
    s2    vid_stride 2, msf, second_fusion; T = 80, lengths [80, 55] -> pyramid 40 / 20 / 10; center_sampling 'radius' with DIoU
    s1    vid_stride 1, no msf (the gate is and-ed into the mask: holes through vid_map, the fusion, every encoder level, the pooling
          chain and the heads), no second fusion; T = 40, lengths [40, 27]; center_sampling 'none' with GIoU
The model is .train() with every dropout probability 0: opt's rates are 0, the hard-wired ones (channel_drop, the refinement TCN's
Dropout(0.5)) are set to 0.  Parameters: biases and LayerNorm weights moved off their initial values by 0.1 N(0, 1), the LayerScales
set to 0.5 + 0.25 N(0, 1), the regression Scales to (1, 0.7, 1.3); parameters and inputs rounded to multiples of 2^-10.  The targets
put positive points on every level of the pyramid, so every regression Scale takes a gradient.

Files per case (each below the 1 MiB limit of a committed file), tensors in the reference's channel-major layout:
    step_grad_<case>.npz            meta, opt_kwargs, param/<name> (the state dict), vid, shallow, vid_masks, tokens, token_masks,
                                    text_cls, targets, gate, mask_gated, labels, gt_offsets, mask/l<i>, and by precision tag 32 / 64:
                                    logits1_<tag>/l<i>, logits2_<tag>/l<i>, offsets_<tag>/l<i>, total_<tag>, the forward taps
                                    tap_<tag>/vid_map, /text, /fused, /fpn<i> and the gradients gtap_<tag>/text, /fused
    step_grad_<case>_gp_<part>.npz  32/<name> -> the fp32 gradient of that parameter, d/<name> -> fp32(g_64 - g_32): the fp64 gradient is
                                    their sum in fp64 (exact to 2^-24 e_ref); split by top-level module: part `front` (vid_map,
                                    text_net, fusion), `vid_net`, `heads` (cls_head, refine, cls_head2, reg_head)

Conditions on the reference alone, asserted here and again on the committed files by tests/test_step_grad_cpu.py: the two precisions
agree on the gate, the masks and the labels; no positive point is a non-smooth point of the IoU loss; every parameter takes a
gradient; and for every parameter but the exactly-zero ones (key.bias, k_norm.bias: backbone_grad_ref.Fixture.top)
    e_ref = max |g_32 - g_64| <= 2^-15 max |g_64|
which guards against a ReLU, max-pool or top-k decision that differs between the precisions.  If a seed trips it, change the seed."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402
import objective_cases as C  # noqa: E402
import objective_grad_ref as OR  # noqa: E402

LIMIT = 1 << 20
E_REF_CAP = 2.0 ** -15
BASE = dict(D=32, E=32, TE=32, text_in=32, n_levels=3, win=3, n_heads=2, sn=8, sratio=0.5, norm=True, max_seq_len=64, text_layers=2,
            text_max_len=24, text_use_abs_pe=True, n_stem=1)
TOK_LENS, TEXT_SIZE = [9, 5, 7], [2, 1]
# targets in level-0 positions (the Trainer divides by vid_stride, worker_v2.py:417).  s2: those of tests/test_gpu_refine_grad.py.  s1: the
# gate leaves row 0 the positions 16-31, row 1 0-7 and 32-39, row 2 0-6 and 14-20; a short segment inside a kept block gives the level-0
# points, a long one across two kept blocks of row 2 the level-2 points
CASES = {
    's2': dict(opt=dict(BASE, vid_stride=2, msf=True), second_fusion=True, T=80, lens=[80, 55], center_sampling='radius', reg_loss='diou',
               seed=20256, targets=[[4.0, 21.0], [3.0, 8.5], [20.0, 25.5]]),
    's1': dict(opt=dict(BASE, vid_stride=1, msf=False), second_fusion=False, T=40, lens=[40, 27], center_sampling='none', reg_loss='giou',
               seed=20257, targets=[[18.25, 23.25], [32.5, 39.5], [10.5, 21.5]]),
}
SCALES = {'0': 1.0, '1': 0.7, '2': 1.3}
PARTS = {'front': ('vid_map.', 'text_net.', 'fusion.'), 'vid_net': ('vid_net.',), 'heads': ('cls_head.', 'refine.', 'cls_head2.', 'reg_head.')}
ZERO_BY_SYMMETRY = ('key.bias', 'k_norm.bias')
LOSS_NORM, WORLD_SIZE, LOSS_WEIGHT = 160.0, 1, 1.0            # config.make_opt's opt.train
WARMUP = 2


def coarse(x):
    return torch.round(x * 1024) / 1024


def save(name, d):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **MG.npify(d))
    print(name, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < LIMIT, name


def perturb(model, t):
    with torch.no_grad():
        for k, p in model.named_parameters():
            if '.scales.' in k:
                p.fill_(SCALES[k.split('.')[2]])
            elif k.endswith(('drop_path_attn.scale', 'drop_path_ffn.scale')):
                p.copy_(0.5 + 0.25 * t(*p.shape))
            elif k.endswith('bias') or 'norm' in k or 'ln_' in k:                       # biases and the LayerNorm weights
                p.add_(0.1 * t(*p.shape))
            p.copy_(coarse(p))


def main():
    MG.install_stubs()
    from libs.modeling.model import PtGenerator, PtTransformerEarlyFusionIterative
    from libs.worker_v2 import annotate_points_per_video, calc_focal_loss, calc_iou_loss

    def trainer_total(l1, l2, off, msk, labels, gt_off, reg_loss):
        """make_golden_objective_grad.py::trainer_total"""
        pos = torch.logical_and(labels, msk)
        cls1 = calc_focal_loss(logits=l1[msk], labels=labels[msk], alpha=C.FC_A, smoothing=C.FC_S) / LOSS_NORM * WORLD_SIZE
        cls2 = calc_focal_loss(logits=l2[msk], labels=labels[msk], alpha=C.FC_A, smoothing=C.FC_S) / LOSS_NORM * WORLD_SIZE
        reg = calc_iou_loss(pred_offsets=off[pos], gt_offsets=gt_off[pos], reg_loss=reg_loss) / LOSS_NORM * WORLD_SIZE
        return (cls1 + cls2) / 2 + LOSS_WEIGHT * reg

    for name, c in CASES.items():
        rs = np.random.RandomState(c['seed'])
        t = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32))
        torch.manual_seed(c['seed'])
        kw, T, D = c['opt'], c['T'], c['opt']['D']
        L, stride = kw['n_levels'], kw['vid_stride']

        def make():
            net = PtTransformerEarlyFusionIterative(MG.make_opt(**kw).clone(), second_fusion=c['second_fusion'])
            for mod in net.modules():
                if isinstance(mod, (torch.nn.Dropout, torch.nn.Dropout1d)):               # channel_drop, the TCN's Dropout(0.5)
                    mod.p = 0.0
            return net

        proto = make()
        perturb(proto, t)
        names = [k for k, _ in proto.named_parameters()]
        assert all(k.startswith(sum(PARTS.values(), ())) for k in names)
        bs, nq, lq = len(c['lens']), sum(TEXT_SIZE), max(TOK_LENS)
        vid_masks = torch.arange(T)[None, :] < torch.tensor(c['lens'])[:, None]
        vid, shallow = coarse(t(bs, D, T)) * vid_masks[:, None], coarse(t(bs, D, T)) * vid_masks[:, None]
        token_masks = (torch.arange(lq)[None, :] < torch.tensor(TOK_LENS)[:, None])[:, None]      # (B', 1, Lq)
        tokens = coarse(t(nq, kw['text_in'], lq)) * token_masks
        text_cls = coarse(t(nq, D))
        text_pad = torch.zeros(bs, max(TEXT_SIZE), kw['text_in'], lq)                 # the padded layout of the training collate
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

        def run(dt, reference_loss):
            net = make()
            net.load_state_dict(proto.state_dict())
            net = net.to(dt).train()
            tap = {}
            net.vid_map.register_forward_pre_hook(lambda m, a: tap.update(vid_map_in=a[0].detach(), mask_gated=a[1][:, 0]))
            net.vid_map.register_forward_hook(lambda m, a, o: tap.update(vid_map=o[0]))

            def keep(key):
                def hook(m, a, o):                                                     # (a hook that returns a value would replace the output)
                    if not isinstance(o[0], tuple):                                    # the second fusion hands over a tuple of levels
                        o[0].retain_grad()
                        tap[key] = o[0]
                return hook

            net.text_net.register_forward_hook(keep('text'))
            net.fusion.register_forward_hook(keep('fused'))
            net.vid_net.register_forward_hook(lambda m, a, o: tap.update(fpn=o[0]))
            l1, l2, off, mo = net(vid.to(dt), shallow.to(dt), vid_masks, text_pad.to(dt), text_cls.to(dt), mask_pad, text_size=torch.tensor(TEXT_SIZE))
            msk = torch.cat(mo, 1).reshape(nq, -1)
            cl1, cl2, coff = torch.cat(l1, 1), torch.cat(l2, 1), torch.cat(off, 1)
            if reference_loss:
                total = trainer_total(cl1, cl2, coff, msk, labels, gt_off.to(dt), c['reg_loss'])
            else:
                total = OR.objective_value(cl1, cl2, coff, msk, labels, gt_off.to(dt), c['reg_loss'], LOSS_NORM, WORLD_SIZE, LOSS_WEIGHT, C.FC_A, C.FC_S, dt)
            total.backward()
            x_in = tap['vid_map_in']
            rep = vid.repeat_interleave(torch.tensor(TEXT_SIZE), dim=0).to(dt)
            gate = (x_in[:, :D] != 0).any(1)
            assert torch.equal(x_in[:, :D], rep * gate[:, None].to(dt)), 'the gate could not be read off the input of vid_map'
            grads = {k: p.grad for k, p in net.named_parameters()}
            assert list(grads) == names and all(g is not None for g in grads.values()), [k for k, g in grads.items() if g is None]
            return dict(l1=l1, l2=l2, off=off, masks=[m.reshape(nq, -1) for m in mo], total=total.detach(), gate=gate,
                        mask_gated=tap['mask_gated'], msk=msk, coff=coff.detach(), grads=grads,
                        taps={'vid_map': tap['vid_map'].detach(), 'text': tap['text'].detach(), 'fused': tap['fused'].detach(),
                              **{f'fpn{l}': x.detach() for l, x in enumerate(tap['fpn'])}},
                        gtaps={'text': tap['text'].grad, 'fused': tap['fused'].grad})

        # the scripted loss functions of the reference: warm-up calls first, then two that must agree (make_golden_objective_grad.py)
        for _ in range(WARMUP):
            run(torch.float32, True)
        r32, again = run(torch.float32, True), run(torch.float32, True)
        assert all(torch.equal(r32['grads'][k], again['grads'][k]) for k in names), 'the fp32 gradient changed between calls'
        r64 = run(torch.float64, False)
        e_tot = abs(float(r64['total']) - float(OR.objective_value(*(torch.cat([x.detach() for x in r32[k]], 1) for k in ('l1', 'l2', 'off')), r32['msk'],
                                                                   labels, gt_off, c['reg_loss'], LOSS_NORM, WORLD_SIZE, LOSS_WEIGHT, C.FC_A, C.FC_S)))
        print(f'{name}: total {float(r64["total"]):.9f} (fp32 {float(r32["total"]):.9f}; restated objective on the fp32 outputs differs by {e_tot:.2e})')

        # ---- conditions on the reference alone
        assert torch.equal(r32['gate'], r64['gate']) and torch.equal(r32['mask_gated'], r64['mask_gated']), 'gate decisions differ'
        assert all(torch.equal(a, b) for a, b in zip(r32['masks'], r64['masks']))
        pos = labels & r32['msk']
        lv = np.cumsum([0] + sizes)
        per_level = [int(pos[:, lv[l]:lv[l + 1]].sum()) for l in range(L)]
        n_ex = sum(int((OR.non_smooth(r[k], gt_off) & pos).sum()) for r, k in ((r32, 'coff'), (r64, 'coff')))
        print(f'{name}: positive points per level {per_level}, {n_ex} excluded; gate keeps {r32["gate"].sum(1).tolist()} of '
              f'{vid_masks.repeat_interleave(torch.tensor(TEXT_SIZE), 0).sum(1).tolist()} valid positions per row')
        for r in range(nq):
            print('   row', r, 'valid', ''.join('x' if v else '.' for v in r32['msk'][r, :sizes[0]].tolist()), 'positive', torch.nonzero(pos[r])[:, 0].tolist(),
                  'offsets', [[round(z, 3) for z in o] for o in r32['coff'][r][pos[r]].tolist()])
        assert min(per_level) >= 1 and n_ex == 0
        assert int(r32['gate'].sum()) > 0 and not bool(r32['gate'][vid_masks.repeat_interleave(torch.tensor(TEXT_SIZE), 0)].all())
        rows, worst = [], (0.0, None)
        print(f'{"parameter":58s} {"max|g64|":>10s} {"e_ref":>10s} {"e_ref/max":>10s}')
        for k in names:
            g32, g64 = r32['grads'][k].double(), r64['grads'][k]
            top, e = float(g64.abs().max()), float((g32 - g64).abs().max())
            zero = k.endswith(ZERO_BY_SYMMETRY)
            if zero:                                              # three roundings of 0: the scale is that of the same layer's weight
                top = float(r64['grads'][k[:-len('bias')] + 'weight'].abs().max())
            rel = e / top if top else float('inf')
            rows.append(rel)
            print(f'{k:58s} {top:10.3e} {e:10.3e} {rel:10.3e}{"  (zero in exact arithmetic)" if zero else ""}')
            assert top > 0, k
            if not zero:
                assert rel <= E_REF_CAP, (k, rel)
                worst = max(worst, (rel, k))
        print(f'{name}: {len(names)} parameters, worst e_ref / max|g64| {worst[0]:.3e} ({worst[1]}), median {float(np.median(rows)):.3e}, '
              f'smallest max|g64| {min(float(r64["grads"][k].abs().max()) for k in names if not k.endswith(ZERO_BY_SYMMETRY)):.3e}')

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
        for part, prefixes in PARTS.items():
            gp = {}
            for k in names:
                if k.startswith(prefixes):
                    g32, g64 = r32['grads'][k], r64['grads'][k]
                    gp[f'32/{k}'], gp[f'd/{k}'] = g32, (g64 - g32.double()).float()
                    assert float((g32.double() + gp[f'd/{k}'].double() - g64).abs().max()) <= 2.0 ** -23 * float(gp[f'd/{k}'].abs().max()), k
            save(f'step_grad_{name}_gp_{part}.npz', gp)
        core['meta'] = {'case': name, 'T': T, 'lens': c['lens'], 'tok_lens': TOK_LENS, 'text_size': TEXT_SIZE, 'second_fusion': c['second_fusion'],
                        'center_sampling': c['center_sampling'], 'reg_loss': c['reg_loss'], 'n_levels': L, 'level_lengths': sizes,
                        'n_params': len(names), 'loss_norm': LOSS_NORM, 'positive_per_level': per_level, 'excluded': n_ex, 'parts': list(PARTS)}
        save(f'step_grad_{name}.npz', core)


if __name__ == '__main__':
    main()
