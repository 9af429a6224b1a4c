"""Generate tests/golden/front_grad_<case>.npz: the first stage of one training step of the reference -- the gate, the
concatenation and vid_map of PtTransformerEarlyFusionIterative.forward(..., eval=False) (libs/modeling/model.py:567-616) -- with the
upstream gradient the rest of the step sends back into it, for the four input layouts of vid_map:

    msf+scat (Cin = 2 D + 1), msf (2 D), nomsf+scat (D + 1), nomsf (D)

The step is make_golden_step_grad.py's: the model in train() with every dropout at 0, run in fp32 and, cast to fp64, in fp64, through
the Trainer's objective and backward().  Hooks on model.vid_map capture its input, its output and grad_output.

Run where the reference is importable (not on the GPU machine):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_front_grad.py

Shape: D = 32, E = 64, two videos with text_size [2, 1], T = 200, lengths [200, 139] (64-clip tiles 64 + 64 + 64 + 8, the second
video with a padded tail), sn = 8, sratio = 0.25, norm on, a small pyramid and heads as in BASE of the step generator.  The shallow
features are a slowly drifting sequence on the 2^-10 grid (an AR(1) walk per channel), so that the blocks the gate keeps cluster and
whole tiles stay closed.

Stored per case (channel-major as the reference holds them): vid, shallow (2, D, T), vid_masks, text_cls, text_size, W (E, Cin), bias,
gate / mask_gated / correl (B', T; correl_d: the fp64 run's scores as a difference), Y_32 (B', E, T), dY (the fp32 run's grad_output), dW_32 / db_32 (the reference's fp32
vid_map.conv.weight.grad / bias.grad), and the fp64 yardstick as differences Y_d, dW_d, db_d: x_64 = x_32 + d in fp64.  The yardstick is
the reference's own vid_map module in double on the captured fp64 input with dY.double() as the upstream gradient.

Asserted here and again on the committed files by tests/test_front_grad_cpu.py: the fp32 and fp64 gates and masks are equal; the
two-query video has at least one 64-clip tile closed for both queries and one kept by exactly one of them; a gate block edge falls
inside a tile; e_ref <= 2^-15 max |x_64| for Y, dW, db.  If a seed trips a condition, the next one is tried (the seed is recorded)."""
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402
import make_golden_step_grad as SG  # noqa: E402
import objective_cases as C  # noqa: E402
import objective_grad_ref as OR  # noqa: E402

LIMIT = 1 << 20
E_REF_CAP = 2.0 ** -15
TILE = 64
BASE = dict(D=32, E=64, TE=32, text_in=32, n_levels=3, win=3, n_heads=2, sn=8, sratio=0.25, norm=True, max_seq_len=256, text_layers=2,
            text_max_len=24, text_use_abs_pe=True, n_stem=1, vid_stride=1)
T, LENS, TOK_LENS, TEXT_SIZE = 200, [200, 139], [9, 5, 7], [2, 1]
TARGETS = [[20.0, 41.0], [100.5, 131.0], [30.0, 60.5]]
CASES = {'msf+scat': dict(msf=True, scat=True), 'msf': dict(msf=True, scat=False), 'nomsf+scat': dict(msf=False, scat=True),
         'nomsf': dict(msf=False, scat=False)}
FIRST_SEED, MAX_TRIES = 30100, 40


def save_npz(path, arrays):
    """np.savez_compressed with a fixed time stamp on every member: run twice, the generator writes the same bytes"""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for k in arrays:
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def file_name(case):
    return f'front_grad_{case}.npz'


def tile_conditions(gate, sizes, lens):
    """gate (B', T) bool.  -> (closed_for_both, kept_by_one, edge_inside): on the first video with two queries, a 64-clip tile no query
    keeps, a tile exactly one query keeps; on any row, a 0/1 edge of the gate at a position that is no multiple of 64"""
    q = 0
    closed = one = False
    for b, k in enumerate(sizes):
        if k == 2:
            for t0 in range(0, lens[b], TILE):
                kept = [bool(gate[q + j, t0:t0 + TILE].any()) for j in range(2)]
                closed |= not any(kept)
                one |= sum(kept) == 1
        q += k
    edges = torch.nonzero(gate[:, 1:] != gate[:, :-1])[:, 1] + 1
    return closed, one, bool((edges % TILE != 0).any())


def build(case, flags, seed):
    from libs.modeling.model import PtGenerator, PtTransformerEarlyFusionIterative
    from libs.worker_v2 import annotate_points_per_video, calc_focal_loss, calc_iou_loss
    rs = np.random.RandomState(seed)
    t = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32))
    torch.manual_seed(seed)
    kw = dict(BASE, **flags)
    D, L = kw['D'], kw['n_levels']

    def make():
        net = PtTransformerEarlyFusionIterative(MG.make_opt(**kw).clone(), second_fusion=False)
        for mod in net.modules():
            if isinstance(mod, (torch.nn.Dropout, torch.nn.Dropout1d)):
                mod.p = 0.0
        return net

    proto = make()
    SG.perturb(proto, t)
    bs, nq, lq = len(LENS), sum(TEXT_SIZE), max(TOK_LENS)
    vid_masks = torch.arange(T)[None, :] < torch.tensor(LENS)[:, None]
    vid = SG.coarse(t(bs, D, T)) * vid_masks[:, None]
    walk = torch.zeros(bs, D, T)
    step = t(bs, D, T)
    walk[..., 0] = step[..., 0]
    for i in range(1, T):                                            # AR(1): neighbouring clips look alike, so kept blocks cluster
        walk[..., i] = 0.97 * walk[..., i - 1] + 0.25 * step[..., i]
    shallow = SG.coarse(walk) * vid_masks[:, None]
    token_masks = (torch.arange(lq)[None, :] < torch.tensor(TOK_LENS)[:, None])[:, None]
    tokens = SG.coarse(t(nq, kw['text_in'], lq)) * token_masks
    text_cls = SG.coarse(t(nq, D))
    text_pad = torch.zeros(bs, max(TEXT_SIZE), kw['text_in'], lq)
    mask_pad = torch.zeros(bs, max(TEXT_SIZE), lq, dtype=torch.bool)
    q = 0
    for b, k in enumerate(TEXT_SIZE):
        text_pad[b, :k], mask_pad[b, :k] = tokens[q:q + k], token_masks[q:q + k, 0]
        q += k
    targets = torch.tensor(TARGETS)
    sizes = [T >> l for l in range(L)]
    points = torch.cat(PtGenerator(kw['max_seq_len'], L, 4, 0.5, use_offset=False)(sizes))
    ann = [annotate_points_per_video(points, tg, center_sampling='none', center_sampling_radius=C.RADIUS) for tg in targets]
    labels, gt_off = torch.stack([a[0] for a in ann]), torch.stack([a[1] for a in ann])

    def trainer_total(l1, l2, off, msk):
        pos = torch.logical_and(labels, msk)
        cls1 = calc_focal_loss(logits=l1[msk], labels=labels[msk], alpha=C.FC_A, smoothing=C.FC_S) / SG.LOSS_NORM * SG.WORLD_SIZE
        cls2 = calc_focal_loss(logits=l2[msk], labels=labels[msk], alpha=C.FC_A, smoothing=C.FC_S) / SG.LOSS_NORM * SG.WORLD_SIZE
        reg = calc_iou_loss(pred_offsets=off[pos], gt_offsets=gt_off[pos], reg_loss='giou') / SG.LOSS_NORM * SG.WORLD_SIZE
        return (cls1 + cls2) / 2 + SG.LOSS_WEIGHT * reg

    def run(dt, reference_loss):
        net = make()
        net.load_state_dict(proto.state_dict())
        net = net.to(dt).train()
        tap = {}
        net.vid_map.register_forward_pre_hook(lambda m, a: tap.update(x=a[0].detach(), mask=a[1][:, 0]))

        def after(m, a, o):
            tap['y'] = o[0].detach()
            o[0].register_hook(lambda g: tap.update(dy=g.detach()))

        net.vid_map.register_forward_hook(after)
        l1, l2, off, mo = net(vid.to(dt), shallow.to(dt), vid_masks, text_pad.to(dt), text_cls.to(dt), mask_pad, text_size=torch.tensor(TEXT_SIZE))
        msk = torch.cat(mo, 1).reshape(nq, -1)
        cl1, cl2, coff = torch.cat(l1, 1), torch.cat(l2, 1), torch.cat(off, 1)
        if reference_loss:
            total = trainer_total(cl1, cl2, coff, msk)
        else:
            total = OR.objective_value(cl1, cl2, coff, msk, labels, gt_off.to(dt), 'giou', SG.LOSS_NORM, SG.WORLD_SIZE, SG.LOSS_WEIGHT, C.FC_A, C.FC_S, dt)
        total.backward()
        x = tap['x']
        rep = vid.repeat_interleave(torch.tensor(TEXT_SIZE), dim=0).to(dt)
        gate = (x[:, :D] != 0).any(1)
        assert torch.equal(x[:, :D], rep * gate[:, None].to(dt)), 'the gate could not be read off the input of vid_map'
        correl = x[:, -1] if flags['scat'] else None
        return dict(net=net, x=x, gate=gate, mask=tap['mask'], correl=correl, y=tap['y'], dy=tap['dy'],
                    dw=net.vid_map.conv.weight.grad[:, :, 0].clone(), db=net.vid_map.conv.bias.grad.clone())

    for _ in range(SG.WARMUP):
        run(torch.float32, True)
    r32, r64 = run(torch.float32, True), run(torch.float64, False)
    if not (torch.equal(r32['gate'], r64['gate']) and torch.equal(r32['mask'], r64['mask'])):
        return None, 'the precisions disagree on the gate'
    cond = tile_conditions(r32['gate'], TEXT_SIZE, LENS)
    if not all(cond):
        return None, f'tile conditions (closed for both, kept by one, edge inside a tile) = {cond}'
    # the yardstick: the reference's own vid_map in double on the captured fp64 input, dY of the fp32 run as the upstream gradient
    vm = r64['net'].vid_map
    vm.zero_grad()
    y64, _ = vm(r64['x'], r64['mask'][:, None])
    y64.backward(r32['dy'].double())
    g64 = {'Y': y64.detach(), 'dW': vm.conv.weight.grad[:, :, 0], 'db': vm.conv.bias.grad}
    g32 = {'Y': r32['y'], 'dW': r32['dw'], 'db': r32['db']}
    rel = {}
    for k in g64:
        rel[k] = float((g32[k].double() - g64[k]).abs().max()) / float(g64[k].abs().max())
        if not rel[k] <= E_REF_CAP:
            return None, f'e_ref of {k} = {rel[k]:.3e} max |x_64|'
    d = {'meta': {'case': case, 'seed': seed, 'T': T, 'lens': LENS, 'text_size': TEXT_SIZE, 'D': D, 'E': kw['E'], 'sn': kw['sn'],
                  'sratio': kw['sratio'], 'norm': kw['norm'], 'e_ref_rel': rel, **flags},
         'vid': vid, 'shallow': shallow, 'vid_masks': vid_masks, 'text_cls': text_cls,
         'W': proto.vid_map.conv.weight.detach()[:, :, 0].clone(), 'bias': proto.vid_map.conv.bias.detach().clone(),
         'gate': r32['gate'], 'mask_gated': r32['mask'], 'Y_32': r32['y'], 'dY': r32['dy'], 'dW_32': r32['dw'], 'db_32': r32['db']}
    if flags['scat']:
        d['correl'] = r32['correl']
        d['correl_d'] = (r64['correl'] - r32['correl'].double()).float()      # the fp64 run's scores: the yardstick's input channel
    for k in g64:
        d[f'{k}_d'] = (g64[k] - g32[k].double()).float()
    return d, rel


def main():
    MG.install_stubs()
    for case, flags in CASES.items():
        for seed in range(FIRST_SEED, FIRST_SEED + MAX_TRIES):
            d, why = build(case, flags, seed)
            if d is not None:
                break
            print(f'{case}: seed {seed} rejected: {why}')
        assert d is not None, case
        path = os.path.join(HERE, file_name(case))
        save_npz(path, MG.npify(d))
        size = os.path.getsize(path)
        print(f'{case}: seed {seed}, e_ref / max|x_64| {why}, gate keeps {d["gate"].sum(1).tolist()}, {size} bytes')
        assert size < LIMIT, case


if __name__ == '__main__':
    main()
