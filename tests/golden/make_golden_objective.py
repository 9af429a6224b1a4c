"""Generate tests/golden/objective.npz: point annotation and the Trainer's / Evaluator's loss values from the reference's own
functions (annotate_points_per_video, calc_focal_loss, calc_iou_loss of libs/worker_v2.py, PtGenerator of libs/modeling/model.py),
combined exactly as Trainer._microbatch_forward_backward (worker_v2.py:441-476) and Evaluator._calc_loss (:1029-1061) combine them.

Run where the reference is importable (not on the GPU machine):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_objective.py

Cases: tests/objective_cases.py.  Small: the model outputs stored in train.npz (and the 'late' case of train_secondary.npz for the
single-head form).  Bench scale: inputs regenerated from a seed; stored are the labelled points as index lists, SHA-256 digests of
the reference's offsets and predicates (a megabyte each otherwise), its fp32 results and the same sums accumulated in fp64.
"""
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402
import objective_cases as C  # noqa: E402


def digest(t):
    return hashlib.sha256(np.ascontiguousarray(t.numpy()).tobytes()).hexdigest()


def main():
    MG.install_stubs()
    from libs.modeling.model import PtGenerator
    from libs.worker_v2 import annotate_points_per_video, calc_focal_loss, calc_iou_loss

    def annotate(points, targets, mode):
        ls, os_, ws, rs = [], [], [], []
        for t in targets:
            l, o, (w, r) = annotate_points_per_video(points, t, center_sampling=mode, center_sampling_radius=C.RADIUS)
            ls.append(l), os_.append(o), ws.append(w), rs.append(r)
        return torch.stack(ls), torch.stack(os_), torch.stack(ws), torch.stack(rs)

    def trainer(l1, l2, off, msk, labels, gt_off, reg_loss, loss_norm, ws, lw):
        """worker_v2.py:441-476 with self.loss_norm, get_world_size(), self.loss_weight as arguments; l1 None: one head"""
        pos = torch.logical_and(labels, msk)
        norm = pos.sum()
        cls2 = calc_focal_loss(logits=l2[msk], labels=labels[msk], alpha=C.FC_A, smoothing=C.FC_S) / loss_norm * ws
        if l1 is not None:
            cls1 = calc_focal_loss(logits=l1[msk], labels=labels[msk], alpha=C.FC_A, smoothing=C.FC_S) / loss_norm * ws
            cls = (cls1 + cls2) / 2
        else:
            cls = cls2
        reg = calc_iou_loss(pred_offsets=off[pos], gt_offsets=gt_off[pos], reg_loss=reg_loss) / loss_norm * ws
        total = cls + lw * reg
        return torch.stack([cls, reg, total, norm.to(torch.float32)]), int(norm)

    def evaluator(l2, off, msk, labels, gt_off):
        """worker_v2.py:1043-1060 per row, easy_reduce(..., 'mean', skip_nan=True) over the rows"""
        rows = []
        for i in range(l2.size(0)):
            m, l, o = msk[i:i + 1], labels[i:i + 1], gt_off[i:i + 1]
            pos = torch.logical_and(l, m)
            norm = max(pos.sum().item(), 1)
            cls = calc_focal_loss(l2[i:i + 1][m], l[m], reduction='sum') / norm
            reg = calc_iou_loss(off[i:i + 1][pos], o[pos], reg_loss='iou', reduction='sum') / norm
            rows.append([cls.item(), reg.item()])
        rows = np.asarray(rows, dtype=np.float64)
        mean = [float(np.mean([x for x in rows[:, k] if not np.isnan(x)])) for k in range(2)]
        return rows, np.asarray(mean)

    def sums64(l1, l2, off, msk, labels, gt_off, reg_loss):
        """per row (focal1, focal2, iou, n_pos): the reference's fp32 element values, added in fp64"""
        rows = []
        for i in range(l2.size(0)):
            m, l = msk[i], labels[i]
            pos = torch.logical_and(l, m)
            f = [calc_focal_loss(x[i][m], l[m], alpha=C.FC_A, smoothing=C.FC_S, reduction='none').double().sum().item() for x in (l1, l2)]
            r = calc_iou_loss(off[i][pos], gt_off[i][pos], reg_loss=reg_loss, reduction='none').double().sum().item()
            rows.append(f + [r, float(pos.sum())])
        return np.asarray(rows, dtype=np.float64)

    out = {}
    # ------------------------------------------------------------------ small
    g = np.load(os.path.join(HERE, 'train.npz'))
    L = C.SMALL['L']
    cat = lambda n, z=g, p='': torch.cat([torch.from_numpy(z[f'{p}{n}/l{l}']) for l in range(L)], 1)      # noqa: E731
    l1, l2, off, msk = cat('logits1'), cat('logits2'), cat('offsets'), cat('masks')
    sec = np.load(os.path.join(HERE, 'train_secondary.npz'))
    sl, so, sm = cat('logits', sec, 'late/'), cat('offsets', sec, 'late/'), cat('masks', sec, 'late/')
    counts = {}
    for uo in (False, True):
        pg = PtGenerator(C.SMALL['max_seq_len'], L, C.SMALL['regression_range'], C.SMALL['sigma'], use_offset=uo)
        points = torch.cat(pg(C.level_sizes(C.SMALL['T'], L)))
        for bn, (tg, rows) in C.SMALL_BATCHES.items():
            tg = torch.tensor(tg, dtype=torch.float32)
            for mode, (cs, reg_loss) in C.MODES.items():
                labels, gt_off, win, rng = annotate(points, tg, cs)
                k = f'small/{bn}/{mode}/uo{int(uo)}'
                out[f'{k}/labels'], out[f'{k}/in_window'], out[f'{k}/in_range'] = labels, win, rng
                out[f'small/{bn}/uo{int(uo)}/offsets'] = gt_off
                if uo:
                    continue
                a1, a2, ao, am = l1[rows], l2[rows], off[rows], msk[rows]
                counts[f'{bn}/{mode}'] = [labels.sum(1).tolist(), (labels & am).sum(1).tolist()]
                res = [trainer(a1, a2, ao, am, labels, gt_off, reg_loss, ln, ws, lw)[0] for ln, ws, lw in C.GRID]
                out[f'small/{bn}/{mode}/trainer'] = torch.stack(res)                                   # (len(GRID), 4)
                out[f'small/{bn}/{mode}/rows64'] = sums64(a1, a2, ao, am, labels, gt_off, reg_loss)
                if mode == 'radius':
                    out[f'small/{bn}/eval_rows'], out[f'small/{bn}/eval_mean'] = evaluator(a2, ao, am, labels, gt_off)
                    if bn == 'a':                                                                      # single-head form
                        out['small/late/trainer'] = trainer(None, sl, so, sm, labels, gt_off, reg_loss, 160.0, 1, 1.0)[0]
                        out['small/late/eval_rows'], out['small/late/eval_mean'] = evaluator(sl, so, sm, labels, gt_off)
    out['small/counts'] = counts
    print('small: labelled / positive per row', counts)

    # ------------------------------------------------------------------ bench scale
    T, L = C.BENCH['T'], C.BENCH['L']
    b1, b2, bo, bm, tg = C.bench_inputs()
    counts = {}
    for uo in (False, True):
        pg = PtGenerator(C.BENCH['max_seq_len'], L, C.BENCH['regression_range'], C.BENCH['sigma'], use_offset=uo)
        points = torch.cat(pg(C.level_sizes(T, L)))
        for mode, (cs, reg_loss) in C.MODES.items():
            labels, gt_off, win, rng = annotate(points, tg, cs)
            k = f'bench/{mode}/uo{int(uo)}'
            out[f'{k}/label_idx'] = torch.nonzero(labels)                                              # (n, 2): row, point
            out[f'{k}/sha'] = dict(offsets=digest(gt_off), in_window=digest(win), in_range=digest(rng))
            if uo:
                continue
            counts[mode] = [labels.sum(1).tolist(), (labels & bm).sum(1).tolist()]
            ref32, norm = trainer(b1, b2, bo, bm, labels, gt_off, reg_loss, 160.0, 1, 1.0)
            rows = sums64(b1, b2, bo, bm, labels, gt_off, reg_loss)
            f1, f2, io = (rows[:, q].sum() for q in range(3))
            cls, reg = (f1 / 160.0 + f2 / 160.0) / 2, io / 160.0
            ref64 = np.asarray([cls, reg, cls + reg, float(norm)])
            out[f'bench/{mode}/trainer32'], out[f'bench/{mode}/trainer64'] = ref32, ref64
            out[f'bench/{mode}/dev'] = np.abs(ref32.double().numpy() - ref64)                          # |fp32 reference - fp64|
            out[f'bench/{mode}/rows64'] = rows
            print(f'bench {mode}: fp32 {ref32.tolist()} fp64 {ref64.tolist()} |dev| {out[f"bench/{mode}/dev"].tolist()}')
    out['bench/counts'] = counts
    print('bench: labelled / positive per row', counts)
    MG.save('objective.npz', out)


if __name__ == '__main__':
    main()
