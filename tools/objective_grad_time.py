"""Device time of the objective's gradient at the bench shape (T = 16384, L = 8): (a) the fused gradient call
(loss.PointObjective.grad into preallocated buffers: one launch), (b) value and gradient through autograd
(PointObjective(...)['total'].backward() on packed leaves) and (c) the reference's formulation on the same GPU -- torch ops with
boolean-mask indexing (`logits[masks]`, `offsets[pos]`), the losses as torch expressions, `backward()`; its annotation is done once
outside the timed region, so (c) is the loss and its backward alone.  All in one process, alternating, device events, warmed up;
the kernel's own time comes from the library's profiler.  GPU only, dev tool.

    python tools/objective_grad_time.py [calls]
"""
import ctypes, importlib, json, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import objective_cases as C  # noqa: E402
pkg = importlib.import_module('cvpr2025-decafnet_amd')
Ls = pkg.loss
N = int(sys.argv[1]) if len(sys.argv) > 1 else 200
T, L = C.BENCH['T'], C.BENCH['L']
sizes = C.level_sizes(T, L)
opt = pkg.config.make_opt(n_levels=L, max_seq_len=C.BENCH['max_seq_len'])
pg = pkg.modeling.PtGenerator(C.BENCH['max_seq_len'], L, 4, 0.5).cuda()


def focal(x, labels, alpha=0.5, smoothing=0.2):
    t = labels.float() * (1.0 - smoothing) + smoothing / 2
    p = torch.sigmoid(x)
    ce = torch.nn.functional.binary_cross_entropy_with_logits(x, t, reduction='none')
    loss = ce * (1 - (p * t + (1 - p) * (1 - t))) ** 2.0
    return ((alpha * labels + (1 - alpha) * (~labels)) * loss).sum()


def diou(pred, gt, eps=1e-8):
    lp, rp, lg, rg = pred[:, 0], pred[:, 1], gt[:, 0], gt[:, 1]
    inter = torch.min(rp, rg) + torch.min(lp, lg)
    union = (lp + rp) + (lg + rg) - inter
    hull = torch.max(lp, lg) + torch.max(rp, rg)
    return (1.0 - inter / union.clamp(min=eps) + torch.square(0.5 * (rp - lp - rg + lg) / hull.clamp(min=eps))).sum()


def torch_step(leaves, msk, labels, gt, loss_norm=160.0, ws=1, lw=1.0):
    for x in leaves:
        x.grad = None
    l1, l2, off = leaves
    pos = torch.logical_and(labels, msk)
    cls = (focal(l1[msk], labels[msk]) / loss_norm * ws + focal(l2[msk], labels[msk]) / loss_norm * ws) / 2
    reg = diou(off[pos], gt[pos]) / loss_norm * ws
    (cls + lw * reg).backward()


def autograd_step(obj, leaves, parts, msk_parts, tg):
    for x in leaves:
        x.grad = None
    obj((*parts, msk_parts), tg)['total'].backward()


for rows in (4, 24):
    l1, l2, off, msk, tg = (x.cuda() for x in C.bench_inputs(rows))
    parts = tuple(x.split(sizes, 1) for x in (l1, l2, off, msk))
    obj = Ls.PointObjective(opt)
    bufs = obj.grad(parts, tg)
    leaves = [x.clone().requires_grad_(True) for x in (l1, l2, off)]
    leaf_parts = tuple(x.split(sizes, 1) for x in leaves)
    labels, gt = Ls.annotate_points(torch.cat(pg(sizes)), tg)
    tleaves = [x.clone().requires_grad_(True) for x in (l1, l2, off)]
    fa = lambda: obj.grad(parts, tg, out=bufs)                                   # noqa: E731
    fb = lambda: autograd_step(obj, leaves, leaf_parts, parts[3], tg)           # noqa: E731
    fc = lambda: torch_step(tleaves, msk, labels, gt)                            # noqa: E731
    fa(), fb(), fc()
    for a, b, c in zip(bufs, leaves, tleaves):
        assert torch.equal(torch.cat(a, 1), b.grad)
        torch.testing.assert_close(b.grad, c.grad, rtol=1e-4, atol=1e-9)
    for _ in range(10):
        fa(), fb(), fc()
    ta, tb, tc = [], [], []
    for _ in range(N):
        for fn, acc in ((fa, ta), (fb, tb), (fc, tc)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            acc.append(e0.elapsed_time(e1) * 1e3)
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
    print(f"B' = {rows:2d}: fused gradient {med(ta):8.1f} us (min {min(ta):.1f})   value + backward() {med(tb):8.1f} us (min {min(tb):.1f})   "
          f'torch ops + backward() {med(tc):8.1f} us (min {min(tc):.1f})   ratio {med(tc) / med(ta):.1f}x / {med(tc) / med(tb):.1f}x   '
          f'[{N} calls each, alternating]', flush=True)
    # the kernel alone: the library's own profiler (device events around the launch)
    lib = pkg._lib.lib()
    lib.dcf_profile_enable(1)
    for _ in range(20):
        fa()
    torch.cuda.synchronize()
    need = lib.dcf_profile_report(None, 0)
    buf = ctypes.create_string_buffer(int(need) + 16)
    lib.dcf_profile_report(buf, len(buf))
    lib.dcf_profile_enable(0)
    print('    kernel alone (us per launch):', {k: round(1e3 * v['ms'] / v['count'], 1) for k, v in json.loads(buf.value.decode()).items()}, flush=True)
