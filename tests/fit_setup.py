"""What tests/test_gpu_loss_meter.py, tests/test_gpu_fit_parallel.py and tests/fit_rank_main.py share: the set-up of tests/test_gpu_fit.py
(the tiny model of tests/golden/step_grad_s2 built by ``modeling.create_model``, a generated tree of 5 videos with 9 queries, T = 80,
``front_end='shared'``, ``crop_ratio`` None, the validation set the same videos in a ``data.EvalBank``) as plain functions, so that two
fresh processes build the same objects as the test that compares them; and the host route of the validation loss."""
import numpy as np
import torch

import step_grad_ref as R
import train_data_tree as TT

T_IN = 80                                                                     # the input length of the training batches
N_VIDEOS = 5
N_VIDEOS_TWO_RANKS = 6                                                        # 8 training samples: two steps of two per rank and epoch


def build_world(pkg, root, n_videos=N_VIDEOS):
    """write the tree under ``root`` -> (fixture, cfg, eval data, eval bank)"""
    f = R.Fixture('s2')
    kw = f.opt_kwargs
    arrays, data = TT.random_tree(5, n_videos, kw['D'], kw['text_in'], T_IN, 9)
    TT.write_tree(root, arrays)
    return (f,) + open_world(pkg, f, root, n_videos, data)


def open_world(pkg, f, root, n_videos=N_VIDEOS, data=None):
    """the tree that lies under ``root`` -> (cfg, eval data, eval bank)"""
    kw = f.opt_kwargs
    if data is None:
        data = TT.random_tree(5, n_videos, kw['D'], kw['text_in'], T_IN, 9)[1]
    cfg = dict(TT.cfg_of(root, dict(data, crop_ratio=None)), eval_split=('train',))
    ed = pkg.data.VideoCentricEvalData(cfg)
    return cfg, ed, pkg.data.EvalBank(ed, vid_stride=kw['vid_stride'])


def make_opt(pkg, f):
    opt = f.opt(pkg)
    opt.train.warmup_epochs = 1
    return opt


def make_step(pkg, f, cfg, rank=0, world=1, cls=None, **kw):
    """fresh objects: (ts, loader) with two steps per epoch on every rank"""
    td = pkg.data.VideoCentricTrainData(cfg, num_epochs=2, seed=3)
    loader = pkg.data.TrainLoader(td, pkg.data.FeatureBank(td), len(td) // world // 2, rank=rank, world_size=world, input_vid_len=T_IN,
                                  vid_stride=f.opt_kwargs['vid_stride'])
    assert len(loader) == 2, (len(td), world)
    opt = make_opt(pkg, f)
    model = pkg.modeling.create_model(opt)
    model.load_state_dict(f.sd)
    cls = cls or pkg.train.TrainStep
    return cls(model.cuda(), opt, itrs_per_epoch=len(loader), front_end='shared', **kw), loader


def tensors(ts):
    """parameters, EMA copy and optimizer state as one list of tensors on the CPU"""
    out = [p.detach().cpu() for p in ts.model.parameters()] + [p.detach().cpu() for p in ts.ema.module.parameters()]
    for st in ts.optimizer.state_dict()['state'].values():
        out += [v.detach().cpu() for _, v in sorted(st.items()) if torch.is_tensor(v)]
    return out


def differing(a, b):
    """the indices at which two tensor lists differ in dtype, shape or any bit"""
    assert len(a) == len(b) and len(a) > 0
    u8 = lambda t: t.contiguous().reshape(-1).view(torch.uint8)
    return [i for i, (x, y) in enumerate(zip(a, b)) if x.dtype != y.dtype or x.shape != y.shape or not torch.equal(u8(x), u8(y))]


def host_loss(pkg, ev, ed, opt):
    """The host route of the validation loss: per video ``calc_loss`` on that video's forward (one host read each), then the mean of
    the stats as ``easy_reduce(loss_list, 'mean')`` takes it.  -> (rows (N, 4) fp32 as dcf_point_objective wrote them, per-row (N, 2)
    as calc_loss returns them, {'cls_loss', 'reg_loss'})"""
    E, L = pkg.evaluator, pkg.loss
    vs, levels = ev.vid_stride, ev.num_fpn_levels
    rows, per_row, stats = [], [], []
    params, use_offset = L.pt_gen_params(opt)
    tr = opt['train']
    for data in ed:
        flat, T = ev.forward(data)
        sizes = [(T // vs) >> l for l in range(levels)]
        outputs = tuple(tuple(torch.split(x, sizes, 1)) for x in flat)
        targets = ed.targets(data['clip_id'], vs).cuda()
        s, pr = E.calc_loss(outputs, targets, opt)
        stats.append(s), per_row.append(pr)
        rows.append(L._objective(outputs, targets, params, use_offset, tr.get('center_sampling', 'radius'), tr['center_sampling_radius'],
                                 0.5, 0.2, 'iou', None, 1, 1.0)[0].cpu())
    mean = {k: float(np.mean([s[k] for s in stats])) for k in ('cls_loss', 'reg_loss')}
    return torch.cat(rows), np.concatenate(per_row), mean


def loss_bound(bank):
    """(N + V) * 2^-52: sums of N + V non-negative doubles taken in two orders"""
    return (bank.meta.shape[0] + len(bank)) * 2.0 ** -52
