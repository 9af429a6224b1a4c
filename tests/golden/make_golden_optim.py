"""Generate tests/golden/optim_ref.npz: what the reference's own optimizer and scheduler factories produce
(libs/modeling/optim.py:66-239 make_optimizer, :485-717 the two warm-up schedulers and make_scheduler).  Names and numbers only:

    groups          JSON {model: {'decay': [...], 'no_decay': [...], 'weight_decay': [wd of group 0, wd of group 1]}} for the models of
                    tests/golden/step_grad_s1.npz, step_grad_s2.npz and the default config.make_opt(): the parameter names of the two
                    groups of the reference's make_optimizer, in the order of the groups' parameter lists (sorted)
    sched           JSON {config name: the `opt['scheduler']` dict handed to the reference's make_scheduler, plus 'lr' and 'n'}
    lr/<config>     float64 [n]: group 0's lr after each of n calls of the reference scheduler's step() (each preceded by
                    optimizer.step(), as the Trainer calls them), base lr as in 'sched'

Run where the reference is importable (not on the GPU machine):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_optim.py

The archive is written with fixed member timestamps: a second run reproduces the file byte for byte."""
import io
import json
import os
import sys
import warnings
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402
from conftest import Golden  # noqa: E402

OUT = 'optim_ref.npz'
OPTIMIZER = dict(name='adamw', lr=1e-3, weight_decay=0.05, clip_grad_norm=1.0)          # libs/core/opt.py:160-164
# six schedules, 40 - 60 iterations each; itrs_per_epoch is what the Trainer sets from its data loader (worker_v2.py:252)
SCHEDULES = {
    'multistep_plain': dict(name='multistep', steps=(2,), gamma=0.1, warmup_epochs=0, epochs=5, itrs_per_epoch=8, lr=1e-3, n=40),
    'multistep_warmup': dict(name='multistep', steps=(3,), gamma=0.5, warmup_epochs=2, epochs=5, itrs_per_epoch=6, lr=2e-3, n=48),
    'multistep_two': dict(name='multistep', steps=(2, 3), gamma=0.1, warmup_epochs=1, epochs=5, itrs_per_epoch=10, lr=1e-3, n=50),
    'multistep_default': dict(name='multistep', steps=(-1,), gamma=0.1, warmup_epochs=5, epochs=5, itrs_per_epoch=5, lr=1e-3, n=60),
    'cosine_warmup': dict(name='cosine', warmup_epochs=2, epochs=5, itrs_per_epoch=8, lr=1e-3, n=60),      # 16 + 40 = 56 < 60: past the end
    'cosine_plain': dict(name='cosine', warmup_epochs=0, epochs=4, itrs_per_epoch=11, lr=3e-4, n=44),
}


def write_npz(path, arrays):
    """np.savez_compressed with every member stamped 1980-01-01, members in the order given"""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    MG.install_stubs()
    from libs.modeling.model import PtTransformerEarlyFusionIterative
    from libs.modeling.optim import make_optimizer, make_scheduler

    models = {}
    for case in ('s1', 's2'):
        g = Golden(f'step_grad_{case}.npz')
        models[f'step_grad_{case}'] = (g.js('opt_kwargs'), g.js('meta')['second_fusion'])
    models['default'] = ({}, True)
    groups = {}
    for name, (kw, second) in models.items():
        torch.manual_seed(0)
        net = PtTransformerEarlyFusionIterative(MG.make_opt(**kw).clone(), second_fusion=second)
        names = {id(p): k for k, p in net.named_parameters()}
        opt = make_optimizer(net, dict(OPTIMIZER))
        assert len(opt.param_groups) == 2
        decay, no_decay = ([names[id(p)] for p in g['params']] for g in opt.param_groups)
        assert len(decay) + len(no_decay) == len(names) and decay == sorted(decay) and no_decay == sorted(no_decay)
        groups[name] = {'decay': decay, 'no_decay': no_decay, 'weight_decay': [g['weight_decay'] for g in opt.param_groups]}
        print(f'{name}: {len(decay)} decayed, {len(no_decay)} not')

    out = {'groups': groups, 'sched': SCHEDULES}
    for name, c in SCHEDULES.items():
        w = torch.nn.Parameter(torch.zeros(1))
        opt = torch.optim.AdamW([w], lr=c['lr'])
        sched = make_scheduler(opt, {k: v for k, v in c.items() if k not in ('lr', 'n')})
        lrs = []
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            for _ in range(c['n']):
                w.grad = torch.zeros(1)
                opt.step()
                sched.step()
                lrs.append(opt.param_groups[0]['lr'])
        out[f'lr/{name}'] = np.asarray(lrs, dtype=np.float64)
        print(f'{name}: lr {lrs[0]:.3e} ... {max(lrs):.3e} ... {lrs[-1]:.3e}')
    path = os.path.join(HERE, OUT)
    write_npz(path, MG.npify(out))
    print(f'{OUT}: {os.path.getsize(path) / 1024:.1f} KiB')


if __name__ == '__main__':
    main()
