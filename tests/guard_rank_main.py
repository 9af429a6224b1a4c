"""One rank of the two-rank check of tests/test_gpu_guard_step.py; started by the test as a fresh process.  The set-up is that of
tests/dp_rank_main.py (imported for its step count; same environment variables and arguments):

    RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT in the environment;  python guard_rank_main.py gloo <out_dir>

Both ranks on cuda:0; rank r takes video r of fixture s1.  Three steps of ``train.DataParallelTrainStep(..., skip_nonfinite=True)``
(warmup_epochs = 0); at the second step rank 1 ALONE gets a batch with one NaN in one clip's expert feature.  After each step the state
(``state_of``), the returned grad_norm and ``guard.report(names)`` are kept -- host reads, outside the step -- and all of it is written
to <out_dir>/rank<r>.pt."""
import datetime
import os
import sys

import torch
import torch.distributed as dist

import dp_rank_main


def main():
    backend, out_dir = sys.argv[1], sys.argv[2]
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    assert backend == 'gloo'
    dist.init_process_group(backend, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    torch.cuda.set_device(0)
    from conftest import load_pkg
    from test_gpu_train_step import batch_of, fixture, opt_of, state_of
    pkg = load_pkg()
    f = fixture('s1')
    model = f.model(pkg).cuda()
    opt = opt_of(pkg, f)
    opt.train.warmup_epochs = 0
    ts = pkg.train.DataParallelTrainStep(model, opt, itrs_per_epoch=1, process_group=dist.group.WORLD, skip_nonfinite=True)
    assert ts.world == world and ts.guard is not None
    names = [n for n, _ in model.named_parameters()]
    batch, targets = batch_of(f, [rank])
    bad = dict(batch, vid=batch['vid'].clone())
    bad['vid'][0, 3, 5] = float('nan')
    steps, conv_flag_seen = [], False
    for k in range(dp_rank_main.STEPS):
        out = ts.step(bad if (k == 1 and rank == 1) else batch, targets)
        report = ts.guard.report(names)
        conv_flag_seen |= bool(report['conv_flag']) and report['verdict'] == 1
        report.pop('conv_flag')                                     # rank-local by design: kept apart from what the ranks must share
        steps.append({'state': state_of(ts), 'grad_norm': out['grad_norm'].detach().cpu().clone(), 'report': report})
    torch.save({'steps': steps, 'names': names, 'conv_flag_seen': conv_flag_seen}, os.path.join(out_dir, f'rank{rank}.pt'))
    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
