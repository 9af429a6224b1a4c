"""One rank of the two-rank checks of tests/test_gpu_dp_step.py; started by the test as a fresh process, never imported.

    RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT in the environment;  python dp_rank_main.py <backend> <out_dir> [bucket_bytes]

backend gloo: every rank on cuda:0 (the flow check of a one-GPU box); nccl: rank r on cuda:r.  Rank r takes video r of fixture s1.
Rank 1 perturbs its parameters BEFORE it constructs the step, so that what the construction broadcasts shows.  Three steps of
``train.DataParallelTrainStep`` (warmup_epochs = 0); after each one the state (``state_of``), every ``p.grad`` and the returned grad_norm
are kept, and all of it is written to <out_dir>/rank<r>.pt."""
import datetime
import os
import sys

import torch
import torch.distributed as dist

STEPS = 3


def main():
    backend, out_dir = sys.argv[1], sys.argv[2]
    bucket_bytes = int(sys.argv[3]) if len(sys.argv) > 3 else None
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    device = 0 if backend == 'gloo' else rank
    kw = {} if backend == 'gloo' else {'device_id': torch.device('cuda', device)}
    dist.init_process_group(backend, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120), **kw)
    torch.cuda.set_device(device)
    from conftest import load_pkg
    from test_gpu_train_step import batch_of, fixture, opt_of, state_of
    pkg = load_pkg()
    f = fixture('s1')
    model = f.model(pkg).cuda()
    if rank == 1:
        with torch.no_grad():
            for p in model.parameters():
                p.add_(0.03125)
    opt = opt_of(pkg, f)
    opt.train.warmup_epochs = 0
    kw = {} if bucket_bytes is None else {'bucket_bytes': bucket_bytes}
    ts = pkg.train.DataParallelTrainStep(model, opt, itrs_per_epoch=1, process_group=dist.group.WORLD, **kw)
    assert ts.world == world == ts.objective.world_size
    batch, targets = batch_of(f, [rank])
    steps = []
    for _ in range(STEPS):
        out = ts.step(batch, targets)
        steps.append({'state': state_of(ts), 'grads': [p.grad.detach().cpu().clone() for p in model.parameters()],
                      'out': {k: v.detach().cpu().clone() for k, v in out.items()}, 'launched': list(ts.reducer.launched),
                      'loss_norm': ts.objective.loss_norm})
    torch.save({'steps': steps, 'buckets': len(ts.reducer.plan['buckets']), 'uploads': ts.optimizer.table_uploads}, os.path.join(out_dir, f'rank{rank}.pt'))
    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
