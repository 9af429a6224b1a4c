"""One rank of the two-rank checks of tests/test_gpu_fit_parallel.py; started by the test as a fresh process.

    RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT in the environment;  python fit_rank_main.py gloo <out_dir> <tree_root>

Both ranks on cuda:0, the set-up of tests/fit_setup.py on the tree the parent wrote (6 videos: two steps of two samples per rank and
epoch).  Three scenarios in sequence; what the parent compares goes to <out_dir>/rank<r>.pt.

(a) ``fit_parallel`` over two epochs with ``eval_run=1, val_loss=True`` into <out_dir>/a: the tensors, the results, every ``torch.save``
    call and every file this rank opened for writing, the videos this rank evaluated at each evaluation, the reduced loss row table.
(b) one epoch into <out_dir>/b, then fresh objects with ``resume=True`` up to two epochs: the tensors and the results.
(c) three steps of ``DataParallelTrainStep(skip_nonfinite=True, agree_skips=<True, then False>)``; at step 1 rank 1 ALONE raises the
    conv-gradient word after its real backward (a wrapped ``_backward`` runs dcf_op_conv_bwd_weight on scratch tensors with an inf in
    dY): the real gradients stay finite.  The tensors and ``guard.report()`` after every step.  A numerics flag, not a fault."""
import datetime
import os
import sys

import torch
import torch.distributed as dist


def main():
    backend, out_dir, tree = sys.argv[1], sys.argv[2], sys.argv[3]
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    assert backend == 'gloo' and world == 2
    dist.init_process_group(backend, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    torch.cuda.set_device(0)
    from conftest import load_pkg
    import fit_setup as S
    import step_grad_ref as R
    pkg = load_pkg()
    T, E = pkg.train, pkg.evaluator
    f = R.Fixture('s2')
    cfg, ed, bank = S.open_world(pkg, f, tree, S.N_VIDEOS_TWO_RANKS)

    def make(**kw):
        return S.make_step(pkg, f, cfg, rank, world, cls=T.DataParallelTrainStep, process_group=dist.group.WORLD, **kw)

    # ---- what this rank saves, writes and evaluates -------------------------------------------------------------------------------
    log = {'saves': [], 'writes': [], 'evaluated': [], 'rows': []}
    real_save, real_item, real_losses = torch.save, bank.item, E.DeviceLossMeter.losses

    def save(obj, path, *a, **k):
        log['saves'].append(str(path))
        return real_save(obj, path, *a, **k)

    def open_(path, mode='r', *a, **k):
        if any(c in mode for c in 'wax+'):
            log['writes'].append(str(path))
        return open(path, mode, *a, **k)

    def item(vid_id):
        log['evaluated'][-1].append(vid_id)
        return real_item(vid_id)

    def losses(self, *a, **k):
        log['rows'].append(self.rows.cpu().clone())                  # after the all-reduce: the table of the whole set
        return real_losses(self, *a, **k)

    real_evaluate = T.evaluate

    def evaluate(*a, **k):
        log['evaluated'].append([])
        return real_evaluate(*a, **k)

    torch.save, T.open, bank.item, E.DeviceLossMeter.losses, T.evaluate = save, open_, item, losses, evaluate
    kw = dict(eval_data=bank, eval_by='epoch', eval_run=1, val_loss=True)

    # ---- (a) ----------------------------------------------------------------------------------------------------------------------
    ts, loader = make()
    assert ts.world == 2 and (loader.rank, loader.world_size) == (rank, 2)
    res_a = T.fit_parallel(ts, loader, os.path.join(out_dir, 'a'), num_epochs=2, **kw)
    a = {'tensors': S.tensors(ts), 'results': [tuple(r) for r in res_a], 'epoch_itr': (ts.epoch, ts.itr), 'log': {k: list(v) for k, v in log.items()}}
    assert all(isinstance(r, T.EvalResult) for r in res_a)

    # ---- (b) ----------------------------------------------------------------------------------------------------------------------
    ts, loader = make()
    first = T.fit_parallel(ts, loader, os.path.join(out_dir, 'b'), num_epochs=1, **kw)
    assert ts.epoch == 1
    ts, loader = make()                                              # fresh objects: everything comes from the two last.pth files
    second = T.fit_parallel(ts, loader, os.path.join(out_dir, 'b'), num_epochs=2, resume=True, **kw)
    b = {'tensors': S.tensors(ts), 'results': [tuple(r) for r in first + second], 'epoch_itr': (ts.epoch, ts.itr)}
    torch.save, E.DeviceLossMeter.losses, T.evaluate = real_save, real_losses, real_evaluate
    del T.open, bank.item

    # ---- (c) ----------------------------------------------------------------------------------------------------------------------
    L = pkg._lib
    X, dY, dW = torch.randn(64, 32).cuda(), torch.randn(64, 32).cuda(), torch.empty(32, 1, 32, device='cuda')
    dY[7, 3] = float('inf')

    def three_steps(agree):
        ts, loader = make(skip_nonfinite=True, agree_skips=agree)
        batches = list(loader.epoch(0)) + list(loader.epoch(1))[:1]
        step = [0]
        backward = ts._backward

        def wrapped(total, last):
            backward(total, last)
            if last and rank == 1 and step[0] == 1:                  # the word alone: no gradient of the model is touched
                L.check(L.lib().dcf_op_conv_bwd_weight(L.ptr(X), None, L.ptr(dY), L.ptr(dW), None, 1, 64, 32, 32, 1, 0, L.current_stream()),
                        'dcf_op_conv_bwd_weight')

        ts._backward = wrapped
        rows = []
        for k, (batch, targets) in enumerate(batches):
            step[0] = k
            out = ts.step(batch, targets)
            finite = all(bool(torch.isfinite(p.grad).all()) for p in ts.model.parameters())
            rows.append({'tensors': S.tensors(ts), 'report': ts.guard.report(), 'grad_norm': out['grad_norm'].detach().cpu().clone(),
                         'finite_grads': finite})
        return rows

    c = {'agree': three_steps(True), 'alone': three_steps(False)}
    torch.save({'a': a, 'b': b, 'c': c, 'remote': L.GUARD_REMOTE}, os.path.join(out_dir, f'rank{rank}.pt'))
    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
