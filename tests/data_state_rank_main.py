"""One rank of the two-rank check of tests/test_steplog_cpu.py; started by the test as a fresh process, on the CPU.

    python data_state_rank_main.py <rank> <world> <dir>

The ranks meet over gloo through a file under <dir>.  Each owns a stub loader whose state is seeded by its rank; the states are
gathered to rank 0 as ``fit_parallel(..., data_state=True)`` gathers them, written, and read back by every rank into a second stub.
What the parent checks goes to <dir>/rank<r>.ok."""
import datetime
import os
import random
import sys

import numpy as np
import torch.distributed as dist


class Loader:
    def __init__(self, seed):
        self.seed, self.loaded = seed, None

    def state(self):
        return {'rng': {'random': random.Random(self.seed).getstate(), 'numpy': np.random.RandomState(self.seed).get_state()}}

    def load_state(self, state):
        self.loaded = state


def key(state):
    r, n = state['rng']['random'], state['rng']['numpy']
    return r, n[0], n[1].tobytes(), tuple(n[2:])


def main():
    rank, world, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    dist.init_process_group('gloo', init_method=f'file://{os.path.join(out, "store")}', rank=rank, world_size=world,
                            timeout=datetime.timedelta(seconds=60))
    from conftest import load_pkg
    T = load_pkg().train
    root = os.path.join(out, 'run')
    states = T._gather_data_states(Loader(10 + rank), rank, world, None)
    assert (states is None) == (rank != 0)
    if rank == 0:
        assert [key(s) for s in states] == [key(Loader(10 + r).state()) for r in range(world)]
        T._checkpoint_data(root, states)
    dist.barrier()
    fresh = Loader(99)
    T._resume_data(fresh, root, rank, world)
    assert key(fresh.loaded) == key(Loader(10 + rank).state()), 'every rank reads its own entry'
    try:
        T._resume_data(Loader(99), root, 0, world + 1)
    except ValueError as e:
        assert f'{world} ranks' in str(e)
    else:
        raise AssertionError('another world size must be refused')
    dist.barrier()
    dist.destroy_process_group()
    with open(os.path.join(out, f'rank{rank}.ok'), 'w') as fh:
        fh.write('ok')


if __name__ == '__main__':
    main()
