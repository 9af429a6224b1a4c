"""Cases of the point-objective fixture (tests/golden/objective.npz), shared by its generator (tests/golden/make_golden_objective.py)
and the tests: the target batches, the option grid and the bench-scale inputs, which are regenerated from a seed instead of
being committed."""
import torch

# ---- small: the outputs of tests/golden/train.npz (T = 256, L = 4, 3 (video, query) rows, the second video valid to 201)
SMALL = dict(T=256, L=4, max_seq_len=256, regression_range=4, sigma=0.5)
SMALL_BATCHES = {
    'a': ([[10.3, 14.9], [100.25, 100.75], [210.0, 250.0]], [0, 1, 2]),      # targets, rows of train.npz
    'b': ([[40.0, 200.5], [0.0, 256.0]], [0, 1]),
    'z': ([[100.25, 100.75]] * 3, [0, 1, 2]),                                # no positive point at all
}
MODES = {'radius': ('radius', 'diou'), 'none': ('none', 'giou')}             # center_sampling -> reg_loss it is paired with
RADIUS = 1.5
FC_A, FC_S = 0.5, 0.2
GRID = [(ln, ws, lw) for ln in (160.0, 7.5) for ws in (1, 4) for lw in (1.0, 0.25)]    # loss_norm, world_size, loss_weight

# ---- bench scale
BENCH = dict(T=16384, L=8, max_seq_len=16384, regression_range=4, sigma=0.5)
BENCH_VALID = [16384, 16384, 12000, 9001]
BENCH_TARGETS = [[5000.2, 5007.9], [100.0, 9000.0], [11900.0, 12040.0], [16000.0, 16383.5]]
BENCH_SEED = 20251


def level_sizes(T, L):
    return [T >> l for l in range(L)]


def bench_inputs(rows=None):
    """logits1, logits2 (n, S), offsets (n, S, 2) >= 0, masks (n, S) of the bench-scale case, on the CPU from BENCH_SEED; level l of
    row b is valid where mask_b[::2**l] is.  ``rows``: repeat the 4 rows cyclically to that many (timing)."""
    T, L = BENCH['T'], BENCH['L']
    S = sum(level_sizes(T, L))
    g = torch.Generator().manual_seed(BENCH_SEED)
    n = len(BENCH_VALID)
    logits1 = torch.randn(n, S, generator=g) * 2.0 - 2.0
    logits2 = torch.randn(n, S, generator=g) * 2.0 - 2.0
    offsets = torch.rand(n, S, 2, generator=g) * 6.0
    masks = torch.zeros(n, S, dtype=torch.bool)
    for b, v in enumerate(BENCH_VALID):
        m = torch.arange(T) < v
        masks[b] = torch.cat([m[::2 ** l] for l in range(L)])
    targets = torch.tensor(BENCH_TARGETS, dtype=torch.float32)
    if rows is not None:
        idx = torch.arange(rows) % n
        logits1, logits2, offsets, masks, targets = (x[idx].contiguous() for x in (logits1, logits2, offsets, masks, targets))
    return logits1, logits2, offsets, masks, targets
