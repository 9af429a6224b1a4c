"""dcf_op_loss_table_mean (include/decafnet_hip_fit.h) restated in numpy on the CPU, in the operator's documented order: the fp32
divisions one at a time, the per-video sums in query order, the sum over the videos lane-strided and then as a halving tree, every
float64 operation a Python float operation (IEEE, rounded on its own).  What the operator is compared with on the GPU
(tests/test_gpu_loss_table.py), and what tests/test_fit_cpu.py compares with ``evaluator.calc_loss``'s filtering.  The synthetic tables
of both live here too."""
import numpy as np

LANES = 256
QNAN64 = np.array([0x7ff8000000000000], dtype=np.uint64).view(np.float64)[0]


def per_query(rows):
    """rows (N, 4) fp32 -> (N, 2) float64: cls = focal2 / max(n_pos, 1), reg = iou / max(n_pos, 1), each one fp32 division"""
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, 4)
    n_pos = rows[:, 3]
    norm = np.where(n_pos < np.float32(1), np.float32(1), n_pos)                  # a NaN stays, as in torch.clamp(min=1)
    with np.errstate(all='ignore'):
        return np.stack((rows[:, 1] / norm, rows[:, 2] / norm), 1).astype(np.float32).astype(np.float64)


def per_video(values, offsets):
    """values (N, 2) float64, offsets (V + 1) -> (V, 2) float64: the mean, in query order, of the values that are not NaN"""
    V = len(offsets) - 1
    out = np.empty((V, 2), dtype=np.float64)
    for v in range(V):
        for k in range(2):
            s, n = 0.0, 0
            for q in range(int(offsets[v]), int(offsets[v + 1])):
                x = float(values[q, k])
                if x == x:
                    s, n = s + x, n + 1
            out[v, k] = s / n if n else QNAN64
    return out


def over_videos(pv):
    """(V, 2) float64 -> (2,) float64: lane t adds the videos t, t + 256, ...; then h = 128 ... 1: a[t] += a[t + h]; then / V"""
    V = len(pv)
    out = np.empty(2, dtype=np.float64)
    with np.errstate(all='ignore'):
        for k in range(2):
            a = [0.0] * LANES
            for v in range(V):
                a[v % LANES] = a[v % LANES] + float(pv[v, k])
            h = LANES // 2
            while h >= 1:
                for t in range(h):
                    a[t] = a[t] + a[t + h]
                h //= 2
            out[k] = np.float64(a[0]) / np.float64(V)
    return out


def loss_table_mean(rows, offsets):
    """-> (per_video (V, 2), out2 (2,)) float64"""
    pv = per_video(per_query(rows), offsets)
    return pv, over_videos(pv)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def numpy_mean_of_means(rows, offsets):
    """np.mean of np.means, numpy's own summation order: for tables without NaN, inf or an empty video"""
    values = per_query(rows)
    return np.mean(np.stack([np.mean(values[int(offsets[v]):int(offsets[v + 1])], axis=0) for v in range(len(offsets) - 1)]), axis=0)


# ---------------------------------------------------------------------------------------------- synthetic tables
def table(counts, seed, special=True):
    """-> (rows (N, 4) fp32, offsets (V + 1) int64) of non-negative losses for videos of ``counts`` queries.  ``special``: a row
    with n_pos = 0, an inf row, a NaN row inside a video (where a video has two rows) and a video whose rows are all NaN (where there
    are two videos); a single video of one query gets one of the four by ``seed`` % 4."""
    g = np.random.default_rng(seed)
    counts = [int(c) for c in counts]
    offsets = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    N, V = int(offsets[-1]), len(counts)
    rows = np.empty((N, 4), dtype=np.float32)
    rows[:, 0] = g.uniform(0, 90, N)
    rows[:, 1] = g.uniform(0, 60, N)
    rows[:, 2] = g.uniform(0, 12, N)
    rows[:, 3] = g.integers(1, 24, N)
    if not special:
        return rows, offsets
    if N == 1:
        kind = seed % 4
        if kind == 0:
            rows[0, 3] = 0
        elif kind == 1:
            rows[0, 1:3] = np.nan
        elif kind == 2:
            rows[0, 2] = np.inf
        else:
            rows[0, 1], rows[0, 3] = np.nan, np.nan                                # a NaN n_pos: both losses NaN
        return rows, offsets
    order = sorted(range(V), key=lambda v: (-counts[v], v))
    big = order[0]                                                                 # the longest video: NaN inside it, n_pos = 0
    rows[offsets[big], 3] = 0
    if counts[big] >= 2:
        rows[offsets[big] + 1, 1:3] = np.nan
    if counts[big] >= 3:
        rows[offsets[big] + 2, 1] = np.nan                                         # NaN in one key only: the counts of the keys differ
    if V >= 2:
        dead = order[-1]                                                           # the shortest video: all of its rows NaN
        rows[offsets[dead]:offsets[dead + 1], 1:3] = np.nan
    if V >= 3:
        rows[offsets[order[1]], 2] = np.inf
    for v in range(7, V, 61):                                                      # more of each kind further on
        q = int(offsets[v])
        rows[q, 1 + v % 2] = (np.nan, np.inf, 0.0)[v % 3]
        rows[q, 3] = v % 2
    return rows, offsets


def counts_for(V, seed):
    """1 to 5 queries per video"""
    return np.random.default_rng(seed).integers(1, 6, V).tolist()
