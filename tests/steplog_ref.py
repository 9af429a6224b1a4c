"""The numpy / Python restatement of dcf_op_steplog_add and dcf_op_steplog_flush (include/decafnet_hip_steplog.h) for
tests/test_steplog_cpu.py, tests/steplog_abi_cases.py and tests/test_gpu_steplog.py: the tables as the header lays them out, every
addition and division one IEEE double operation (numpy's float64 scalars), the tie rule of min / max and the flush of an empty table.

``stats`` is (K, 6) float64 -- sum, finite_sum, min, max, last, reserved -- and ``counts`` (K + 1) int64, both all zero when empty."""
import numpy as np

COLS = 6
SUM, FINITE_SUM, MIN, MAX, LAST, RESERVED = range(COLS)
QNAN = np.array([0x7ff8000000000000], dtype=np.uint64).view(np.float64)[0]

# the values a meter has to survive: NaN, both infinities, both zeros, denormals, and the largest finite floats twice (their sum is
# finite in double and overflows fp32)
SPECIAL = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45, -1e-40, 3.4e38, 3.4e38, 0.1, -2.5], dtype=np.float32)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def word(v):
    """the bits of one float64 as an int"""
    return int(bits(v).reshape(-1)[0])


def canon(v):
    """every NaN is the one quiet NaN: IEEE 754 leaves sign and payload of a NaN that an operation makes to the implementation (x86
    makes inf + -inf a negative NaN), and the header says which one the tables hold"""
    return QNAN if v != v else v


def empty(K):
    return np.zeros((K, COLS), dtype=np.float64), np.zeros(K + 1, dtype=np.int64)


def add(stats, counts, vals):
    """one step: ``vals`` (K) float32 into the tables, in place"""
    K = len(vals)
    assert stats.shape == (K, COLS) and counts.shape == (K + 1,) and np.asarray(vals).dtype == np.float32
    with np.errstate(all='ignore'):
        for k in range(K):
            v = canon(np.float64(vals[k]))                                     # exact
            stats[k, SUM] = canon(stats[k, SUM] + v)
            stats[k, LAST] = v
            if np.isfinite(v):
                stats[k, FINITE_SUM] = stats[k, FINITE_SUM] + v
                if counts[k] == 0 or v < stats[k, MIN]:
                    stats[k, MIN] = v
                if counts[k] == 0 or v > stats[k, MAX]:
                    stats[k, MAX] = v
                counts[k] += 1
    counts[K] += 1


def flush(stats, counts):
    """-> out (K + 1, 6); the tables are reset in place (the reserved column keeps its bits)"""
    K = stats.shape[0]
    steps = int(counts[K])
    out = np.zeros((K + 1, COLS), dtype=np.float64)
    with np.errstate(all='ignore'):
        for k in range(K):
            n = int(counts[k])
            out[k, 0] = canon(stats[k, SUM] / np.float64(steps)) if steps else 0.0
            out[k, 1] = stats[k, FINITE_SUM] / np.float64(n) if n else QNAN
            out[k, 2] = stats[k, MIN] if n else QNAN
            out[k, 3] = stats[k, MAX] if n else QNAN
            out[k, 4] = stats[k, LAST]
            out[k, 5] = np.float64(n)
    out[K, 0] = np.float64(steps)
    stats[:, :RESERVED] = 0.0
    counts[:] = 0
    return out


def random_vals(K, seed):
    """a plain step: K losses of a plausible size"""
    return (np.random.default_rng(seed).random(K) * 4.0 + 0.01).astype(np.float32)


def special_vals(K, shift):
    """K of the special values, starting at ``shift``"""
    return SPECIAL[(np.arange(K) + shift) % len(SPECIAL)].copy()


def tables_after(K, n_steps, seed):
    """the tables after ``n_steps`` earlier steps: plain and special vectors in turn, so that every column has been through both"""
    stats, counts = empty(K)
    for i in range(n_steps):
        add(stats, counts, special_vals(K, i) if i % 2 else random_vals(K, seed + i))
    return stats, counts
