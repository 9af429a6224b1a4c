"""The verdict rule of the step guard (include/decafnet_hip_guard.h, csrc/optim_guard.hip) restated on the CPU in numpy, for
tests/test_guard_cpu.py and the GPU tests of the extension.

A table is a list of ``(g, no_grad)``: ``g`` a float32 array (or None for g == NULL), ``no_grad`` the DCF_OPTIM_NO_GRAD flag.  A row
is bad if one of its chunks of 4096 elements has a non-finite partial.  A chunk's partial is the fp64 sum of 256 fp32 lane sums; lane t
adds the squares of the elements [1024 s + 4 t, + 4), s = 0 .. 3, in that order with one rounding per element.  fp64 cannot overflow on
256 finite fp32 values, so the partial is non-finite exactly when a lane sum is: an element is NaN or +-inf, or the lane's running sum
of squares passes the largest fp32 (one element of 1e20 does).  Rows with ``no_grad`` or ``g is None`` are never read.

``judge`` advances a state record exactly as the final pass of dcf_guard_grad_norm does: ``verdict`` describes this call, ``applied``
/ ``skipped`` count, and ``first_bad_row`` / ``n_bad_rows`` / ``conv_flag`` / ``last_skipped_attempt`` describe the last SKIPPED attempt
and keep their values through applied ones."""
import numpy as np

CHUNK, NT, VEC = 4096, 256, 4
SWEEPS = CHUNK // (NT * VEC)
FIELDS = ('verdict', 'first_bad_row', 'n_bad_rows', 'applied', 'skipped', 'last_skipped_attempt', 'conv_flag')


def fresh_state(applied=0, skipped=0):
    return dict(verdict=0, first_bad_row=-1, n_bad_rows=0, applied=applied, skipped=skipped, last_skipped_attempt=-1, conv_flag=0)


def lane_sums(chunk):
    """the 256 fp32 lane sums of one chunk (at most 4096 float32 values; what is missing counts as 0)"""
    x = np.zeros(CHUNK, dtype=np.float32)
    x[:len(chunk)] = chunk
    x = x.reshape(SWEEPS, NT, VEC).astype(np.float64)
    acc = np.zeros(NT, dtype=np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        for s in range(SWEEPS):
            for j in range(VEC):
                acc = (acc.astype(np.float64) + x[s, :, j] * x[s, :, j]).astype(np.float32)      # fma: the product is exact in fp64
    return acc


def bad_chunks(g):
    g = np.asarray(g, dtype=np.float32).reshape(-1)
    return [not bool(np.isfinite(lane_sums(g[c:c + CHUNK])).all()) for c in range(0, len(g), CHUNK)]


def bad_rows(table):
    return [r for r, (g, no_grad) in enumerate(table) if not no_grad and g is not None and any(bad_chunks(g))]


def judge(table, state, conv_word=0):
    """-> the state after one dcf_guard_grad_norm over `table` with the armed conv-gradient word `conv_word` (0: clear or not armed)"""
    new, bad = dict(state), bad_rows(table)
    skip = bool(bad) or conv_word != 0
    new['verdict'] = int(skip)
    if skip:
        new.update(first_bad_row=bad[0] if bad else -1, n_bad_rows=len(bad), conv_flag=int(conv_word),
                   last_skipped_attempt=state['applied'] + state['skipped'], skipped=state['skipped'] + 1)
    else:
        new['applied'] = state['applied'] + 1
    return new
