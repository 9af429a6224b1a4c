"""The bias corrections of the step-count extension (include/decafnet_hip_clock.h, csrc/optim_clock.hip) restated on the CPU, for
tests/test_clock_cpu.py and the GPU tests of the extension.

``corrections(b1, b2, t)`` is the pair the host path passes by value for the count t (``optim.AdamW._group_array``): 1 - b1^t and
sqrt(1 - b2^t) in double, rounded to fp32.  ``from_table(table, t)`` is what dcf_clock_adam_step reads for the count t from a table
whose entry t - 1 belongs to t: the entry, or (1, 1) past the end.  ``table_length(b1, b2)`` walks the counts until both floats are 1."""
import math

import numpy as np

MAX_TABLE = 1 << 22


def corrections(b1, b2, t):
    return np.float32(1.0 - b1 ** t), np.float32(math.sqrt(1.0 - b2 ** t))


def from_table(table, t):
    if 1 <= t <= len(table):
        return np.float32(table[t - 1][0]), np.float32(table[t - 1][1])
    return np.float32(1.0), np.float32(1.0)


def table_length(b1, b2):
    t = 1
    while corrections(b1, b2, t) != (np.float32(1.0), np.float32(1.0)):
        t += 1
    return t
