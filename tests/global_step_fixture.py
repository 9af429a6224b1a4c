"""The reader of case g1 of the whole training step, tests/golden/step_grad_global*.npz (make_golden_global_attn_grad.py: E = 64 on 2
heads with mha_win_size = 0 -- global attention in the stem and in every pyramid level -- 3 levels, vid_stride 1, no msf, T = 80 with
lengths 80 / 55, two videos, three queries, text_size [2, 1]).  It is step_grad_ref.Fixture, unchanged, on the core file merged with
the files that hold the state dict (at E = 64 the state dict does not fit one committed file beside the rest)."""
import glob
import os

import numpy as np

import step_grad_ref as S
from conftest import GOLDEN, Golden

NAME = 'global'


class _Merged:
    def __init__(self, paths):
        self.parts = [np.load(p) for p in paths]
        self.files = [k for z in self.parts for k in z.files]
        assert len(set(self.files)) == len(self.files)

    def __getitem__(self, k):
        return next(z for z in self.parts if k in z.files)[k]


class _Golden(Golden):
    def __init__(self, name):
        if name == f'step_grad_{NAME}.npz':
            self.z = _Merged([os.path.join(GOLDEN, name)] + param_files())
        else:
            super().__init__(name)


def param_files():
    return sorted(glob.glob(os.path.join(GOLDEN, f'step_grad_{NAME}_params_*.npz')))


def files():
    """every committed file of the case"""
    return sorted(glob.glob(os.path.join(GOLDEN, f'step_grad_{NAME}*.npz')))


_cache = []


def fixture():
    if not _cache:
        keep = S.Golden
        S.Golden = _Golden
        try:
            _cache.append(S.Fixture(NAME))
        finally:
            S.Golden = keep
    return _cache[0]
