"""The one-kernel head (csrc/head_chain.hip) with its output convolution as the chain's last matrix-core product (f16x3 on the image
of launch_split_chain_out) instead of fp32 FMAs: through dcf_op_head(..., chain = 1) at the shapes of
test_gpu_ops.test_head_chain_vs_fp64 and one that ends exactly on a window, both widths, one and two outputs, with and without
Scale + ReLU, inside that test's bounds (3e-5 against fp64, 2e-5 against the GEMM launches); nothing written beyond the output;
ten repeats bit-identical; and one forward through the benchmark in child processes.  GPU only."""
import ctypes
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, load_pkg

pytestmark = pytest.mark.gpu

# (B, T): (5, 64): three windows of 122 rows, sequences shorter than a window, a window straddling sequence ends; (2, 333): ragged
# last window; (1, 4000): 33 windows; (1, 366): ends exactly on a window
SHAPES = [(5, 64), (3, 100), (2, 333), (1, 4000), (1, 122 * 3)]
# (C, NO, scale): scale = 0 raw logits (mode 0), otherwise relu(scale * y) (mode 1)
HEADS = [(256, 1, 0.0), (288, 2, 1.7), (288, 1, 0.0), (256, 2, 0.6)]


@pytest.fixture(scope='module')
def L():
    pkg = load_pkg()
    return pkg, pkg._lib.lib()          # raises if the .so is missing: no silent fallback


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def problem(B, T, C, NO, scale):
    """inputs (CPU) as test_head_chain_vs_fp64 builds them (ragged masks with a hole at row 17) and the fp64 reference, once per case"""
    g = torch.Generator().manual_seed(B * 1000 + T + C + NO)
    X = torch.randn(B * T, C, generator=g)
    mask = torch.ones(B, T, dtype=torch.bool)
    for b in range(B):
        n = int(torch.randint(T // 2, T + 1, (1,), generator=g))
        mask[b, n:] = False
        if T > 40:
            mask[b, 17] = False
    t = dict(X=X, mask=mask.to(torch.uint8),
             W1=torch.randn(C, C, 3, generator=g) / math.sqrt(3 * C), W2=torch.randn(C, C, 3, generator=g) / math.sqrt(3 * C),
             l1w=torch.rand(C, generator=g) + 0.5, l1b=torch.randn(C, generator=g) * 0.3,
             l2w=torch.rand(C, generator=g) + 0.5, l2b=torch.randn(C, generator=g) * 0.3,
             Wo=torch.randn(NO, C, 3, generator=g) / math.sqrt(3 * C), bo=torch.randn(NO, generator=g))
    mf = mask[:, None, :].double()
    x = X.double().view(B, T, C).transpose(1, 2)

    def ln(v, w, b):
        mu = v.mean(1, keepdim=True)
        return (v - mu) / torch.sqrt(((v - mu) ** 2).mean(1, keepdim=True) + 1e-5) * w.double()[None, :, None] + b.double()[None, :, None]

    y = torch.relu(ln(F.conv1d(x * mf, t['W1'].double(), padding=1), t['l1w'], t['l1b']))
    y = torch.relu(ln(F.conv1d(y * mf, t['W2'].double(), padding=1), t['l2w'], t['l2b']))
    o = F.conv1d(y * mf, t['Wo'].double(), t['bo'].double(), padding=1)
    if scale != 0.0:
        o = torch.relu(o * scale)
    return t, mask.view(-1), o.transpose(1, 2).reshape(B * T, NO)


def run_head(L, d, B, T, C, NO, scale, chain):
    """-> (B * T + 1, NO): the last row keeps its NaN fill"""
    pkg, lib = L
    out = torch.full((B * T + 1, NO), float('nan'), device='cuda')
    pkg._lib.check(lib.dcf_op_head(P(d['X']), P(d['mask']), P(d['W1']), P(d['l1w']), P(d['l1b']), P(d['W2']), P(d['l2w']), P(d['l2b']),
                                   P(d['Wo']), P(d['bo']), P(out), B, T, C, NO, scale, chain, st()), 'dcf_op_head')
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('C,NO,scale', HEADS)
@pytest.mark.parametrize('B,T', SHAPES)
def test_head_with_matrix_core_output_convolution(L, B, T, C, NO, scale):
    t, valid, ref = problem(B, T, C, NO, scale)
    d = {k: v.cuda() for k, v in t.items()}
    outs = {}
    for chain in (1, 0):
        oc = run_head(L, d, B, T, C, NO, scale, chain).cpu()
        assert torch.isnan(oc[B * T]).all(), 'wrote beyond the last row'
        assert torch.isfinite(oc[:B * T]).all()
        print(f'B {B} T {T} C {C} NO {NO} scale {scale} chain {chain}: max abs error vs fp64 {(oc[:B * T][valid].double() - ref[valid]).abs().max():.3e}')
        torch.testing.assert_close(oc[:B * T][valid].double(), ref[valid], rtol=3e-5, atol=3e-5)
        outs[chain] = oc[:B * T]
    torch.testing.assert_close(outs[1][valid], outs[0][valid], rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize('B,T,C,NO,scale', [(2, 333, 288, 2, 1.7), (5, 64, 256, 1, 0.0)])
def test_ten_repeats_are_bit_identical(L, B, T, C, NO, scale):
    t, _, _ = problem(B, T, C, NO, scale)
    d = {k: v.cuda() for k, v in t.items()}
    first = run_head(L, d, B, T, C, NO, scale, 1)[:B * T].view(torch.int32).clone()
    for rep in range(1, 10):
        cur = run_head(L, d, B, T, C, NO, scale, 1)[:B * T].view(torch.int32)
        assert torch.equal(first, cur), f'repeat {rep} differs from the first run'


def test_forward_with_one_kernel_heads_against_the_launches(tmp_path):
    """End to end: the benchmark's forward_videos at T = 2048 (two videos per forward: 8 160 pyramid rows, query-major outputs, both
    modes, the pair grid) in child processes; one lowers DCF_HEAD_CHAIN_MIN_ROWS in its environment so that the heads run as one
    kernel each, the other keeps the GEMM / LayerNorm / output-convolution launches.  Bound: the 2e-4 on logits and offsets that the
    sharded forward is held to against the unsharded one (test_gpu_e2e.test_two_rank_sharded_forward_on_one_gpu); masks equal."""
    T = 2048
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1', '--T', str(T), '--videos', '2',
           '--batch', '2', '--min-timed-s', '0', '--full', '--no-cpu-baseline', '--no-post']
    for name, extra in (('chain', {'DCF_HEAD_CHAIN_MIN_ROWS': '4000'}), ('launches', {})):
        env = dict({k: v for k, v in os.environ.items() if k not in ('DCF_HEAD_CHAIN_MIN_ROWS', 'DCF_NO_HEAD_CHAIN')},
                   PYTHONDONTWRITEBYTECODE='1', **extra)
        r = subprocess.run(cmd + ['--dump-outputs', str(tmp_path / name)], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        res = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][-1])
        assert any('head_chain' in k for k in res['stages']) == (name == 'chain'), sorted(res['stages'])
    a, b = np.load(tmp_path / 'chain' / 'masks.npy'), np.load(tmp_path / 'launches' / 'masks.npy')
    assert np.array_equal(a, b)
    for k in ('logits', 'offsets'):
        a, b = np.load(tmp_path / 'chain' / f'{k}.npy'), np.load(tmp_path / 'launches' / f'{k}.npy')
        assert a.shape == b.shape and np.isfinite(a).all() and np.isfinite(b).all()
        print(f'{k}: max abs difference one-kernel heads vs launches {np.abs(a - b).max():.3e}')
        assert np.abs(a - b).max() < 2e-4, k
