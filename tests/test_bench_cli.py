"""bench.py's command line and its --dump-outputs writer, on the CPU: a plain run times exactly --steps steps and leaves the
other measurements to --full; the dump holds every video of a step in float32, within its size budget."""
import importlib.util
import os
import sys

import numpy as np
import torch

from conftest import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location('bench_for_tests', os.path.join(ROOT, 'bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                       # module level defines functions only (main() is behind __name__)
    return mod


def _fake_step(nv, nq, sizes, seed):
    """per video what forward(..., eval=True) returns: per query, per level (1, n) logits, (1, n, 2) offsets, (1, n) bool masks"""
    g = torch.Generator().manual_seed(seed)
    vids = []
    for _ in range(nv):
        lg = [tuple(torch.randn(1, n, generator=g) for n in sizes) for _ in range(nq)]
        of = [tuple(torch.randn(1, n, 2, generator=g) for n in sizes) for _ in range(nq)]
        mk = [tuple(torch.rand(1, n, generator=g) > 0.3 for n in sizes) for _ in range(nq)]
        vids.append((lg, of, mk))
    return vids


def test_plain_run_defaults(monkeypatch):
    bench = _bench()
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--steps', '7', '--warmup', '2'])
    a = bench.parse()
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    assert a.min_timed_s == 0, 'a plain run must time exactly --steps steps'
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--full', '--dump-outputs', 'out_dir'])
    a = bench.parse()
    assert a.full and a.dump_outputs == 'out_dir'


def test_dump_outputs_layout(tmp_path):
    bench = _bench()
    sizes = [16, 8, 4, 2]
    vids = _fake_step(3, 2, sizes, 5)
    info = bench.dump_outputs(str(tmp_path), vids)
    assert info['files'] == ['logits.npy', 'masks.npy', 'offsets.npy'] and info['sampled_points'] is None
    lg, of, mk = (np.load(tmp_path / f'{k}.npy') for k in ('logits', 'offsets', 'masks'))
    assert lg.shape == (3, 2, 30) and of.shape == (3, 2, 30, 2) and mk.shape == (3, 2, 30)
    assert lg.dtype == of.dtype == mk.dtype == np.float32
    for v in range(3):
        for q in range(2):
            np.testing.assert_array_equal(lg[v, q], torch.cat(vids[v][0][q], 1)[0].numpy())
            np.testing.assert_array_equal(of[v, q], torch.cat(vids[v][1][q], 1)[0].numpy())
            np.testing.assert_array_equal(mk[v, q], torch.cat(vids[v][2][q], 1)[0].float().numpy())


def test_dump_outputs_sample_within_budget(tmp_path, monkeypatch):
    bench = _bench()
    sizes = [512, 256, 128]
    vids = _fake_step(2, 3, sizes, 6)
    S = sum(sizes)
    full = 2 * 3 * S * 4 * 4                           # logits + 2 offsets + masks, float32
    monkeypatch.setattr(bench, 'DUMP_BUDGET_BYTES', full // 3)
    infos = [bench.dump_outputs(str(tmp_path / d), vids) for d in ('a', 'b')]
    assert infos[0] == infos[1] and infos[0]['sampled_points'] and 'points.npy' in infos[0]['files']
    for d in ('a', 'b'):
        assert sum(os.path.getsize(tmp_path / d / f) - 128 for f in infos[0]['files']) <= full // 3   # .npy header: 128 bytes
    pts = np.load(tmp_path / 'a' / 'points.npy')
    assert pts.dtype == np.float64 and np.all(np.diff(pts) > 0) and pts[-1] < S
    idx = pts.astype(np.int64)
    lg = np.load(tmp_path / 'a' / 'logits.npy')
    assert lg.shape == (2, 3, len(idx))
    np.testing.assert_array_equal(lg[1, 2], torch.cat(vids[1][0][2], 1)[0].numpy()[idx])
    for f in infos[0]['files']:                        # a fixed sample: the same bytes on every run
        assert (tmp_path / 'a' / f).read_bytes() == (tmp_path / 'b' / f).read_bytes()
