"""CPU checks around the point objective (csrc/objective.hip): the ABI table, the configuration defaults, the refusal of point
tables the kernels cannot derive, and the self-consistency of tests/golden/objective.npz.  No GPU, no compute calls."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import Golden, ROOT, load_pkg
import objective_cases as C


def test_exports_are_in_the_ctypes_table_with_the_headers_arity():
    pkg = load_pkg()
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'decafnet_hip.h')).read(), flags=re.S)
    for name, arity in (('dcf_annotate_points', 15), ('dcf_point_objective', 24)):
        assert name in pkg._lib.SIGNATURES
        m = re.search(name + r'\s*\((.*?)\)\s*;', src, flags=re.S)
        assert m, name
        assert len(m.group(1).split(',')) == len(pkg._lib.SIGNATURES[name][1]) == arity
    eng = open(os.path.join(ROOT, 'cvpr2025-decafnet_amd', 'csrc', 'engine.hip')).read()
    assert re.search(r'dcf_abi_version\(void\)\s*\{\s*return 12;', eng)


def test_make_opt_carries_the_train_and_loss_defaults():
    """libs/core/opt.py:132-134, :147-157"""
    opt = load_pkg().config.make_opt()
    assert dict(opt.train) == dict(center_sampling='radius', center_sampling_radius=1.5, loss_norm=160, loss_norm_momentum=0.9,
                                   loss_weight=1.0, reg_loss='diou')
    assert dict(opt.loss) == dict(fc_a=0.5, fc_s=0.2)
    assert opt.pt_gen.regression_range == 4 and opt.pt_gen.sigma == 0.5             # no existing key changed


def test_point_layout_is_recovered_and_foreign_tables_are_refused():
    pkg = load_pkg()
    Ls = pkg.loss
    for uo in (False, True):
        pg = pkg.modeling.PtGenerator(2560, 4, 4, 0.5, use_offset=uo)
        pts = pg(C.level_sizes(256, 4))
        for form in (pts, torch.cat(pts)):
            T, L, (rr, sigma, msl), use_offset = Ls._point_layout(form)
            assert (T, L, rr, sigma, use_offset) == (256, 4, 4.0, 0.5, uo) and msl + 1 == 2561
        assert Ls.pt_gen_params(None, pg) == ((4.0, 0.5, 2560), uo)
    pts = torch.cat(pkg.modeling.PtGenerator(256, 4, 4, 0.5)(C.level_sizes(256, 4)))
    tgt = torch.tensor([[1.0, 2.0]])
    for spoil in ('coordinate', 'range', 'stride', 'length', 'shape'):
        bad = pts.clone()
        if spoil == 'coordinate':
            bad[17, 0] += 0.25
        elif spoil == 'range':
            bad[300:, 1] = 3.0
        elif spoil == 'stride':
            bad[256:384, 3] = 3.0
        elif spoil == 'length':
            bad = bad[:-1]
        else:
            bad = bad[:, :3]
        with pytest.raises(ValueError, match='PtGenerator'):
            Ls.annotate_points(bad, tgt)
    with pytest.raises(RuntimeError, match='MI355X'):            # a valid table, CPU targets: no CPU path
        Ls.annotate_points(pts, tgt)


def restated_labels(T, L, max_seq_len, rr, sigma, use_offset, target, mode, radius):
    """the rule of annotate_points_per_video (worker_v2.py:93-133) on PtGenerator's points (model.py:686-723), in numpy fp32"""
    f = np.float32
    ranges, cur = [(0, rr)], rr
    for l in range(1, L):
        lo, hi = cur * sigma, cur * 2
        if l == L - 1:
            hi = max(hi, max_seq_len + 1)
        ranges.append((lo, hi))
        cur = hi
    t0, t1 = f(target[0]), f(target[1])
    labels, wins, rngs = [], [], []
    for l in range(L):
        s = f(2 ** l)
        x = np.arange(T >> l, dtype=np.float32) * s + (s - f(0.5) if use_offset else f(0))      # in-place add on a view, model.py:710-712
        a, b = x - t0, t1 - x
        if mode == 'radius':
            ctr = f(0.5) * (t0 + t1)
            r = s * f(radius)
            win = (x - np.maximum(ctr - r, t0) > 0) & (np.minimum(ctr + r, t1) - x > 0)
        else:
            win = (a > 0) & (b > 0)
        d = np.maximum(a, b)
        rng = (d >= f(ranges[l][0])) & (d < f(ranges[l][1]))
        labels.append(win & rng), wins.append(win), rngs.append(rng)
    return tuple(np.concatenate(v) for v in (labels, wins, rngs))


def test_fixture_is_self_consistent():
    """guards the fixture, not the kernel: the restated rule reproduces the stored labels, and the counts are the ones the cases
    were chosen for"""
    g = Golden('objective.npz')
    for uo in (False, True):
        for bn, (targets, _) in C.SMALL_BATCHES.items():
            for mode in C.MODES:
                k = f'small/{bn}/{mode}/uo{int(uo)}'
                for b, t in enumerate(targets):
                    lab, win, rng = restated_labels(C.SMALL['T'], C.SMALL['L'], C.SMALL['max_seq_len'], C.SMALL['regression_range'],
                                                    C.SMALL['sigma'], uo, t, mode, C.RADIUS)
                    assert np.array_equal(lab, g.t(f'{k}/labels')[b].numpy()), (k, b)
                    assert np.array_equal(win, g.t(f'{k}/in_window')[b].numpy()) and np.array_equal(rng, g.t(f'{k}/in_range')[b].numpy())
        S = sum(C.level_sizes(C.BENCH['T'], C.BENCH['L']))
        for mode in C.MODES:
            idx = g.t(f'bench/{mode}/uo{int(uo)}/label_idx')
            want = torch.zeros(len(C.BENCH_TARGETS), S, dtype=torch.bool)
            want[idx[:, 0], idx[:, 1]] = True
            for b, t in enumerate(C.BENCH_TARGETS):
                lab, _, _ = restated_labels(C.BENCH['T'], C.BENCH['L'], C.BENCH['max_seq_len'], C.BENCH['regression_range'], C.BENCH['sigma'],
                                            uo, t, mode, C.RADIUS)
                assert np.array_equal(lab, want[b].numpy()), (mode, uo, b)
    sc, bc = g.js('small/counts'), g.js('bench/counts')
    assert sc['a/radius'] == [[5, 0, 3], [5, 0, 0]] and sc['a/none'] == [[6, 0, 5], [6, 0, 0]]
    assert sc['b/radius'] == [[3, 3], [3, 3]] and sc['b/none'] == [[20, 31], [20, 31]]
    assert sc['z/radius'] == [[0, 0, 0], [0, 0, 0]] and sc['z/none'] == [[0, 0, 0], [0, 0, 0]]
    assert bc['radius'] == [[4, 3, 8, 4], [4, 3, 5, 0]] and bc['none'] == [[4, 70, 8, 4], [4, 70, 5, 0]]
    assert float(g.t('bench/radius/trainer32')[3]) == 12 and float(g.t('bench/none/trainer32')[3]) == 79
    for mode in C.MODES:                                          # the empty-selection batch: reg exactly 0, norm 0
        tr = g.t(f'small/z/{mode}/trainer')
        assert bool((tr[:, 1] == 0).all()) and bool((tr[:, 3] == 0).all())
    # the bench-scale inputs regenerate to what the fixture was computed from (masks by valid length, a stable seed)
    _, _, off, msk, _ = C.bench_inputs()
    assert msk.sum(1).tolist() == [sum(-(-v // 2 ** l) for l in range(C.BENCH['L'])) for v in C.BENCH_VALID] and float(off.min()) >= 0
