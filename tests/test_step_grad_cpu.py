"""CPU checks of the whole-step fixtures tests/golden/step_grad_<case>*.npz (make_golden_step_grad.py): the conditions their generator
asserts on the reference alone, asserted again on the committed files, because tests/test_gpu_step_grad.py takes its bound from them.
No GPU.

    every file is below the 1 MiB limit of a committed file
    the fixture holds a gradient for every parameter of the package's model of that configuration, by name, and n_params of them
    e_ref = max |g_32 - g_64| <= 2^-15 max |g_64| for every parameter outside the exactly-zero ones (key.bias, k_norm.bias, whose
        scale is that of the same layer's weight): no ReLU, max-pool or top-k decision differs between the two precisions
    the discrete decisions: the oracle's gate in fp32 and in fp64 gives the recorded gate weights and the recorded mask after the gate;
        the masks of the levels are that mask at the levels' strides; the labels and target offsets are those of the point rule
    no positive point is a non-smooth point of the IoU loss, in either precision, and every level has a positive point
    the recorded fp64 total is the objective of the recorded fp64 outputs
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_pkg
import objective_cases as C
import objective_grad_ref as OR
import step_grad_ref as R

LIMIT = 1 << 20
E_REF_CAP = 2.0 ** -15


@pytest.fixture(scope='module', params=R.CASES)
def f(request):
    return R.Fixture(request.param)


def test_files_are_below_the_limit(f):
    for suffix in R.FILES:
        path = os.path.join(GOLDEN, f'step_grad_{f.name}{suffix}.npz')
        assert 0 < os.path.getsize(path) < LIMIT, path


def test_every_parameter_of_the_model_has_a_recorded_gradient(f):
    model = f.model(load_pkg())
    names = [k for k, _ in model.named_parameters()]
    assert len(names) == f.meta['n_params'] == 252
    assert sorted(names) == sorted(f.gp['32']) == sorted(f.gp['64']) and len(set(names)) == len(names)      # (the files group them by module)
    for k, p in model.named_parameters():
        assert f.gp['32'][k].dtype == torch.float32 and f.gp['64'][k].dtype == torch.float64
        assert f.gp['32'][k].shape == f.gp['64'][k].shape == p.shape, k
        assert torch.equal(p.detach(), f.sd[k]) and torch.equal(p.detach() * 1024, torch.round(p.detach() * 1024)), k
    assert model.second_fusion == (f.name == 's2') and model.msf == (f.name == 's2') and model.vid_net.stride == (2 if f.name == 's2' else 1)


def test_reference_error_is_under_the_cap(f):
    worst, zero = 0.0, 0
    for k, g64 in f.gp['64'].items():
        top, e_ref = f.top(k), float((f.gp['32'][k].double() - g64).abs().max())
        assert top > 0 and bool(torch.isfinite(g64).all()), k
        if k.endswith(R.ZERO_BY_SYMMETRY):
            zero += 1
            assert float(g64.abs().max()) <= 1e-10 * top, k              # rounding noise around 0
            continue
        assert float(g64.abs().max()) == top
        assert e_ref <= E_REF_CAP * top, (k, e_ref, top)
        worst = max(worst, e_ref / top)
    print(f'{f.name}: worst e_ref / max|g64| {worst:.3e}, {zero} gradients that are zero in exact arithmetic')
    assert zero > 0
    for t in R.GTAPS:
        g64 = f.gtaps['64'][t]
        assert float((f.gtaps['32'][t].double() - g64).abs().max()) <= E_REF_CAP * float(g64.abs().max()), t
    for scale in ('reg_head.scales.0.scale', 'reg_head.scales.1.scale', 'reg_head.scales.2.scale'):
        assert float(f.gp['64'][scale].abs().max()) > 0, scale


def test_discrete_decisions(f):
    meta, kw = f.meta, f.opt_kwargs
    for dt in (torch.float32, torch.float64):
        gate, mask = f.oracle_gate(dt)
        assert torch.equal(gate, f.gate) and torch.equal(mask, f.mask_gated), dt
    rows = f.vid_masks.repeat_interleave(torch.tensor(f.text_size), 0)
    assert bool((f.gate & ~rows).sum() == 0) and 0 < int(f.gate.sum()) < int(rows.sum())
    assert torch.equal(f.mask_gated, rows if kw['msf'] else rows & f.gate)
    if not kw['msf']:                                                  # holes: an invalid position with valid ones on both sides
        m = f.mask_gated
        assert any(bool(m[b, :t].any()) and bool(m[b, t + 1:].any()) for b in range(m.size(0)) for t in range(m.size(1)) if not m[b, t])
    stride = kw['vid_stride']
    for l, m in enumerate(f.masks):
        assert torch.equal(m, f.mask_gated[:, ::stride << l]), l
    T0 = meta['T'] // stride
    assert meta['level_lengths'] == [T0 >> l for l in range(f.L)]
    labels, gt = OR.annotate(T0, f.L, kw['max_seq_len'], 4, 0.5, f.targets.tolist(), meta['center_sampling'], C.RADIUS)
    assert torch.equal(labels, f.labels) and torch.equal(gt, f.gt_offsets)


def test_positive_points(f):
    msk = torch.cat(f.masks, 1)
    pos = f.labels & msk
    lv = np.cumsum([0] + f.meta['level_lengths'])
    per_level = [int(pos[:, lv[l]:lv[l + 1]].sum()) for l in range(f.L)]
    assert per_level == f.meta['positive_per_level'] and min(per_level) >= 1
    for t in ('32', '64'):
        off = torch.cat(f.out[t]['offsets'], 1)
        assert int((OR.non_smooth(off, f.gt_offsets) & pos).sum()) == 0 == f.meta['excluded'], t


def test_total_is_the_objective_of_the_recorded_outputs(f):
    msk = torch.cat(f.masks, 1)
    for t, dt, tol in (('64', torch.float64, 1e-13), ('32', torch.float32, 2.0 ** -20)):
        l1, l2, off = (torch.cat(f.out[t][k], 1) for k in ('logits1', 'logits2', 'offsets'))
        assert l1.dtype == dt and f.total[t].dtype == dt
        total = OR.objective_value(l1, l2, off, msk, f.labels, f.gt_offsets, f.meta['reg_loss'], f.meta['loss_norm'], 1, 1.0, C.FC_A, C.FC_S)
        assert abs(float(total) - float(f.total[t])) <= tol * abs(float(total)), t
    assert abs(float(f.total['32']) - float(f.total['64'])) <= 2.0 ** -20 * float(f.total['64'])
