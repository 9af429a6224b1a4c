"""CPU checks that go with the step-count extension (include/decafnet_hip_clock.h; its header and table: tests/test_abi_headers.py): the
names of ``_lib.CLOCK_SIGNATURES`` and the parameter order of dcf_clock_adam_step; the host's bias-correction tables
(``optim.bias_correction_table``) entry by entry against the pair the host path passes by value (tests/clock_ref.py); and what
``optim.AdamW`` and ``train.TrainStep`` make of ``device_count`` without a GPU.  No GPU."""
import copy
import math

import numpy as np
import pytest
import torch

import abi_headers as H
from conftest import load_pkg
import clock_ref as C

NAMES = ['dcf_clock_adam_step', 'dcf_clock_ext_version']
# ---------------------------------------------------------------------------------------------- the ABI
def test_clock_table_names_parameter_order_and_source():
    pkg = load_pkg()
    assert sorted(pkg._lib.CLOCK_SIGNATURES) == NAMES
    assert H.param_names('decafnet_hip_clock.h', 'dcf_clock_adam_step') == [
        'table', 'chunk_map', 'n_tensors', 'n_chunks', 'groups', 'n_groups', 'bc_tables', 'bc_len', 'steps', 'coef', 'guard_state', 'with_ema',
        'ema_beta', 'stream']
    assert 'optim_clock.hip' in pkg.build.SOURCES


# ---------------------------------------------------------------------------------------------- the table builder
@pytest.mark.parametrize('betas', [(0.9, 0.999), (0.0, 0.5), (0.95, 0.9999)], ids=str)
def test_every_entry_is_the_pair_the_host_path_passes(betas):
    pkg = load_pkg()
    b1, b2 = betas
    table = pkg.optim.bias_correction_table(b1, b2)
    assert table.dtype == np.float32 and table.ndim == 2 and table.shape[1] == 2 and table.flags['C_CONTIGUOUS']
    assert len(table) == C.table_length(b1, b2) <= pkg._lib.CLOCK_MAX_TABLE == C.MAX_TABLE
    h = pkg._lib.DcfOptimGroup()
    for t in range(1, len(table) + 1):
        want = C.corrections(b1, b2, t)
        got = (table[t - 1, 0], table[t - 1, 1])
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), (t, got, want)
        if t < 64 or t % 997 == 0:                        # and the float a C assignment makes of the same double, as _group_array does
            h.bc1, h.sqrt_bc2 = 1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t)
            assert (np.float32(h.bc1), np.float32(h.sqrt_bc2)) == want, t
    ones = (np.float32(1.0), np.float32(1.0))
    assert tuple(table[-1]) == ones and all(tuple(row) != ones for row in table[:-1]), 'the last entry is the first that is (1, 1)'
    assert C.from_table(table, len(table) + 1) == ones == C.corrections(b1, b2, len(table) + 1)
    assert C.from_table(table, 100000000) == ones == C.corrections(b1, b2, 100000000)


def test_a_zero_beta_gives_one_entry_and_a_beta_too_close_to_one_is_refused():
    pkg = load_pkg()
    assert pkg.optim.bias_correction_table(0.0, 0.0).tolist() == [[1.0, 1.0]]
    assert len(pkg.optim.bias_correction_table(0.0, 0.5)) == C.table_length(0.0, 0.5) > 1
    with pytest.raises(ValueError, match='4194304'):
        pkg.optim.bias_correction_table(0.9, 0.9999999)
    with pytest.raises(ValueError, match='4194304'):
        pkg.optim.bias_correction_table(0.999999, 0.999)         # 25 ln 2 / 1e-6 = 17 M entries; 0.99999 (1.7 M) would fit
    with pytest.raises(ValueError, match=r'\[0, 1\)'):
        pkg.optim.bias_correction_table(1.0, 0.5)
    assert len(pkg.optim.bias_correction_table(0.5, 0.5, max_len=64)) == C.table_length(0.5, 0.5) <= 64
    with pytest.raises(ValueError, match='more than 8 steps'):
        pkg.optim.bias_correction_table(0.5, 0.5, max_len=8)


# ---------------------------------------------------------------------------------------------- the host layer without a GPU
@pytest.mark.parametrize('value', [1, 0, None, 'yes'])
def test_a_device_count_that_is_no_bool_is_refused(value):
    pkg = load_pkg()
    with pytest.raises(ValueError, match='device_count'):
        pkg.train.TrainStep(None, None, device_count=value)
    with pytest.raises(ValueError, match='device_count'):
        pkg.train.DataParallelTrainStep(None, None, device_count=value)
    with pytest.raises(ValueError, match='device_count'):
        pkg.optim.AdamW([torch.nn.Parameter(torch.zeros(3))], device_count=value)


def test_a_step_on_cpu_tensors_reaches_the_gpu_error():
    pkg = load_pkg()
    ps = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))]
    for p in ps:
        p.grad = torch.ones_like(p)
    opt = pkg.optim.AdamW(ps, device_count=True)
    assert opt.device_count is True and pkg.optim.AdamW(ps).device_count is False
    with pytest.raises(RuntimeError, match='GPU only'):
        opt.step()
    assert opt._steps is None and not opt.state, 'nothing was laid out or initialised'


@pytest.mark.parametrize('skip', [False, True])
def test_a_train_step_on_cpu_tensors_reaches_the_gpu_error(skip):
    from test_guard_cpu import _step_on_the_cpu
    pkg, ts, batch, targets = _step_on_the_cpu(skip_nonfinite=skip, device_count=True)
    assert ts.device_count is True and ts.optimizer.device_count is True
    with pytest.raises(RuntimeError, match='GPU') as e:
        ts.step(batch, targets)
    assert 'MI355X only' in str(e.value)
    assert sorted(ts.state()[1]) == sorted(['optimizer', 'scheduler', 'epoch', 'itr', 'loss_norm'] + (['guard'] if skip else []))


def test_a_state_dict_moves_between_the_settings_without_a_gpu():
    """torch.optim.AdamW -> device_count=True -> device_count=False -> torch, on CPU tensors: the counts wait on the host until the
    first step on the GPU lays them out"""
    from test_optim_cpu import same_state, toy
    g = torch.Generator().manual_seed(6)
    pkg = load_pkg()
    ps = toy()
    ref = torch.optim.AdamW([{'params': ps[:2], 'weight_decay': 0.05}, {'params': ps[2:], 'weight_decay': 0.0}], lr=2e-3)
    for _ in range(2):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g)
        ref.step()
    sd = ref.state_dict()
    on = pkg.optim.AdamW([{'params': toy()[:2]}, {'params': toy()[2:]}], device_count=True)
    on.load_state_dict(copy.deepcopy(sd))
    assert on._steps is None and sorted(on._host_counts.values()) == [2, 2, 2]
    same_state(on.state_dict(), sd)
    off = pkg.optim.AdamW([{'params': toy()[:2]}, {'params': toy()[2:]}])
    off.load_state_dict(copy.deepcopy(on.state_dict()))
    same_state(off.state_dict(), sd)
    assert all(isinstance(st['step'], float) and st['step'] == 2.0 for st in off.state.values())
