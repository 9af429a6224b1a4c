"""CPU checks that go with the step-guard extension (include/decafnet_hip_guard.h; its header and table: tests/test_abi_headers.py): the
names of ``_lib.GUARD_SIGNATURES``, the verdict values and ``_lib.DcfGuardState`` against the header; the restatement
of the verdict rule (tests/guard_ref.py) on NaN, +-inf, an overflowing square and a NO_GRAD row; and what ``train.TrainStep`` makes of
``skip_nonfinite`` without a GPU.  No GPU."""
import ctypes
import re

import numpy as np
import pytest
import torch

import abi_headers as H
from conftest import load_pkg
import guard_ref as G

NAMES = ['dcf_guard_adam_step', 'dcf_guard_arm', 'dcf_guard_disarm', 'dcf_guard_ext_version', 'dcf_guard_grad_norm']
# ---------------------------------------------------------------------------------------------- the ABI
def test_guard_table_names_verdicts_and_source():
    pkg = load_pkg()
    assert sorted(pkg._lib.GUARD_SIGNATURES) == NAMES
    src = H.source_of('decafnet_hip_guard.h')
    assert f'#define DCF_GUARD_APPLY {pkg._lib.GUARD_APPLY}' in src and f'#define DCF_GUARD_SKIP {pkg._lib.GUARD_SKIP}' in src
    assert 'optim_guard.hip' in pkg.build.SOURCES


def test_guard_state_record_equals_the_header():
    """field by field, in order; 48 bytes with every 64-bit counter on an 8-byte boundary; the host's numpy record is the same"""
    pkg = load_pkg()
    body = re.search(r'typedef\s+struct\s+dcf_guard_state\s*\{(.*?)\}\s*dcf_guard_state\s*;', H.source_of('decafnet_hip_guard.h'), flags=re.S).group(1)
    fields = [tuple(d.split()) for d in body.split(';') if d.strip()]
    S = pkg._lib.DcfGuardState
    assert [(n, H.SCALARS[t]) for t, n in fields] == [(n, t) for n, t in S._fields_]
    assert ctypes.sizeof(S) == 48 == pkg.optim._GUARD.itemsize
    for n, t in S._fields_:
        off = getattr(S, n).offset
        assert off == pkg.optim._GUARD.fields[n][1] and off % ctypes.sizeof(t) == 0, n
    assert {n for n, _ in S._fields_} - {'reserved0', 'reserved1'} == set(G.FIELDS)


# ---------------------------------------------------------------------------------------------- the restatement
def _table(seed=3):
    """five rows: 3, 4097, 0, 5 (NO_GRAD) and 8200 finite elements"""
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(n).astype(np.float32), flag) for n, flag in ((3, 0), (4097, 0), (0, 0), (5, 1), (8200, 0))]


@pytest.mark.parametrize('value', [float('nan'), float('inf'), -float('inf'), 1e20, -1e20], ids=['nan', '+inf', '-inf', '1e20', '-1e20'])
def test_one_bad_value_makes_its_row_bad(value):
    for row, at in ((0, 0), (1, 4096), (4, 8199), (4, 4095)):
        table = _table()
        table[row][0][at] = value
        assert G.bad_rows(table) == [row]
        chunks = G.bad_chunks(table[row][0])
        assert chunks == [c == at // G.CHUNK for c in range(len(chunks))]
        st = G.judge(table, G.fresh_state(applied=7, skipped=2))
        assert st == dict(verdict=1, first_bad_row=row, n_bad_rows=1, applied=7, skipped=3, last_skipped_attempt=9, conv_flag=0)


def test_the_square_overflows_where_the_value_is_finite():
    """|g| = 1e20 is a finite fp32 whose square is not: the row is bad; 1e19 squares to 1e38 and stays; sixteen of them in one lane
    (elements 4 t + j + 1024 s of a chunk) add up past the largest fp32 and do not"""
    with np.errstate(over='ignore'):
        assert np.isfinite(np.float32(1e20)) and not np.isfinite(np.float32(1e20) * np.float32(1e20))
    g = np.zeros(4096, dtype=np.float32)
    g[17] = 1e19
    assert G.bad_rows([(g, 0)]) == []
    g[[1024 * s + 4 * 4 + j for s in range(4) for j in range(4)]] = 1e19         # lane 4 holds element 17
    assert G.bad_rows([(g, 0)]) == [0]
    g = np.zeros(4096, dtype=np.float32)
    g[0:64:4] = 1e19                                                             # sixteen, in sixteen lanes: fp64 adds them
    assert G.bad_rows([(g, 0)]) == []


def test_rows_without_a_gradient_are_ignored_and_counters_run():
    table = _table()
    table[3][0][2] = float('nan')                                                # the NO_GRAD row
    assert G.bad_rows(table) == [] and G.bad_rows([(None, 0)]) == []
    st = G.judge(table, G.fresh_state())
    assert st == dict(verdict=0, first_bad_row=-1, n_bad_rows=0, applied=1, skipped=0, last_skipped_attempt=-1, conv_flag=0)
    table[4][0][5000] = float('inf')
    table[1][0][0] = float('nan')
    st = G.judge(table, st)
    assert st == dict(verdict=1, first_bad_row=1, n_bad_rows=2, applied=1, skipped=1, last_skipped_attempt=1, conv_flag=0)
    st = G.judge(_table(), st)                                                   # finite again: the last skip stays on record
    assert st == dict(verdict=0, first_bad_row=1, n_bad_rows=2, applied=2, skipped=1, last_skipped_attempt=1, conv_flag=0)
    st = G.judge(_table(), st, conv_word=1)                                      # the armed conv-gradient word alone
    assert st == dict(verdict=1, first_bad_row=-1, n_bad_rows=0, applied=2, skipped=2, last_skipped_attempt=3, conv_flag=1)


# ---------------------------------------------------------------------------------------------- the host layer without a GPU
def _step_on_the_cpu(**kw):
    import step_grad_ref as S
    pkg = load_pkg()
    f = S.Fixture('s1')
    ts = pkg.train.TrainStep(f.model(pkg), f.opt(pkg), itrs_per_epoch=1, **kw)
    batch = dict(vid=f.vid, shallow=f.shallow, vid_masks=f.vid_masks, tokens=S.tm(f.tokens), text_cls=f.text_cls, token_masks=f.token_masks,
                 text_size=f.text_size)
    return pkg, ts, batch, f.targets


@pytest.mark.parametrize('skip', [False, True])
def test_a_step_on_cpu_tensors_reaches_the_gpu_error_with_and_without_the_guard(skip):
    pkg, ts, batch, targets = _step_on_the_cpu(skip_nonfinite=skip)
    assert ts.skip_nonfinite is skip and ts.guard is None
    with pytest.raises(RuntimeError, match='GPU') as e:
        ts.step(batch, targets)
    assert 'MI355X only' in str(e.value)
    assert ('guard' in ts.state()[1]) == skip
    if skip:
        assert ts.state()[1]['guard'] == {'applied': 0, 'skipped': 0}


@pytest.mark.parametrize('value', [1, 0, None, 'yes'])
def test_a_skip_nonfinite_that_is_no_bool_is_refused(value):
    pkg = load_pkg()
    with pytest.raises(ValueError, match='skip_nonfinite'):
        pkg.train.TrainStep(None, None, skip_nonfinite=value)
    with pytest.raises(ValueError, match='skip_nonfinite'):
        pkg.train.DataParallelTrainStep(None, None, skip_nonfinite=value)


def test_a_guard_on_the_cpu_is_refused():
    pkg = load_pkg()
    with pytest.raises(RuntimeError, match='GPU only'):
        pkg.optim.StepGuard('cpu')
    p = torch.nn.Parameter(torch.zeros(3))
    p.grad = torch.zeros(3)
    with pytest.raises(RuntimeError, match='GPU only'):
        pkg.optim.grad_norm_and_coef([p], 1.0)
