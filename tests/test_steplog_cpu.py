"""CPU checks that go with the training log (include/decafnet_hip_steplog.h, csrc/steplog.hip, ``train.StepLog``) and with the data
loader's resumable random streams.

1. The declared boundary of the ``_lib.STEPLOG`` record: the table equals the header (tests/abi_headers.check_table), the built
   library exports the declared symbols and the version is 1, the source is part of the build, no name is shared with another table,
   ``EXTENSIONS`` / ``PENDING`` / ``STAGED`` / ``FIT`` are what they were, and hipcc compiles the source without a warning.
2. The restatement of tests/steplog_ref.py: ``sum`` and ``mean`` against a literal ``AverageMeter`` (libs/train_utils.py) written out
   here, bit for bit, on sequences with NaN, both infinities, both zeros, denormals and 3.4e38 twice; the tie rule; the empty flush.
3. The line: the width of the iteration field, the key order, the three ranges of ``time_str``.
4. The refusals of ``fit`` / ``fit_parallel`` / ``StepLog`` on stub objects: nothing is opened.
5. ``TrainLoader.state()`` / ``load_state()`` on the generated tree with ``crop_ratio=(0.5, 1.0)``: decisions, not tensors; and the
   file of ``data_state=True`` over two gloo ranks on the CPU (tests/data_state_rank_main.py): one entry per rank, gathered to rank 0."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import abi_headers as H
import steplog_ref as R
import train_data_tree as TT
from conftest import load_pkg


# ---------------------------------------------------------------------------------------------- 1. the boundary
def test_steplog_record_equals_its_header_and_the_library():
    pkg = load_pkg()
    L = pkg._lib
    assert len(L.STEPLOG) == 1
    ext = L.STEPLOG[0]
    assert ext == L.Extension('steplog', 'decafnet_hip_steplog.h', 'dcf_steplog_ext_version', 1, 'DCF_STEPLOG_EXT_VERSION',
                              ('decafnet_hip.h',), L.STEPLOG_TABLE)
    H.check_table(ext)
    assert sorted(ext.table) == ['dcf_op_steplog_add', 'dcf_op_steplog_flush', 'dcf_steplog_ext_version']
    assert 'steplog.hip' in pkg.build.SOURCES
    h = ctypes.CDLL(pkg.build.build())
    for s in H.declared_symbols(ext.header):
        assert hasattr(h, s), f'{s} declared in include/{ext.header} but not exported'
    assert h.dcf_steplog_ext_version() == 1
    src = H.source_of(ext.header)
    for macro, value in (('DCF_STEPLOG_MAX_KEYS', L.STEPLOG_MAX_KEYS), ('DCF_STEPLOG_COLS', L.STEPLOG_COLS)):
        m = [line for line in src.splitlines() if line.startswith(f'#define {macro} ')]
        assert m and int(m[0].split()[-1], 0) == value, macro
    assert L.STEPLOG_COLS == R.COLS == len(pkg.train.LOG_STATS)


def test_source_compiles_without_warnings_under_the_project_flags(tmp_path):
    b = load_pkg().build
    cmd = [b.hipcc()] + b.FLAGS + b.EXTRA.get('steplog.hip', []) + ['-c', os.path.join(b.CSRC, 'steplog.hip'), '-o', str(tmp_path / 'steplog.o')]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0 and 'warning' not in r.stderr and 'warning' not in r.stdout, r.stderr


def test_the_other_records_are_unchanged_and_share_no_name():
    L = load_pkg()._lib
    assert [e.key for e in L.EXTENSIONS] == ['base', 'train', 'dist', 'attn', 'front', 'guard', 'clock', 'half', 'front_half', 'embd']
    assert [e.key for e in L.PENDING] == ['batch'] and [e.key for e in L.STAGED] == ['eval'] and [e.key for e in L.FIT] == ['fit']
    assert sorted(L.FIT_TABLE) == ['dcf_fit_ext_version', 'dcf_guard_word_merge', 'dcf_guard_word_publish', 'dcf_op_loss_table_mean']
    assert not [n for n in dir(L) if n.endswith('SIGNATURES') and getattr(L, n) is L.STEPLOG_TABLE]
    others = L.EXTENSIONS + L.PENDING + L.STAGED + L.FIT
    assert not {name for e in others for name in e.table} & set(L.STEPLOG_TABLE)
    assert L.STEPLOG[0].key not in {e.key for e in others} and L.STEPLOG[0].header not in {e.header for e in others}
    for e in others:
        assert not set(H.declared_symbols(e.header)) & set(L.STEPLOG_TABLE), e.header


# ---------------------------------------------------------------------------------------------- 2. the restatement
class AverageMeter:
    """libs/train_utils.py:34-53, written out"""

    def __init__(self):
        self.reset()

    def reset(self):
        self.val = 0
        self.sum = 0
        self.mean = 0
        self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.mean = self.sum / self.count

    def item(self):
        return self.mean


def _sequences():
    g = np.random.default_rng(0)
    plain = (g.random(40) * 3.0).astype(np.float32)
    big = np.array([3.4e38, 3.4e38, 1.0], dtype=np.float32)                     # the sum overflows fp32 and is finite in double
    tiny = np.array([1e-45, -1e-40, 1e-45, 2e-39, -0.0, 0.0], dtype=np.float32)
    mixed = np.concatenate([plain[:5], R.SPECIAL, plain[5:9]])
    zeros = np.array([-0.0, -0.0, 0.0], dtype=np.float32)
    return {'plain': plain, 'big': big, 'tiny': tiny, 'mixed': mixed, 'special': R.SPECIAL, 'zeros': zeros, 'one-nan': np.array([np.nan], np.float32),
            'inf-then-minus-inf': np.array([np.inf, -np.inf, 1.0], dtype=np.float32)}


@pytest.mark.parametrize('name', sorted(_sequences()))
def test_sum_and_mean_are_the_average_meters(name):
    """Bit for bit, with every NaN counted as the one quiet NaN of the header: the sign of the NaN that inf + -inf makes is the
    processor's choice (IEEE 754-2008 6.2.1), negative on x86, and the tables name theirs."""
    seq = _sequences()[name]
    meter = AverageMeter()
    stats, counts = R.empty(1)
    with np.errstate(all='ignore'):
        for i, v in enumerate(seq):
            meter.update(float(v))                                                # what v.detach().item() hands the reference
            R.add(stats, counts, seq[i:i + 1])
            assert R.bits(stats[0, R.SUM]) == R.bits(R.canon(np.float64(meter.sum))), (name, i)
            assert R.bits(stats[0, R.LAST]) == R.bits(R.canon(np.float64(meter.val))) and counts[1] == meter.count == i + 1
    if name == 'big':
        assert np.isfinite(stats[0, R.SUM]) and stats[0, R.SUM] > np.finfo(np.float32).max
    finite = seq[np.isfinite(seq)].astype(np.float64)
    out = R.flush(stats, counts)
    assert R.bits(out[0, 0]) == R.bits(R.canon(np.float64(meter.item()))), 'the mean'
    assert out[1, 0] == len(seq) and out[0, 5] == len(finite) and not out[1, 1:].any()
    if len(finite):
        assert out[0, 2] == finite.min() and out[0, 3] == finite.max()
        want = np.float64(0.0)
        for v in finite:
            want = want + v
        assert R.bits(out[0, 1]) == R.bits(want / np.float64(len(finite)))
    else:
        assert [int(b) for b in R.bits(out[0, 1:4])] == [0x7ff8000000000000] * 3
    meter.reset()                                                                 # Trainer.log resets after every line
    assert not stats.any() and not counts.any() and meter.sum == 0 and meter.count == 0


def test_the_first_value_wins_a_tie_and_the_empty_flush():
    for first, second in ((-0.0, 0.0), (0.0, -0.0)):
        stats, counts = R.empty(1)
        R.add(stats, counts, np.array([first], dtype=np.float32))
        R.add(stats, counts, np.array([second], dtype=np.float32))
        want = R.word(first)
        assert R.word(stats[0, R.MIN]) == want and R.word(stats[0, R.MAX]) == want
        assert R.word(stats[0, R.LAST]) == R.word(second)
    stats, counts = R.empty(3)
    stats[:, R.RESERVED] = 7.0
    out = R.flush(stats, counts)
    assert out.shape == (4, 6) and not out[:, 0].any() and not out[3].any() and not out[:3, 4:].any(), 'mean 0.0 as AverageMeter.reset leaves it'
    assert (R.bits(out[:3, 1:4]) == 0x7ff8000000000000).all() and (stats[:, R.RESERVED] == 7.0).all()
    R.add(stats, counts, np.array([np.nan, np.inf, 2.0], dtype=np.float32))       # a NaN poisons sum and mean, not the finite columns
    out = R.flush(stats, counts)
    assert np.isnan(out[0, 0]) and out[1, 0] == np.inf and out[2, 0] == 2.0 and out[:3, 5].tolist() == [0.0, 0.0, 1.0]
    assert np.isnan(out[0, 4]) and out[1, 4] == np.inf and np.isnan(out[1, 1]) and out[2, 1:4].tolist() == [2.0, 2.0, 2.0]


# ---------------------------------------------------------------------------------------------- 3. the line
def test_the_line_on_fixed_numbers():
    T = load_pkg().train
    assert T.log_line(7, 1200, ('cls', 'reg', 'total'), (0.12345, 1.0, 1.12355), 0.26) == '[0007/1200] cls 0.123 | reg 1.000 | total 1.124 | 0.3s'
    assert T.log_line(4, 4, ('total', 'cls'), (2.0, float('nan')), 61.0) == '[4/4] total 2.000 | cls nan | 1.0m'
    assert T.log_line(100, 99999, ('grad_norm',), (float('inf'),), 7200.0) == '[00100/99999] grad_norm inf | 2.0h'
    # time_str's three ranges (libs/train_utils.py:56-61): hours from 3600, minutes above 60, seconds up to 60 inclusive
    assert [T.time_str(t) for t in (0.0, 0.04, 59.96, 60.0, 60.1, 3599.0, 3600.0, 5400.0)] == \
        ['0.0s', '0.0s', '60.0s', '60.0s', '1.0m', '60.0m', '1.0h', '1.5h']
    assert T.LOG_STATS == ('mean', 'finite_mean', 'min', 'max', 'last', 'n_finite') and T.STEP_KEYS == ('cls', 'reg', 'total', 'grad_norm')


# ---------------------------------------------------------------------------------------------- 4. the refusals
def test_bad_log_arguments_are_refused_before_anything_is_opened(tmp_path):
    T = load_pkg().train
    root = str(tmp_path / 'run')                                                  # not even the directory is made
    one = object.__new__(T.TrainStep)
    for run in (T.fit, T.fit_parallel):
        with pytest.raises(ValueError, match='log_interval'):
            run(one, None, root, log_interval=-1)
        with pytest.raises(ValueError, match='log_interval'):
            run(one, None, root, log_interval=2.5)
        with pytest.raises(ValueError, match='log_keys'):
            run(one, None, root, log_interval=2, log_keys=('cls', 'lr'))
        with pytest.raises(ValueError, match='log_keys'):
            run(one, None, root, log_interval=2, log_keys=())
        with pytest.raises(ValueError, match='log_keys'):
            run(one, None, root, log_interval=2, log_keys=('cls', 'cls'))
        with pytest.raises(ValueError, match='log_keys'):                        # checked with the log off too: a typo shows at once
            run(one, None, root, log_keys=('loss',))
    with pytest.raises(ValueError, match='log_interval'):
        T.StepLog(one, 10, log_interval=0)
    with pytest.raises(ValueError, match='log_keys'):
        T.StepLog(one, 10, keys=('norm',))
    assert not os.path.exists(root)


# ---------------------------------------------------------------------------------------------- 5. the data stream
SEED = 3


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('tree'))
    arrays, data = TT.random_tree(11, 6, 8, 6, 40, 5)
    TT.write_tree(root, arrays)
    return TT.cfg_of(root, dict(data, crop_ratio=(0.5, 1.0)))


def _loader(tree):
    """a fresh loader on the host route with two batches per epoch, and the list its decisions are recorded into"""
    data = load_pkg().data
    td = data.VideoCentricTrainData(tree, num_epochs=3, seed=SEED)
    seen, decide = [], td.decide

    def recording(epoch, idx, num_trials=5000):
        vid_id, seg_idx, window, target = decide(epoch, idx, num_trials)
        seen.append((epoch, idx, vid_id, tuple(seg_idx), None if window is None else tuple(window), target.tobytes()))
        return vid_id, seg_idx, window, target

    td.decide = recording
    loader = data.TrainLoader(td, None, len(td) // 2, device='cpu')
    assert len(loader) == 2
    return loader, seen


def _key(state):
    """a loader state as something ``==`` compares in full"""
    r, n = state['rng']['random'], state['rng']['numpy']
    return r, n[0], n[1].tobytes(), tuple(n[2:])


def _run(loader, epochs):
    for e in epochs:
        for _ in loader.epoch(e):
            pass


def test_rng_state_round_trip(tree):
    loader, _ = _loader(tree)
    td = loader.td
    state = td.rng_state()
    a = (td.rng.random(), td.np_rng.random_sample())
    assert td.set_rng_state(state) is td and (td.rng.random(), td.np_rng.random_sample()) == a
    with pytest.raises(ValueError, match='rng_state'):
        td.set_rng_state({'random': state['random']})
    with pytest.raises(ValueError, match='state'):
        loader.load_state({})


def test_a_resumed_loader_continues_the_decisions(tree):
    whole, seen_whole = _loader(tree)
    _run(whole, (0, 1, 2))
    first, seen_first = _loader(tree)
    _run(first, (0, 1))
    state = first.state()
    assert first._epoch_start is None, 'after an epoch the state is the live state'
    resumed, seen_resumed = _loader(tree)
    assert resumed.load_state(state) is resumed
    _run(resumed, (2,))
    assert seen_first + seen_resumed == seen_whole and len(seen_resumed) == 2 * resumed.batch_size
    assert any(w[4] is not None for w in seen_whole), 'crop_ratio draws windows on this tree'
    plain, seen_plain = _loader(tree)                                             # without load_state the streams start over
    _run(plain, (2,))
    assert [s[:4] for s in seen_plain] == [s[:4] for s in seen_resumed], 'the order and the grouping need no state'
    assert seen_plain != seen_resumed, f'seed {SEED} must give other windows without the state: choose another'


def test_a_state_taken_inside_an_epoch_replays_that_epoch(tree):
    whole, seen_whole = _loader(tree)
    _run(whole, (0, 1))
    first, seen_first = _loader(tree)
    _run(first, (0,))
    live = first.state()
    batches = first.epoch(1)
    next(batches)                                                                 # 1 of 2 batches of epoch 1
    inside = first.state()
    assert len(seen_first) == 3 * first.batch_size
    assert _key(inside) == _key(live), 'the snapshot taken at the start of epoch 1'
    assert _key({'rng': first.td.rng_state()}) != _key(inside), 'the live stream has moved on'
    resumed, seen_resumed = _loader(tree)
    resumed.load_state(inside)
    _run(resumed, (1,))
    n = 2 * first.batch_size
    assert seen_resumed == seen_whole[n:2 * n], 'epoch 1 from its start'
    assert len(list(batches)) == 1 and first._epoch_start is None and _key(first.state()) == _key(whole.state())


def test_two_ranks_gather_their_states_and_read_their_own_entry(tmp_path):
    here = os.path.dirname(os.path.abspath(__file__))
    cmd = ['timeout', '-k', '10', '120', sys.executable] + (['-s'] if sys.flags.no_user_site else []) + [os.path.join(here, 'data_state_rank_main.py')]
    logs = [open(tmp_path / f'rank{r}.log', 'w+') for r in range(2)]
    procs = [subprocess.Popen(cmd + [str(r), '2', str(tmp_path)], stdout=logs[r], stderr=subprocess.STDOUT, cwd=here,
                              env=dict(os.environ, PYTHONDONTWRITEBYTECODE='1')) for r in range(2)]
    codes = [p.wait() for p in procs]
    for r, log in enumerate(logs):
        log.seek(0)
        assert codes[r] == 0 and os.path.exists(tmp_path / f'rank{r}.ok'), f'rank {r}: exit {codes[r]}\n{log.read()}'
        log.close()
    import torch
    saved = torch.load(tmp_path / 'run' / 'states' / 'data_last.pth', map_location='cpu', weights_only=False)
    assert saved['world_size'] == 2 and len(saved['ranks']) == 2 and _key(saved['ranks'][0]) != _key(saved['ranks'][1])
    assert os.listdir(tmp_path / 'run') == ['states'] and os.listdir(tmp_path / 'run' / 'states') == ['data_last.pth']
