"""GPU checks of ``train.fit``: ``Trainer.run`` with its checkpoints and its evaluations of the EMA copy, on the tiny model of
tests/golden/step_grad_s2 (built by ``modeling.create_model``, so that ``GroundingEvaluator.from_checkpoint`` rebuilds the same
network) and a generated tree (tests/train_data_tree.random_tree): 5 videos, two steps per epoch, ``front_end='shared'``, the
validation set -- the same videos through ``VideoCentricEvalData`` -- in a ``data.EvalBank``.  ``crop_ratio`` is None: the loader's
random streams are not part of a checkpoint, and without the crop no decision draws from them.

1. Two epochs with an evaluation per epoch: the files, their keys, and the metrics of epoch 2 against ``from_checkpoint`` on the
   host route with ``RecallCounter``.
2. Evaluation does not disturb training: parameters and the EMA copy bit-equal to a run with ``eval_run=0``.
3. One epoch, then fresh objects with ``resume=True`` up to two epochs: parameters, EMA copy, optimizer state and metrics of the
   uninterrupted run.
4. ``eval_by='itr', eval_run=3`` over two epochs evaluates and checkpoints at iteration 3 only.
5. More than one rank is refused before anything is launched."""
import os

import numpy as np
import pytest
import torch

import step_grad_ref as R
import train_data_tree as TT
from conftest import load_pkg

pytestmark = pytest.mark.gpu
T_IN = 80                                                                     # the input length of the training batches


@pytest.fixture(scope='module')
def world(tmp_path_factory):
    pkg = load_pkg()
    f = R.Fixture('s2')
    kw = f.opt_kwargs
    root = str(tmp_path_factory.mktemp('tree'))
    arrays, data = TT.random_tree(5, 5, kw['D'], kw['text_in'], T_IN, 9)
    TT.write_tree(root, arrays)
    cfg = dict(TT.cfg_of(root, dict(data, crop_ratio=None)), eval_split=('train',))
    ed = pkg.data.VideoCentricEvalData(cfg)
    return pkg, f, cfg, ed, pkg.data.EvalBank(ed, vid_stride=kw['vid_stride'])


def make(world):
    """fresh objects: (ts, loader)"""
    pkg, f, cfg, _, _ = world
    td = pkg.data.VideoCentricTrainData(cfg, num_epochs=2, seed=3)
    loader = pkg.data.TrainLoader(td, pkg.data.FeatureBank(td), len(td) // 2, input_vid_len=T_IN, vid_stride=f.opt_kwargs['vid_stride'])
    assert len(loader) == 2
    opt = f.opt(pkg)
    opt.train.warmup_epochs = 1
    model = pkg.modeling.create_model(opt)
    model.load_state_dict(f.sd)
    return pkg.train.TrainStep(model.cuda(), opt, itrs_per_epoch=len(loader), front_end='shared'), loader


def tensors(ts):
    """parameters, EMA copy and optimizer state as one list of tensors on the CPU"""
    out = [p.detach().cpu() for p in ts.model.parameters()] + [p.detach().cpu() for p in ts.ema.module.parameters()]
    for st in ts.optimizer.state_dict()['state'].values():
        out += [v.detach().cpu() for _, v in sorted(st.items()) if torch.is_tensor(v)]
    return out


def same_tensors(a, b, what):
    assert len(a) == len(b) and len(a) > 0
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == y.dtype and torch.equal(x.contiguous().reshape(-1).view(torch.uint8), y.contiguous().reshape(-1).view(torch.uint8)), f'{what}: tensor {i}'


@pytest.fixture(scope='module')
def full_run(world, tmp_path_factory):
    """two epochs with an evaluation after each: (root, results, tensors, the training model's mode)"""
    pkg, _, _, _, bank = world
    root = str(tmp_path_factory.mktemp('full'))
    ts, loader = make(world)
    mode = ts.model.training
    results = pkg.train.fit(ts, loader, root, num_epochs=2, eval_data=bank, eval_by='epoch', eval_run=1)
    assert ts.model.training == mode and not ts.ema.module.training
    return root, results, tensors(ts), ts


def test_two_epochs_checkpoint_and_evaluate(world, full_run):
    pkg, f, _, ed, bank = world
    root, results, _, ts = full_run
    assert ts.epoch == 2 and ts.itr == 4
    for name in ('models/last.pth', 'models/1-2.pth', 'models/2-4.pth', 'states/last.pth', 'eval_1_2.txt', 'eval_2_4.txt'):
        assert os.path.exists(os.path.join(root, name)), name
    assert sorted(os.listdir(os.path.join(root, 'models'))) == ['1-2.pth', '2-4.pth', 'last.pth']
    m = torch.load(os.path.join(root, 'models', '2-4.pth'), map_location='cpu', weights_only=False)
    s = torch.load(os.path.join(root, 'states', 'last.pth'), map_location='cpu', weights_only=False)
    assert set(m) == {'model', 'model_ema'} and set(m['model']) == set(m['model_ema']) == set(ts.model.state_dict())
    assert set(s) == {'optimizer', 'scheduler', 'epoch', 'itr', 'loss_norm'} and (s['epoch'], s['itr']) == (2, 4)
    assert [(e, i) for e, i, _ in results] == [(1, 2), (2, 4)]
    opt = f.opt(pkg)
    ev = pkg.evaluator.GroundingEvaluator.from_checkpoint(opt, root, ckpt='2-4')
    host = ev.run(ed, counter=pkg.evaluator.RecallCounter(opt['eval']['ranks'], opt['eval']['iou_threshs']))
    print('epoch 2 metrics', results[1][2].tolist(), 'of', host.n_queries)
    assert host.n_queries == bank.meta.shape[0] and np.array_equal(results[1][2], host.metrics())
    assert open(os.path.join(root, 'eval_2_4.txt')).read() == host.report()


def test_evaluation_does_not_disturb_training(world, full_run, tmp_path):
    pkg = world[0]
    ts, loader = make(world)
    assert pkg.train.fit(ts, loader, str(tmp_path), num_epochs=2, eval_run=0) == []
    assert os.path.exists(tmp_path / 'models' / '2-4.pth') and not [n for n in os.listdir(tmp_path) if n.startswith('eval_')]
    same_tensors(tensors(ts), full_run[2], 'with and without evaluation')


def test_resume_continues_the_uninterrupted_run(world, full_run, tmp_path):
    pkg, bank = world[0], world[4]
    kw = dict(eval_data=bank, eval_by='epoch', eval_run=1)
    ts, loader = make(world)
    first = pkg.train.fit(ts, loader, str(tmp_path), num_epochs=1, **kw)
    assert ts.epoch == 1 and len(first) == 1
    ts, loader = make(world)                                                   # fresh objects: everything comes from the two last.pth files
    second = pkg.train.fit(ts, loader, str(tmp_path), num_epochs=2, resume=True, **kw)
    assert (ts.epoch, ts.itr) == (2, 4) and [(e, i) for e, i, _ in second] == [(2, 4)]
    same_tensors(tensors(ts), full_run[2], 'resumed and uninterrupted')
    assert np.array_equal(first[0][2], full_run[1][0][2]) and np.array_equal(second[0][2], full_run[1][1][2])
    ts, loader = make(world)                                                   # resume=False starts over, whatever lies in root
    pkg.train.fit(ts, loader, str(tmp_path), num_epochs=1, resume=False, eval_run=0)
    assert (ts.epoch, ts.itr) == (1, 2)


def test_evaluation_by_iteration(world, tmp_path):
    pkg, bank = world[0], world[4]
    ts, loader = make(world)
    results = pkg.train.fit(ts, loader, str(tmp_path), num_epochs=2, eval_data=bank, eval_by='itr', eval_run=3)
    assert (ts.epoch, ts.itr) == (2, 4) and [(e, i) for e, i, _ in results] == [(1, 3)]
    assert sorted(os.listdir(tmp_path / 'models')) == ['1-3.pth', 'last.pth']
    assert [n for n in os.listdir(tmp_path) if n.startswith('eval_')] == ['eval_1_3.txt']
    s = torch.load(tmp_path / 'states' / 'last.pth', map_location='cpu', weights_only=False)
    assert (s['epoch'], s['itr']) == (1, 3)


def test_more_than_one_rank_is_refused(tmp_path):
    T = load_pkg().train
    ts = object.__new__(T.DataParallelTrainStep)
    ts.group, ts.world = object(), 2                                            # a stub group: nothing is constructed or launched
    with pytest.raises(NotImplementedError, match='world 2'):
        T.fit(ts, None, str(tmp_path))
    assert not os.listdir(tmp_path)
    with pytest.raises(ValueError, match='eval_by'):
        T.fit(object.__new__(T.TrainStep), None, str(tmp_path), eval_by='step')
