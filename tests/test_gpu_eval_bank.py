"""GPU checks of the validation set in device memory (``data.EvalBank``) and of ``GroundingEvaluator.run`` with an
``evaluator.DeviceRecallCounter``, on generated trees (tests/train_data_tree.random_tree) at the widths of the tiny model of
tests/golden/step_grad_s2: 5 videos with 1 - 3 queries each, read through ``VideoCentricEvalData`` with ``eval_split=('train',)``.

1. For every video the bank-fed ``prepare`` gives the bits of the host-fed one -- windows, mask, encoded tokens, text_cls -- in fp32
   and on float16 copies of the files with ``feature_dtype='stored'``; one video of the tree is longer than max_vid_len * vid_stride.
2. ``run(bank, counter=DeviceRecallCounter(...))`` counts what ``run(host dataset, counter=RecallCounter(...))`` counts, in all three
   run modes, with soft-NMS and with greedy NMS; ``max_num_segs = 0`` counts every query as a miss on both routes.
3. After a warm-up pass, a second bank-fed pass with the device counter runs under torch's sync debug mode set to 'error'.
4. A host dataset with the device counter; a pass repeated after the LayerNorm guard reported; an iterator is refused.
5. ``ext_score_dir`` is refused."""
import numpy as np
import pytest
import torch

import step_grad_ref as R
import train_data_tree as TT
from conftest import load_pkg

pytestmark = pytest.mark.gpu
MODES = {'one-stream': dict(n_streams=1), 'batched': dict(batch_videos=2), 'lanes': dict(n_streams=2)}


def same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and a.device == b.device, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8)), what


def eval_cfg(root, data, **more):
    return dict(TT.cfg_of(root, data), eval_split=('train',), **more)


@pytest.fixture(scope='module')
def world():
    """the package, the fixture, the model on the GPU and its opt tree"""
    pkg = load_pkg()
    f = R.Fixture('s2')
    return pkg, f, f.model(pkg).cuda().eval().requires_grad_(False), f.opt(pkg)


def tree(tmp_path, f, seed, longest, half=False):
    kw = f.opt_kwargs
    arrays, data = TT.random_tree(seed, 5, kw['D'], kw['text_in'], longest, 9)
    TT.write_tree(str(tmp_path), arrays, half=half)
    return data


@pytest.mark.parametrize('half', [False, True], ids=['fp32', 'stored-f16'])
def test_bank_fed_prepare_has_the_bits_of_the_host_fed_one(tmp_path, world, half):
    pkg, f, model, opt = world
    data = tree(tmp_path, f, 11, 170, half)
    ed = pkg.data.VideoCentricEvalData(eval_cfg(str(tmp_path), data, feature_dtype='stored' if half else np.float32))
    bank = pkg.data.EvalBank(ed, vid_stride=f.opt_kwargs['vid_stride'])
    want = torch.float16 if half else torch.float32
    assert bank.data['vid'].dtype == bank.data['shallow'].dtype == want and bank.data['text'].dtype == torch.float32 and bank.data['vid'].is_cuda
    assert len(bank) == len(ed) == 5 and bank.meta.shape == (sum(len(v['segments']) for v in ed.videos.values()), 8)
    ev = pkg.evaluator.GroundingEvaluator(opt, model)
    limit = opt['model']['max_vid_len'] * f.opt_kwargs['vid_stride']
    lengths = []
    for item, sample in zip(bank, ed):
        assert item['clip_id'] == sample['clip_id'] and 'vid' not in item
        (a, T, ext), (b, T_host, _) = ev.prepare(item), ev.prepare(sample)
        assert T == T_host and ext is None
        lengths.append(sample['vid'].size(-1))
        for k, name in enumerate(('vid', 'shallow_vid', 'mask')):
            same_bits(a[k], b[k], f"{item['clip_id']}: {name}")
        assert a[0].shape == (1, f.opt_kwargs['D'], T) and a[0].dtype == want
        assert len(a[3]) == len(b[3]) == len(sample['text'])
        for q in range(len(a[3])):
            same_bits(a[3][q], b[3][q], f"{item['clip_id']}: tokens of query {q}")
            same_bits(a[5][q], b[5][q], f"{item['clip_id']}: token mask of query {q}")
        same_bits(a[4], b[4], f"{item['clip_id']}: text_cls")
        same_bits(item['meta'].cpu(), torch.from_numpy(pkg.evaluator.query_meta(sample['segment'], ev.vid_stride, sample['clip_stride'],
                                                                               sample['clip_size'], sample['fps'], sample['duration'])), 'meta')
    assert max(lengths) > limit > min(lengths), lengths                         # one video pads to a multiple of the chunk, the others to the limit


def _run_both(pkg, world, root, data, mode, nms_mode, max_num_segs=None):
    _, f, model, opt = world
    E = pkg.evaluator
    ed = pkg.data.VideoCentricEvalData(eval_cfg(root, data))
    bank = pkg.data.EvalBank(ed, vid_stride=f.opt_kwargs['vid_stride'])
    ev = E.GroundingEvaluator(opt, model)
    ev.nms_cfg['mode'] = nms_mode
    if max_num_segs is not None:
        ev.nms_cfg['max_num_segs'] = max_num_segs
    ranks, threshs = (1, 2, 5), (0.01, 0.05, 0.1, 0.3, 0.5)          # low thresholds too: an untrained model rarely reaches 0.3
    host = ev.run(ed, counter=E.RecallCounter(ranks, threshs), **MODES[mode])
    dev = ev.run(bank, counter=E.DeviceRecallCounter(ranks, threshs), **MODES[mode])
    return host, dev, ed


@pytest.mark.parametrize('nms_mode', ['soft_nms', 'nms'])
@pytest.mark.parametrize('mode', list(MODES))
def test_device_counter_on_the_bank_equals_the_host_route(tmp_path, world, mode, nms_mode):
    pkg = world[0]
    data = tree(tmp_path, world[1], 5, 80)
    host, dev, ed = _run_both(pkg, world, str(tmp_path), data, mode, nms_mode)
    print(f'{mode} {nms_mode}: hits {host.hits.tolist()} of {host.n_queries}')
    assert np.array_equal(dev.hits, host.hits) and dev.n_queries == host.n_queries == sum(len(v['segments']) for v in ed.videos.values())
    assert dev.report() == host.report()


def test_no_kept_segment_is_a_miss_on_both_routes(tmp_path, world):
    pkg = world[0]
    data = tree(tmp_path, world[1], 5, 80)
    host, dev, _ = _run_both(pkg, world, str(tmp_path), data, 'one-stream', 'soft_nms', max_num_segs=0)
    assert dev.n_queries == host.n_queries > 0 and not dev.hits.any() and not host.hits.any()


def test_a_pass_with_the_device_counter_never_waits_for_the_gpu(tmp_path, world):
    pkg, f, model, opt = world
    data = tree(tmp_path, f, 5, 80)
    bank = pkg.data.EvalBank(pkg.data.VideoCentricEvalData(eval_cfg(str(tmp_path), data)), vid_stride=f.opt_kwargs['vid_stride'])
    ev = pkg.evaluator.GroundingEvaluator(opt, model)
    counter = pkg.evaluator.DeviceRecallCounter((1, 5), (0.3, 0.5))
    warm = ev.run(bank, counter=counter).hits                                   # engines, caches and the text position tables exist now
    counter.reset()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        ev.run(bank, counter=counter)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert np.array_equal(counter.hits, warm) and counter.n_queries == bank.meta.shape[0]


def test_host_samples_with_the_device_counter_and_a_repeated_pass(tmp_path, world):
    """a host dataset may feed the device counter too (its records are uploaded per video); and when the one-pass LayerNorm guard
    reports after the last video, the counter is reset and the pass repeated once: the table is that of one pass"""
    pkg, f, model, opt = world
    E = pkg.evaluator
    data = tree(tmp_path, f, 5, 80)
    ed = pkg.data.VideoCentricEvalData(eval_cfg(str(tmp_path), data))
    bank = pkg.data.EvalBank(ed, vid_stride=f.opt_kwargs['vid_stride'])
    ranks, threshs = (1, 2, 5), (0.01, 0.05, 0.1, 0.3, 0.5)
    ev = E.GroundingEvaluator(opt, model)
    host = ev.run(ed, counter=E.RecallCounter(ranks, threshs))
    dev = ev.run(ed, counter=E.DeviceRecallCounter(ranks, threshs))
    assert np.array_equal(dev.hits, host.hits) and dev.n_queries == host.n_queries
    asked = []

    def tripped_once(models):
        asked.append(len(models))
        return len(asked) == 1

    ev._carry_tripped = tripped_once
    forwards = len(ev.time_dict['forward'])
    again = ev.run(bank, counter=E.DeviceRecallCounter(ranks, threshs))
    assert asked == [1] and len(ev.time_dict['forward']) - forwards == 2 * len(bank)            # asked once, after the last video; two passes
    assert np.array_equal(again.hits, host.hits) and again.n_queries == host.n_queries
    with pytest.raises(TypeError, match='iterator'):
        ev.run(iter(bank), counter=E.DeviceRecallCounter(ranks, threshs))


def test_ext_scores_are_refused(tmp_path, world):
    pkg = world[0]
    data = tree(tmp_path, world[1], 5, 80)
    ed = pkg.data.VideoCentricEvalData(eval_cfg(str(tmp_path), data, ext_score_dir=str(tmp_path / 'scores')))
    with pytest.raises(NotImplementedError, match='ext_score_dir'):
        pkg.data.EvalBank(ed)
