"""GPU checks of ``evaluator.DeviceLossMeter``: the validation loss of a train-time evaluation without a host read per video, on the
set-up of tests/test_gpu_fit.py (tests/fit_setup.py: model s2, a tree of 5 videos with 9 queries, T = 80).

1. ``run(bank, counter=DeviceRecallCounter, loss_meter=meter)`` against the host route -- per video ``calc_loss`` on that video's
   forward, then the mean of the stats: the meter's row table bit-equal to the stacked per-row results, the losses within
   (N + V) * 2^-52 relative (sums of non-negative doubles in two orders), the counter what it is without the meter.
2. The same table with ``n_streams=2`` and with ``batch_videos=2``.
3. A 3 / 2 split through ``EvalBank.subset`` plus a summed table gives the bits of the whole pass.
4. ``update_device`` refuses, with the video's name and before the launch, what dcf_point_objective would refuse; the host route refuses
   a meter."""
import numpy as np
import pytest
import torch

import eval_loss_ref as LR
import fit_setup as S
from conftest import load_pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def world(tmp_path_factory):
    pkg = load_pkg()
    f, cfg, ed, bank = S.build_world(pkg, str(tmp_path_factory.mktemp('tree')))
    opt = S.make_opt(pkg, f)
    model = pkg.modeling.create_model(opt)
    model.load_state_dict(f.sd)
    ev = pkg.evaluator.GroundingEvaluator(opt, model.cuda().eval().requires_grad_(False))
    return pkg, opt, ev, ed, bank


@pytest.fixture(scope='module')
def host(world):
    """the host route, computed once: (rows (N, 4), per-row (N, 2), {'cls_loss', 'reg_loss'})"""
    pkg, opt, ev, ed, _ = world
    return S.host_loss(pkg, ev, ed, opt)


def device_pass(world, dataset=None, **kw):
    pkg, opt, ev, _, bank = world
    E = pkg.evaluator
    meter = E.DeviceLossMeter(bank)
    counter = ev.run(bank if dataset is None else dataset, counter=E.DeviceRecallCounter(opt['eval']['ranks'], opt['eval']['iou_threshs']),
                     loss_meter=meter, **kw)
    return meter, counter


def bits(t):
    return t.contiguous().view(torch.int32)


def test_meter_equals_the_host_route(world, host):
    pkg, opt, ev, ed, bank = world
    rows, per_row, stats = host
    meter, counter = device_pass(world)
    assert meter.opt is opt and meter.rows.shape == (9, 4) and meter.offsets.tolist() == [0, 1, 3, 6, 7, 9]
    assert torch.equal(meter.targets.cpu(), torch.cat([ed.targets(k, ev.vid_stride) for k in ed.videos]))
    got = meter.rows.cpu()
    assert torch.equal(bits(got), bits(rows)), 'the row table differs from the stacked per-row results of the host route'
    assert bool((got[:, 3] > 0).any()) and bool(torch.isfinite(got).all())
    assert np.array_equal(LR.per_query(got.numpy()), per_row.astype(np.float64)), 'calc_loss divides as the operator does'
    losses, pv = meter.losses(per_video=True)
    want_pv, want = LR.loss_table_mean(got.numpy(), meter.offsets.cpu().numpy())
    assert np.array_equal(LR.bits(pv), LR.bits(want_pv)) and losses == {'cls_loss': float(want[0]), 'reg_loss': float(want[1])}
    bound = S.loss_bound(bank)
    for k in ('cls_loss', 'reg_loss'):
        err = abs(losses[k] - stats[k]) / stats[k]
        print(f'LOSSMETER {k}: device {losses[k]!r} host {stats[k]!r} relative {err:.3g} bound {bound:.3g}')
        assert err <= bound, k
    assert meter.losses() == losses
    plain = ev.run(bank, counter=pkg.evaluator.DeviceRecallCounter(opt['eval']['ranks'], opt['eval']['iou_threshs']))
    assert np.array_equal(plain.hits, counter.hits) and plain.n_queries == counter.n_queries == 9
    assert pkg.evaluator.DeviceLossMeter.line(losses) == f"cls_loss: {losses['cls_loss']:.3f}; reg_loss: {losses['reg_loss']:.3f}; "


@pytest.mark.parametrize('mode', [dict(n_streams=2), dict(batch_videos=2)], ids=['two-streams', 'two-videos-a-forward'])
def test_the_same_table_in_the_other_modes(world, host, mode):
    meter, counter = device_pass(world, **mode)
    assert torch.equal(bits(meter.rows.cpu()), bits(host[0])) and counter.n_queries == 9


def test_a_split_through_subset_sums_to_the_whole_pass(world, host):
    bank = world[4]
    a, ca = device_pass(world, bank.subset([1, 0, 4]))
    b, cb = device_pass(world, bank.subset([2, 3]))
    assert ca.n_queries + cb.n_queries == 9
    own = lambda m: (m.rows != 0).any(1).cpu()
    assert not bool((own(a) & own(b)).any()), 'the shares own disjoint rows'
    total = a.rows + b.rows
    assert torch.equal(bits(total.cpu()), bits(host[0])), 'adding zeros is exact'
    whole, cw = device_pass(world)
    a.rows.copy_(total)
    assert a.losses() == whole.losses() and np.array_equal(ca.hits + cb.hits, cw.hits)


def test_refusals(world):
    pkg, opt, ev, ed, bank = world
    E = pkg.evaluator
    meter = E.DeviceLossMeter(bank, opt)
    data = next(iter(bank))
    before = meter.rows.clone()
    msl = pkg.loss.pt_gen_params(opt)[0][2]
    T = 2 * msl * ev.vid_stride                                                  # T // vid_stride beyond pt_gen's max_seq_len
    S_ = sum((T // ev.vid_stride) >> l for l in range(ev.num_fpn_levels))
    flat = (torch.zeros(1, S_, device='cuda'), torch.zeros(1, S_, 2, device='cuda'), torch.ones(1, S_, dtype=torch.bool, device='cuda'))
    with pytest.raises(ValueError, match=data['clip_id']):
        meter.update_device(flat, T, data)
    with pytest.raises(ValueError, match=data['clip_id']):                       # the shapes of another layout
        meter.update_device(flat, S.T_IN, data)
    with pytest.raises(ValueError, match='no opt'):
        E.DeviceLossMeter(bank).update_device(flat, S.T_IN, data)
    with pytest.raises(ValueError, match='device route'):
        ev.run(ed, counter=E.RecallCounter(), loss_meter=meter)
    with pytest.raises(ValueError, match='device route'):
        ev.run(ed, loss_meter=meter)
    torch.cuda.synchronize()
    assert torch.equal(meter.rows, before)
