"""GPU checks of the training step on float16 clip features: ``train.training_forward(front_end='shared')`` hands the stored halves to
dcf_op_sidekick_h and to ``autograd.gated_vid_map`` (include/decafnet_hip_front_half.h), and every output, every parameter gradient
and the state after two ``TrainStep`` steps have the bits of the same values passed as fp32.  On the fixtures of
tests/test_gpu_train_step.py (E = 64: the forward products take the upcast path, the weight gradient the half kernel) and on one
model whose forward products read the halves natively (E = 128, T = 512, under half_native = 2)."""
import pytest
import torch

from conftest import load_pkg
import test_gpu_train_step as TS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def pkg():
    return load_pkg()


def half_batch(batch):
    """(the batch with vid / shallow rounded to binary16 and kept as float16, the same values as fp32)"""
    h = dict(batch, vid=batch['vid'].half(), shallow=batch['shallow'].half())
    return h, dict(h, vid=h['vid'].float(), shallow=h['shallow'].float())


def forward_backward(pkg, model, opt, batch, targets, **kw):
    """one training forward, the objective and backward() -> (flat outputs, total, {parameter: gradient})"""
    model.zero_grad(set_to_none=True)
    out = pkg.train.training_forward(model, **batch, **kw)
    total = pkg.loss.PointObjective(opt)(out, targets)['total']
    total.backward()
    flat = [t.detach().clone() for level in out[:3] for t in level] + [m.clone() for m in out[3]]
    return flat, total.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()}


def assert_same(a, b):
    (fa, ta, ga), (fb, tb, gb) = a, b
    assert len(fa) == len(fb) and all(torch.equal(u, v) for u, v in zip(fa, fb))
    assert torch.equal(ta, tb)
    assert ga.keys() == gb.keys() and not [k for k in ga if not torch.equal(ga[k], gb[k])]


@pytest.mark.parametrize('name', ['s1', 's2'])
def test_a_float16_batch_gives_the_bits_of_the_fp32_batch(pkg, name):
    f = TS.fixture(name)
    model, opt = f.model(pkg).cuda(), f.opt(pkg)
    batch, targets = TS.batch_of(f)
    h, f32 = half_batch(batch)
    assert model.half_features is True and model.last_train_feature_dtype is None
    got = forward_backward(pkg, model, opt, h, targets, front_end='shared')
    assert model.last_train_feature_dtype == torch.float16
    want = forward_backward(pkg, model, opt, f32, targets, front_end='shared')
    assert model.last_train_feature_dtype == torch.float32
    assert_same(got, want)
    assert all(bool(torch.isfinite(g).all()) for g in want[2].values())
    model.half_features = False                            # the float16 batch is upcast first, as before
    off = forward_backward(pkg, model, opt, h, targets, front_end='shared')
    assert model.last_train_feature_dtype == torch.float32
    assert_same(off, want)
    model.half_features = True
    if not model.scat:                                     # (a scat model takes the shared path whatever front_end says)
        dense = forward_backward(pkg, model, opt, h, targets, front_end='dense')
        assert model.last_train_feature_dtype == torch.float32
        assert_same(dense, forward_backward(pkg, model, opt, f32, targets, front_end='dense'))
    assert model.last_feature_dtype is None                # the eval forward's record keeps its meaning


def _tapped(pkg, keep):
    """autograd.gated_vid_map wrapped: the dtype of the features and the gate of the call land in `keep`"""
    inner = pkg.autograd.gated_vid_map

    def tap(vid, shallow, gate, mask, correl, *rest, **kw):
        keep.append(dict(dtype=vid.dtype, gate=gate.detach().clone(), sizes=list(rest[0])))
        return inner(vid, shallow, gate, mask, correl, *rest, **kw)
    return inner, tap


def test_a_model_whose_forward_products_read_the_halves(pkg):
    """E % 128 == 0, T % 4 == 0: under half_native = 2 the products of vid_map run on the half mode of the split tile path or fail"""
    kw = dict(D=64, E=128, TE=32, text_in=32, n_levels=4, win=5, n_heads=4, sn=64, sratio=0.3, msf=True, norm=True, max_seq_len=512,
              text_layers=1, text_max_len=24)
    T, lens_nq = 512, [(512, 2), (400, 1)]
    opt = pkg.config.make_opt(**kw)
    model = pkg.modeling.PtTransformerEarlyFusionIterative(opt)
    model.load_state_dict(pkg.synth.make_state_dict({k: list(v.shape) for k, v in model.state_dict().items()}, 45))
    model = model.cuda()
    inps = [pkg.synth.make_inputs(64, T, vid_len, nq, 32, 6, 1600 + v) for v, (vid_len, nq) in enumerate(lens_nq)]
    c = lambda z: z.cuda().contiguous()
    batch = dict(vid=c(torch.cat([i['vid'] for i in inps])), shallow=c(torch.cat([i['shallow_vid'] for i in inps])),
                 vid_masks=c(torch.cat([i['vid_masks'] for i in inps])), tokens=c(torch.stack([t for i in inps for t in i['tokens']])),
                 text_cls=c(torch.cat([i['text_cls'] for i in inps])), token_masks=torch.ones(3, 1, 6, dtype=torch.bool, device='cuda'),
                 text_size=[nq for _, nq in lens_nq])
    targets = torch.tensor([[40.0, 120.0], [200.0, 330.0], [100.0, 180.0]], device='cuda')
    h, f32 = half_batch(batch)
    keep, lb = [], pkg._lib
    inner, tap = _tapped(pkg, keep)
    pkg.autograd.gated_vid_map = tap
    lb.check(lb.lib().dcf_debug_set_option(b'half_native', 2), 'dcf_debug_set_option')
    try:
        got = forward_backward(pkg, model, opt, h, targets, front_end='shared')
        assert model.last_train_feature_dtype == torch.float16
        want = forward_backward(pkg, model, opt, f32, targets, front_end='shared')
    finally:
        lb.check(lb.lib().dcf_debug_set_option(b'half_native', -1), 'dcf_debug_set_option')
        pkg.autograd.gated_vid_map = inner
    assert [k['dtype'] for k in keep] == [torch.float16, torch.float32] and torch.equal(keep[0]['gate'], keep[1]['gate'])
    assert_same(got, want)
    assert all(bool(torch.isfinite(g).all()) for g in want[2].values()) and float(want[2]['vid_map.conv.weight'].abs().max()) > 0
    # a 64-clip tile of a video that none of its queries keeps: the expert product skips it and the weight gradient takes no K step there
    gate, q, closed = keep[0]['gate'].cpu(), 0, []
    for b, k in enumerate(keep[0]['sizes']):
        closed += [(b, t0) for t0 in range(0, T, 64) if not bool(gate[q:q + k, t0:t0 + 64].any())]
        q += k
    assert closed, 'every tile of every video is kept by some query'


def test_two_steps_on_a_float16_batch_leave_the_state_of_the_fp32_batch(pkg):
    f = TS.fixture('s1')
    batch, targets = TS.batch_of(f)
    h, f32 = half_batch(batch)
    steps = []
    for b in (h, f32):
        ts = pkg.train.TrainStep(f.model(pkg).cuda(), TS.opt_of(pkg, f), itrs_per_epoch=1, front_end='shared')
        losses = [ts.step(b, targets) for _ in range(2)]
        steps.append((ts, losses))
    (ta, la), (tb, lb) = steps
    assert ta.model.last_train_feature_dtype == torch.float16 and tb.model.last_train_feature_dtype == torch.float32
    assert not TS.bits_differ(TS.state_of(ta), TS.state_of(tb))
    for da, db in zip(la, lb):
        assert da.keys() == db.keys() and all(torch.equal(da[k], db[k]) for k in da)
