"""The reader of the tests/golden/step_grad_<case>*.npz fixtures (make_golden_step_grad.py: one whole training step of the reference, in
fp32 and fp64) and ONE function, `run_step`, that composes the same step from the package's own pieces: dcf_op_sidekick / dcf_op_gate,
autograd.masked_conv1d (vid_map), text_transformer, xattn_fusion (the first fusion), video_transformer, fuse_and_predict and
loss.PointObjective.  Nothing of the model is restated in torch here; the oracle's gate is behind `oracle_gate` for the CPU test.  A
helper module of tests/test_step_grad_cpu.py and tests/test_gpu_step_grad.py.

Fixture tensors are turned token-major: (B, T, C) features, (B, T) masks."""
import sys
from types import SimpleNamespace

import torch

from conftest import Golden, ROOT

if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import decafnet_ref as O  # noqa: E402

CASES = ('s2', 's1')
ZERO_BY_SYMMETRY = ('key.bias', 'k_norm.bias')
TAPS = ('vid_map', 'text', 'fused')
GTAPS = ('text', 'fused')
FILES = ('', '_gp_front', '_gp_vid_net', '_gp_heads')


def tm(x):
    return x.transpose(1, 2).contiguous()


class Fixture:
    """case `name` of tests/golden/step_grad_<name>*.npz.  Inputs: vid / shallow (bs, D, T) channel-major as the reference takes them,
    vid_masks (bs, T), tokens (B', Lq, C) token-major, token_masks (B', Lq), text_cls (B', D), text_size, targets (B', 2).  Recorded:
    gate / mask_gated (B', T), labels (B', S), gt_offsets (B', S, 2), masks[l] (B', T_l), and by precision tag '32' / '64' out[tag] =
    {logits1, logits2, offsets: per level}, total[tag], taps[tag] = {vid_map, text, fused, fpn0..: token-major}, gtaps[tag] = {text,
    fused}, gp[tag] = {parameter: gradient} (the fp64 one rebuilt as g_32 + d in fp64).  sd: the state dict; opt_kwargs for config.make_opt"""

    def __init__(self, name):
        g = Golden(f'step_grad_{name}.npz')
        self.name, self.meta, self.opt_kwargs = name, g.js('meta'), g.js('opt_kwargs')
        self.L, self.second_fusion = self.meta['n_levels'], self.meta['second_fusion']
        self.text_size = self.meta['text_size']
        lv = range(self.L)
        self.vid, self.shallow, self.vid_masks = g.t('vid'), g.t('shallow'), g.t('vid_masks')
        self.tokens, self.token_masks, self.text_cls = tm(g.t('tokens')), g.t('token_masks')[:, 0], g.t('text_cls')
        self.targets, self.labels, self.gt_offsets = g.t('targets'), g.t('labels'), g.t('gt_offsets')
        self.gate, self.mask_gated = g.t('gate'), g.t('mask_gated')
        self.masks = [g.t(f'mask/l{l}') for l in lv]
        self.sd = g.sub('param/')
        self.out = {t: {k: [g.t(f'{k}_{t}/l{l}') for l in lv] for k in ('logits1', 'logits2', 'offsets')} for t in ('32', '64')}
        self.total = {t: g.t(f'total_{t}') for t in ('32', '64')}
        self.taps = {t: {k: tm(v) for k, v in g.sub(f'tap_{t}/').items()} for t in ('32', '64')}
        self.gtaps = {t: {k: tm(v) for k, v in g.sub(f'gtap_{t}/').items()} for t in ('32', '64')}
        self.gp = {'32': {}, '64': {}}
        for part in self.meta['parts']:
            z = Golden(f'step_grad_{name}_gp_{part}.npz')
            for k, g32 in z.sub('32/').items():
                self.gp['32'][k], self.gp['64'][k] = g32, g32.double() + z.t(f'd/{k}').double()
        assert len(self.gp['32']) == len(self.gp['64']) == self.meta['n_params']

    def opt(self, pkg):
        """the opt tree of the case: config.make_opt plus the Trainer's center_sampling / reg_loss of the case"""
        opt = pkg.config.make_opt(**self.opt_kwargs)
        opt.train.center_sampling, opt.train.reg_loss = self.meta['center_sampling'], self.meta['reg_loss']
        return opt

    def model(self, pkg):
        """a modeling.PtTransformerEarlyFusionIterative with the fixture's state dict (on the CPU)"""
        model = pkg.modeling.PtTransformerEarlyFusionIterative(self.opt(pkg), second_fusion=self.second_fusion)
        model.load_state_dict(self.sd)
        return model

    def top(self, k, tag='64'):
        """max |g_64| of the gradient rule for parameter `k`: for the gradients that are zero in exact arithmetic (key.bias of every
        attention, k_norm.bias of the video blocks: a constant on all keys moves a row's scores alike) that of the same layer's
        key.weight / k_norm.weight, the terms that cancel (backbone_grad_ref.Fixture.top)"""
        if k.endswith(ZERO_BY_SYMMETRY):
            k = k[:-len('bias')] + 'weight'
        return float(self.gp[tag][k].double().abs().max())

    def oracle_gate(self, dtype=torch.float32):
        """(gate (B', T) bool, mask after the gate (B', T)) by the oracle's sidekick_scores / topk_block_gate (model.py:587-608)"""
        cfg = self.opt_kwargs
        sizes = torch.tensor(self.text_size)
        shallow, masks = self.shallow.to(dtype).repeat_interleave(sizes, 0), self.vid_masks.repeat_interleave(sizes, 0)
        correl = O.sidekick_scores(shallow, self.text_cls.to(dtype), cfg['norm'])
        gate = torch.zeros_like(masks)
        for b in range(masks.size(0)):
            n = int(masks[b].sum())
            gate[b, :n] = O.topk_block_gate(correl[b], n, cfg['sn'], cfg['sratio']).bool()
        return gate, (masks if cfg['msf'] else masks & gate)


def run_step(pkg, model, f, text_use=None, check_gate=True):
    """One training step of `model` (on the GPU) on the inputs of fixture `f`, composed as model.py:567-632 composes it, up to the
    Trainer's total: the scores and the gate per video (dcf_op_sidekick / dcf_op_gate, compared with the recorded gate weights and
    mask), the product and the concatenation with the shallow features, vid_map through autograd.masked_conv1d, text_transformer, the
    first fusion, video_transformer, fuse_and_predict and loss.PointObjective.  Nothing is differentiated here: the caller calls
    backward() on `.total`.  `text_use(i, text)`: the tensor the i-th call of xattn_fusion sees in place of the text (0: the first
    fusion, 1 + l: pyramid level l of the second) -- to cut or to tell apart the uses of the shared text.
    -> outputs (logits1, logits2, offsets, masks), total, taps {vid_map, text, fused, fpn0..} (text and fused keep their gradient)"""
    A, lb = pkg.autograd, pkg._lib
    lib, st = lb.lib(), lb.current_stream()
    sizes = f.text_size
    D, T = f.vid.shape[1:]
    gates, masks, keep, q = [], [], [], 0
    for b, k in enumerate(sizes):                                   # one video and its k queries per call
        sh, cls, vm = f.shallow[b].cuda().contiguous(), f.text_cls[q:q + k].cuda().contiguous(), f.vid_masks[b].cuda().contiguous()
        correl = torch.empty(k, T, device='cuda')
        lb.check(lib.dcf_op_sidekick(lb.ptr(sh), lb.ptr(cls), lb.ptr(correl), D, T, k, int(model.norm), st), 'dcf_op_sidekick')
        gate, mo = torch.empty(k, T, device='cuda'), torch.empty(k, T, dtype=torch.bool, device='cuda')
        lb.check(lib.dcf_op_gate(lb.ptr(correl), lb.ptr(vm), lb.ptr(gate), lb.ptr(mo), T, k, model.sn, float(model.sratio), int(model.msf), st),
                 'dcf_op_gate')
        gates.append(gate), masks.append(mo), keep.append((sh, cls, vm, correl))
        q += k
    gate, mask = torch.cat(gates), torch.cat(masks)
    if check_gate:
        assert torch.equal(gate.cpu() != 0, f.gate), 'gate weights'
        assert bool(((gate == 0) | (gate == 1)).all())
        assert torch.equal(mask.cpu(), f.mask_gated), 'mask after the gate'
    kv_size = torch.tensor(sizes, device='cuda')
    rep = lambda z: tm(z.cuda()).repeat_interleave(kv_size, dim=0)          # model.py:578-581: video b once per query
    x = rep(f.vid) * gate[..., None]
    if model.msf:
        x = torch.cat([x, rep(f.shallow)], dim=2)
    vid_map = A.masked_conv1d(x, mask, model.vid_map.conv.weight, model.vid_map.conv.bias)
    text, text_mask = A.text_transformer(f.tokens.cuda(), f.token_masks.cuda(), model.text_net)
    if text.requires_grad:
        text.retain_grad()
    inner, calls = A.xattn_fusion, []

    def fusion(vid, vid_mask, txt, *rest, **kw):
        calls.append(None)
        return inner(vid, vid_mask, text_use(len(calls) - 1, txt), *rest, **kw)

    if text_use is not None:
        A.xattn_fusion = fusion
    try:
        fused, fmask = A.xattn_fusion(vid_map, mask, text, text_mask, model.fusion, kv_size)
        fused.retain_grad()
        fpn, fpn_masks = A.video_transformer(fused, fmask, model.vid_net)
        if model.second_fusion:
            outputs = A.fuse_and_predict(fpn, fpn_masks, model, text=text, text_mask=text_mask, kv_size=kv_size)
        else:
            outputs = A.fuse_and_predict(fpn, fpn_masks, model)
    finally:
        A.xattn_fusion = inner
    assert text_use is None or len(calls) == 1 + (len(fpn) if model.second_fusion else 0)
    total = pkg.loss.PointObjective(f.opt(pkg))(outputs, f.targets.cuda())['total']
    taps = {'vid_map': vid_map, 'text': text, 'fused': fused, **{f'fpn{l}': y for l, y in enumerate(fpn)}}
    return SimpleNamespace(outputs=outputs, total=total, taps=taps, fpn_masks=fpn_masks, keep=keep)
