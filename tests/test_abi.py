"""CPU checks of the drop-in boundary: the config struct equals the header's, the host module reproduces the reference's parameter
ABI, and the host-side text encoder / point generator match the reference fixtures.  (The header, the ctypes table and the exports
of the library: tests/test_abi_headers.py.)  No GPU, no compute calls."""
import os
import re
import sys

import pytest
import torch

from conftest import Golden, ROOT, load_pkg

HEADER = os.path.join(ROOT, 'include', 'decafnet_hip.h')


def test_config_struct_layout():
    pkg = load_pkg()
    src = open(HEADER).read()
    body = src[src.index('typedef struct dcf_config {'):src.index('} dcf_config;')]
    fields = re.findall(r'\b(?:int32_t|float)\s+(\w+)\s*;', body)
    assert fields == [f[0] for f in pkg._lib.DcfConfig._fields_]


@pytest.mark.parametrize('name', ['c1', 'pe', 'nomsf', 'scat', 'sfonly', 'affine', 'late', 'second', 'late_scat', 'early', 'early_single',
                                  'stride2', 'stride4', 'pool', 'pool_stride2'])
def test_parameter_abi_matches_reference(name):
    """state_dict keys and shapes == the reference model's (captured in the fixture)"""
    pkg = load_pkg()
    g = Golden(f'e2e_{name}.npz')
    if name.startswith('late'):
        model = pkg.modeling.PtTransformer(pkg.config.make_opt(**g.js('opt_kwargs')))
    elif name.startswith('early'):
        model = pkg.modeling.PtTransformerEarlyFusion(pkg.config.make_opt(**g.js('opt_kwargs')))
    else:
        model = pkg.modeling.create_model(pkg.config.make_opt(**g.js('opt_kwargs')))
    mine = {k: list(v.shape) for k, v in model.state_dict().items()}
    assert mine == g.js('shapes')
    opt = pkg.config.make_opt(**g.js('opt_kwargs'))
    before = repr(opt)
    pkg.modeling.create_model(opt)
    pkg.modeling.create_model(opt)
    assert repr(opt) == before, 'the constructor must not mutate opt (the reference does, model.py:426-428)'


def test_text_identity_parameter_abi():
    """opt.model.text_net.name == 'identity': state_dict keys / shapes of the reference (text_net.attn_pool.attn.*)"""
    pkg = load_pkg()
    g = Golden('text_identity.npz')
    model = pkg.modeling.create_model(pkg.config.make_opt(**g.js('model/opt_kwargs')))
    assert {k: list(v.shape) for k, v in model.state_dict().items()} == g.js('model/shapes')
    assert isinstance(model.text_net, pkg.modeling.TextIdentity)
    with pytest.raises(RuntimeError):
        model.text_net(torch.zeros(1, 32, 4), torch.ones(1, 1, 4, dtype=torch.bool))


def test_points_match_reference_and_text_encoder_has_no_cpu_path():
    pkg = load_pkg()
    g = Golden('e2e_c1.npz')
    meta, kw = g.js('meta'), g.js('opt_kwargs')
    model = pkg.modeling.create_model(pkg.config.make_opt(**kw)).eval()
    model.load_state_dict(pkg.synth.make_state_dict(g.js('shapes'), meta['wseed']))
    inp = pkg.synth.make_inputs(kw['D'], meta['T'], meta['vid_len'], meta['nq'], kw['text_in'], meta['lq'], meta['iseed'])
    tok = inp['tokens'][0]
    with pytest.raises(RuntimeError, match='MI355X'):       # the text encoder is dcf_text_encode (tests/test_gpu_e2e.py)
        model.encode_text(tok[None], torch.ones(1, 1, tok.size(-1), dtype=torch.bool))
    with pytest.raises(RuntimeError, match='parameter container'):
        model.text_net(tok[None], torch.ones(1, 1, tok.size(-1), dtype=torch.bool))
    pg = pkg.modeling.PtGenerator(kw['max_seq_len'] * 10, kw['n_levels'], 4, 0.5)
    pts = pg([meta['T'] >> l for l in range(kw['n_levels'])])
    for l, p in enumerate(pts):
        assert torch.equal(p, g.t(f'points/l{l}'))


def test_unsupported_switches_fail_loudly():
    pkg = load_pkg()
    kw = Golden('e2e_nomsf.npz').js('opt_kwargs')
    opt = pkg.config.make_opt(**kw)
    opt.model['name'] = 'default'
    with pytest.raises(NotImplementedError):
        pkg.modeling.create_model(opt)
    model = pkg.modeling.create_model(pkg.config.make_opt(**kw))
    # the training-mode forward computes forward values only: any dropout probability > 0 is refused (no random stream here)
    opt_d = pkg.config.make_opt(**kw)
    opt_d.model.vid_net['path_pdrop'] = 0.1
    with pytest.raises(NotImplementedError, match='path_pdrop'):
        pkg.modeling.create_model(opt_d)(torch.zeros(1, 64, 128), torch.zeros(1, 64, 128), torch.ones(1, 128, dtype=torch.bool),
                                         torch.zeros(1, 32, 4), torch.zeros(1, 64), torch.ones(1, 1, 4, dtype=torch.bool))
    with pytest.raises(RuntimeError, match='GPU'):   # ... and it runs on the MI355X only
        model(torch.zeros(1, 64, 128), torch.zeros(1, 64, 128), torch.ones(1, 128, dtype=torch.bool), torch.zeros(1, 32, 4), torch.zeros(1, 64),
              torch.ones(1, 1, 4, dtype=torch.bool))
    with pytest.raises(RuntimeError, match='GPU'):   # the single-head classes' training forward exists since round 5, on the GPU like the rest
        pkg.modeling.PtTransformer(pkg.config.make_opt(**kw))(torch.zeros(1, 64, 128), torch.zeros(1, 64, 128), torch.ones(1, 128, dtype=torch.bool),
                                                            torch.zeros(1, 32, 4), torch.zeros(1, 64), torch.ones(1, 1, 4, dtype=torch.bool))
    with pytest.raises(RuntimeError, match='GPU'):   # CPU tensors: no fallback
        model(torch.zeros(1, 64, 128), torch.zeros(1, 64, 128), torch.ones(1, 128, dtype=torch.bool), (), torch.zeros(0, 64), (), eval=True)


def test_product_never_imports_the_oracle():
    pk = os.path.join(ROOT, 'cvpr2025-decafnet_amd')
    for dirpath, _, files in os.walk(pk):
        for f in files:
            if f.endswith(('.py', '.hip', '.h', '.cpp')):
                txt = open(os.path.join(dirpath, f)).read()
                assert 'oracle' not in txt.replace('nms_oracle', 'oracle') or f == 'README', (f, 'mentions oracle')
    for f in ('nms_1d_cpu_vg/__init__.py',):
        assert 'oracle' not in open(os.path.join(ROOT, f)).read()


def test_padded_length_rule():
    pkg = load_pkg()
    ev = pkg.evaluator
    assert ev.min_chunk_size(8, 9) == 1024 and ev.min_chunk_size(6, 5) == 128
    assert ev.padded_length(1000, 2304, 8, 9) == 2304
    assert ev.padded_length(16000, 2304, 8, 9) == 16384
    assert ev.padded_length(16384, 2304, 8, 9) == 16384
    assert ev.padded_length(65530, 2304, 8, 9) == 65536


def test_metric_loop_matches_reference(tmp_path):
    """R@k / IoU counting (worker_v2.py:857-878) and the (T,C)->(C,T) feature loader against the reference fixture"""
    import numpy as np
    pkg = load_pkg()
    ev = pkg.evaluator
    g = Golden('postproc.npz')
    segs, scores = g.t('soft_novote/seconds'), g.t('soft_novote/scores')
    targets = [tuple(t.tolist()) for t in g.t('metric/targets')]
    c = ev.RecallCounter((1, 5), (0.3, 0.5))
    for tgt in targets:
        c.update([{'segments': segs, 'scores': scores}], [tgt])
    assert np.array_equal(c.counts, g.t('metric/counts').numpy())
    assert c.text_cnt == 3 and 'Rank@1, IoU@0.3' in c.report()
    idx = scores.argsort(descending=True)
    t0 = torch.as_tensor(targets[0]).expand(5, -1)
    torch.testing.assert_close(ev.iou(segs[idx[:5]], t0), g.t('metric/iou_topk')[0])
    a = np.random.RandomState(0).randn(7, 3).astype(np.float32)
    np.save(tmp_path / 'v.npy', a)
    f = ev.load_features(str(tmp_path / 'v'), 'npy')
    assert f.shape == (3, 7) and torch.equal(f, torch.from_numpy(a.T.copy()))


def test_no_packed_fp32_low_lane_from_high_dword():
    """ISA gate (profiles/r04_pkfma_hazard.md): no shipped object contains a packed fp32 instruction whose op_sel routes the high
    dword of a vector-register pair into the low lane -- the form that miscomputed in the LayerNorm-fold epilogue when the SLP
    vectoriser generated it"""
    import importlib.util
    spec = importlib.util.spec_from_file_location('isa_gate', os.path.join(ROOT, 'tools', 'isa_gate.py'))
    gate = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gate)
    if not os.path.exists(gate.OBJDUMP):
        pytest.skip('llvm-objdump not in this image')
    rep = gate.scan()
    assert rep, 'no objects under cvpr2025-decafnet_amd/build: run __graft_entry__.build() first'
    bad = {o: hits[:2] for o, (_, hits) in rep.items() if hits}
    assert not bad, f'packed fp32 with op_sel (low lane <- high dword) in {bad}'

