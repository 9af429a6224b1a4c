"""Every eval route of modeling.py through the shared marshalling helpers, in one place and on the smallest forward the model takes:
the tiny model of tests/test_gpu_select_videos.py, T = 16 (four levels: a multiple of 8; the coarsest level a multiple of win // 2 = 2;
two gate blocks of sn = 8), two videos of 13 and 16 valid clips with 2 and 1 queries.

1. The graph key.  ``forward(eval=True)`` and ``forward_videos`` on the same contiguous inputs with ``reuse_output_buffers``: the flat
   outputs of every call are the same tensor objects, and with graphs asked for the forward is captured once and then replayed.  A
   helper that silently copied an input or an output would hand the engine new pointers every call, and no call would replay.
2. The routes on one video: ``forward_window(gate=sel.gate)``, ``forward_selected`` and ``forward_videos_selected`` on a batch of one.
   What tests/test_gpu_select.py and tests/test_gpu_select_videos.py assert between them: masks exact, logits and offsets under the
   project's parity rule against the oracles (forward_parity.check holds the bound), the two selected routes bit-identical."""
import pytest
import torch

import forward_parity as P
import select_ref as S
import select_videos_ref as V
from conftest import load_pkg
from test_gpu_select_videos import _oracle, build, flat, same_bits, video_of

pytestmark = pytest.mark.gpu
T, LENS = 16, [(13, 2), (16, 1)]


@pytest.fixture(scope='module')
def tiny():
    pkg = load_pkg()
    opt, model, sd = build(pkg, V.KW3, None, V.WSEED3)
    inputs = [pkg.synth.make_inputs(64, T, vid_len, nq, 32, 5 + v, 700 + v) for v, (vid_len, nq) in enumerate(LENS)]
    videos = [video_of(model, inp) for inp in inputs]
    assert all(x.is_contiguous() for a in videos for x in (a[0], a[1], a[2], a[4]))
    oracles = [_oracle(sd, opt.model, inp, a, False) for inp, a in zip(inputs, videos)]
    return pkg, opt, model, inputs, videos, oracles


def check_against_the_oracle(what, out, oracle, nq):
    lg, of, mk = out
    y32, y64 = oracle
    assert len(lg) == len(of) == len(mk) == nq
    for q in range(nq):
        for l in range(4):
            assert torch.equal(y32[2][q][l], y64[2][q][l]) and torch.equal(mk[q][l].cpu(), y32[2][q][l]), (what, q, l)
    P.check(f'routes {what} logits', P.pool(lg), P.pool(y64[0]), P.pool(y32[0]))
    P.check(f'routes {what} offsets', P.pool(of), P.pool(y64[1]), P.pool(y32[1]))


def test_stable_inputs_and_reused_outputs_replay_one_graph(tiny):
    pkg, opt, model, inputs, videos, oracles = tiny
    a = videos[0]
    model.reuse_output_buffers = True
    try:
        assert model.graph_mode == 'auto'
        for route, call in (('forward', lambda: [model(*a, eval=True)]), ('forward_videos', lambda: model.forward_videos(videos))):
            model.graph_mode = 'auto'
            out = call()
            first = model._last_flat
            call()
            assert all(x is y for x, y in zip(model._last_flat, first)), f'{route}: new output buffers on a repeated call'
            assert model.graph_active() == 0                          # 'auto' launches a forward this small eagerly
            model.graph_mode = 'always'
            how = []
            for _ in range(3):
                out = call()
                how.append(model.graph_active())
                assert all(x is y for x, y in zip(model._last_flat, first))
            assert how == [0, 2, 1], f'{route}: {how} (eager, capture, replay): the pointers of a repeated call are not stable'
            assert model.last_feature_dtype == torch.float32
            for v, o in enumerate(out):                               # the replayed forward's values
                check_against_the_oracle(f'{route} v{v}', o, oracles[v], LENS[v][1])
    finally:
        model.reuse_output_buffers, model.graph_mode, model._out_cache = False, 'auto', {}
    assert model.numerics_status() & 1 == 0


def test_window_selected_and_videos_selected_on_one_video(tiny):
    pkg, opt, model, inputs, videos, oracles = tiny
    for v, (a, inp) in enumerate(zip(videos, inputs)):
        nq = LENS[v][1]
        assert min(S.gate_gaps(opt.model, inp['shallow_vid'], inp['vid_masks'], inp['text_cls'])) > S.GAP_MIN
        sel = model.select_clips(a[1], a[2], a[4])
        assert torch.equal(sel.gate.cpu(), S.oracle_gates(opt.model, inp['shallow_vid'], inp['vid_masks'], inp['text_cls']))
        assert 0 < sel.count <= LENS[v][0]
        window = model.forward_window(a[0], a[1], a[2], a[3], a[5], sel.gate)
        one = model.forward_selected(model.gather_clip_rows(a[0], sel), sel, a[1], a[2], a[3], a[5])
        assert model.graph_active() == 0
        b1 = model.select_clips_videos([a])
        assert b1.counts == [sel.count] and torch.equal(b1.pos[0], sel.pos) and torch.equal(b1.gate, sel.gate)
        many = model.forward_videos_selected(model.gather_clip_rows_videos([a[0]], b1), b1, [a])
        assert model.graph_active() == 0 and model.last_feature_dtype == torch.float32
        assert len(many) == 1 and same_bits(flat(many[0]), flat(one)), v
        assert all(torch.equal(x, y) for qa, qb in zip(one[2], window[2]) for x, y in zip(qa, qb))           # masks
        for what, out in (('forward_window', window), ('forward_selected', one), ('forward_videos_selected', many[0])):
            check_against_the_oracle(f'{what} v{v}', out, oracles[v], nq)
    assert model.numerics_status() & 1 == 0
