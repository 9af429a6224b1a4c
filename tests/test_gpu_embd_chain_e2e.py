"""The embedding stage as one kernel inside a forward: T = 2 048, probe hyper-parameters (D = 1024, E = 256, L = 8, w = 9), with the
engine's row threshold lowered through dcf_debug_set_option('embd_chain_min_rows', 0) so that a forward of this size takes the kernel.

  * kernel on against kernel off ('embd_chain' = 0): masks equal, logits and offsets within 2e-5 (the project's bound against the
    oracle at scale shapes); the measured maxima are printed (`EMBDE2E`) and listed in profiles/embd_chain.md;
  * kernel on against the CPU oracle within the bound tests/test_gpu_e2e.py uses at this shape (BIG_TOL);
  * a four-video forward bit-identical, video by video, to four one-video forwards, the kernel on in both (and the dense GEMM's
    kernel choice pinned in both, 'gemm_uniform' = 1: it depends on the grid size otherwise);
  * where the gate must refuse -- gemm_mode 'bf16x6', vid_net.stride 2 -- the option changes no bit.

GPU only."""
import sys

import pytest
import torch

from conftest import ROOT, load_pkg
import embd_chain_cases as C

sys.path.insert(0, ROOT)
from oracle import decafnet_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = dict(rtol=2e-5, atol=2e-5)
KW = dict(D=1024, E=256, TE=256, text_in=128, n_levels=8, win=9, n_heads=4, sn=60, sratio=0.3, msf=True, norm=True,
          max_seq_len=1024, text_layers=2, text_max_len=48)
T, L = 2048, 8


def build(pkg, gemm_mode=None, **over):
    opt = pkg.config.make_opt(**dict(KW, **over))
    if gemm_mode:
        opt.model['gemm_mode'] = gemm_mode
    model = pkg.modeling.create_model(opt)
    sd = pkg.synth.make_state_dict({k: list(v.shape) for k, v in model.state_dict().items()}, 7)
    model.load_state_dict(sd)
    return opt, model.cuda().eval().requires_grad_(False), sd


def video(pkg, model, vid_len, nq, seed):
    inp = pkg.synth.make_inputs(1024, T, vid_len, nq, 128, 32, seed)
    tm = [model.encode_text(t[None].cuda(), torch.ones(1, 1, t.size(-1), dtype=torch.bool, device='cuda')) for t in inp['tokens']]
    return inp, (inp['vid'].cuda(), inp['shallow_vid'].cuda(), inp['vid_masks'].cuda(), tuple(t for t, _ in tm), inp['text_cls'].cuda(),
                 tuple(m for _, m in tm))


def clone(out):
    return tuple([[x.clone() for x in q] for q in part] for part in out)


class Options:
    """debug options for the length of a `with` block; they are process-wide"""
    def __init__(self, pkg, **opts):
        self.pkg, self.opts = pkg, opts

    def __enter__(self):
        C.set_options(self.pkg, **self.opts)

    def __exit__(self, *exc):
        C.set_options(self.pkg, **{k: -1 for k in self.opts})


@pytest.fixture(scope='module')
def probe():
    pkg = load_pkg()
    opt, model, sd = build(pkg)
    return dict(pkg=pkg, opt=opt, model=model, sd=sd)


def max_delta(a, b, part, nq):
    return max(float((a[part][q][l] - b[part][q][l]).abs().max()) for q in range(nq) for l in range(L))


def test_kernel_on_against_off_and_the_oracle(probe):
    pkg, model, sd, opt = probe['pkg'], probe['model'], probe['sd'], probe['opt']
    nq = 2
    inp, a = video(pkg, model, 1900, nq, 8)
    with Options(pkg, embd_chain_min_rows=0):
        on = clone(model(*a, eval=True))
    with Options(pkg, embd_chain=0):
        off = clone(model(*a, eval=True))
    assert model.numerics_status() & 1 == 0
    dl, do = max_delta(on, off, 0, nq), max_delta(on, off, 1, nq)
    print(f'EMBDE2E on-off T={T} nq={nq} max_abs_logit={dl:.3e} max_abs_offset={do:.3e}')
    assert dl > 0 or do > 0, 'the option did not change the launch sequence'
    for q in range(nq):
        for l in range(L):
            assert torch.equal(on[2][q][l], off[2][q][l])
            torch.testing.assert_close(on[0][q][l], off[0][q][l], **TOL)
            torch.testing.assert_close(on[1][q][l], off[1][q][l], **TOL)
    texts = [t.cpu() for t in a[3]]
    tmasks = [m.cpu() for m in a[5]]
    want = R.forward_eval(sd, opt.model, inp['vid'], inp['shallow_vid'], inp['vid_masks'], texts, inp['text_cls'], tmasks)
    cpu = tuple([[x.cpu() for x in q] for q in part] for part in on)
    print(f'EMBDE2E on-oracle T={T} nq={nq} max_abs_logit={max_delta(cpu, want, 0, nq):.3e} max_abs_offset={max_delta(cpu, want, 1, nq):.3e}')
    for q in range(nq):
        for l in range(L):
            assert torch.equal(cpu[2][q][l], want[2][q][l])
            torch.testing.assert_close(cpu[0][q][l], want[0][q][l], **TOL)
            torch.testing.assert_close(cpu[1][q][l], want[1][q][l], **TOL)


def test_four_videos_equal_four_one_video_forwards(probe):
    """Every output of a four-video forward equals, bit for bit, the one-video forward of the same video, the kernel on in both and
    taking both kinds of input rows in turn (LayerNorm carry on: the raw stream, the kernel normalises; off: normalised rows).
    'gemm_uniform' = 1 in both: at this shape a one-video forward has 2 048 level-0 rows and a four-video one 10 240, and the dense
    GEMM otherwise takes its k-sliced kernel -- K split over the waves, another summation order -- for the small grids only, which
    makes the two forwards differ by 2e-6 with this kernel and without it (profiles/embd_chain.md).  With the GEMM pinned, what is
    left to differ is the window and lane a row falls on in k_embd_chain (and in every other kernel of the forward)."""
    pkg, model = probe['pkg'], probe['model']
    videos = [video(pkg, model, vid_len, nq, 20 + v)[1] for v, (vid_len, nq) in enumerate([(2048, 1), (1500, 2), (2000, 1), (64, 1)])]
    try:
        for carry in (True, False):
            model.set_ln_carry(carry)
            with Options(pkg, embd_chain_min_rows=0, gemm_uniform=1):
                single = [clone(model(*a, eval=True)) for a in videos]
                multi = model.forward_videos(videos)
            assert model.numerics_status() & 1 == 0
            for v in range(4):
                for part in range(3):
                    assert len(multi[v][part]) == len(single[v][part])
                    for q in range(len(single[v][part])):
                        for l in range(L):
                            assert torch.equal(multi[v][part][q][l], single[v][part][q][l]), (carry, v, part, q, l)
    finally:
        model.set_ln_carry(True)


@pytest.mark.parametrize('case', ['bf16x6', 'stride2'])
def test_the_gate_refuses_and_nothing_changes(case):
    pkg = load_pkg()
    if case == 'bf16x6':
        opt, model, sd = build(pkg, gemm_mode='bf16x6')
    else:
        opt, model, sd = build(pkg, vid_stride=2)
    _, a = video(pkg, model, 1900, 1, 9)
    with Options(pkg, embd_chain_min_rows=0):
        on = clone(model(*a, eval=True))
    with Options(pkg, embd_chain=0):
        off = clone(model(*a, eval=True))
    for part in range(3):
        for l in range(len(on[part][0])):
            assert torch.equal(on[part][0][l], off[part][0][l]), (part, l)
