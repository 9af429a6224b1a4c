"""CPU checks that go with the training extension (include/decafnet_hip_train.h; its header and table: tests/test_abi_headers.py):
the hand-written backward formulas of tests/step_grad_drop_ref.py equal torch autograd of their forwards in fp64, and the committed
fixtures are what their generator says.  No GPU, no compute calls."""
import os

import torch

from conftest import load_pkg
import philox_ref as P
import step_grad_drop_ref as R

def test_hand_written_backwards_equal_autograd_in_fp64():
    B, T, C, b0, seed = 2, 6, 8, 3, 0x1234567890ABCDEF
    g = torch.Generator().manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    keep = R.keep_rows(seed, P.site(P.G_STEM, 1, P.FFN_OUT), B, T, C, b0, 0.5)
    assert 0 < int(keep.sum()) < keep.numel()
    k = R.factor(keep, 0.5, torch.float64)
    dp = torch.tensor([0.0, float(P.scale(0.3))], dtype=torch.float64)               # one sample dropped, one kept
    m = torch.ones(B, T, dtype=torch.float64)
    m[1, 4:] = 0
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=1e-13, atol=1e-14)

    x, gy = rn(B, T, C).requires_grad_(), rn(B, T, C)
    (R.dropout(x, k) * gy).sum().backward()
    close(R.dropout_bwd(gy, k), x.grad)

    x = rn(B, T, C).requires_grad_()
    (R.gelu_dropout(x, k) * gy).sum().backward()
    close(R.gelu_dropout_bwd(x.detach(), gy, k), x.grad)

    for m_r, m_h in ((m, None), (None, m), (m, m), (None, None)):
        r, h, ls = rn(B, T, C).requires_grad_(), rn(B, T, C).requires_grad_(), rn(C).requires_grad_()
        (R.drop_residual(r, m_r, h, m_h, ls, k, dp) * gy).sum().backward()
        dr, dh, dls = R.drop_residual_bwd(gy, h.detach(), m_r, m_h, ls.detach(), k, dp)
        close(dr, r.grad), close(dh, h.grad), close(dls, ls.grad)
        assert bool((dh[0] == 0).all())


def test_fma32_is_a_single_rounding():
    """the fp32 fused multiply-add of the residual's restatement against exact rational arithmetic"""
    import numpy as np
    from fractions import Fraction
    g = np.random.RandomState(3)
    a, b, c = (g.randn(2000).astype(np.float32) for _ in range(3))
    c[:500] = (-(a[:500].astype(np.float64) * b[:500])).astype(np.float32)            # heavy cancellation
    a[500:600], c[600:700] = 0, 0
    got = R.fma32(a, b, c)
    for i in range(a.size):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        near = np.float32(float(exact))                                  # within one fp32 step of the correctly rounded value
        cands = (np.nextafter(near, np.float32(-np.inf)), near, np.nextafter(near, np.float32(np.inf)))
        best = min(cands, key=lambda w: (abs(Fraction(float(w)) - exact), int(np.float32(w).view(np.int32)) & 1))       # nearest, ties to even
        assert np.float32(best).view(np.int32) == got[i].view(np.int32) or (best == 0 and got[i] == 0), (i, a[i], b[i], c[i], got[i], best)


# ---------------------------------------------------------------------------------------------- the committed fixtures
import numpy as np  # noqa: E402
import pytest  # noqa: E402

from conftest import GOLDEN  # noqa: E402
import objective_cases as C  # noqa: E402
import objective_grad_ref as OR  # noqa: E402
import step_grad_ref as SR  # noqa: E402

DROP_CASES = ('drop_s1d', 'drop_s2d')          # tests/golden/step_grad_drop_<case>*.npz, in the layout step_grad_ref.Fixture reads
E_REF_CAP = 2.0 ** -15


@pytest.fixture(scope='module', params=DROP_CASES)
def f(request):
    return SR.Fixture(request.param)


def test_fixture_files_and_parameters(f):
    for suffix in SR.FILES:
        path = os.path.join(GOLDEN, f'step_grad_{f.name}{suffix}.npz')
        assert 0 < os.path.getsize(path) < 1 << 20, path
    model = f.model(load_pkg())
    names = [k for k, _ in model.named_parameters()]
    assert len(names) == f.meta['n_params'] and sorted(names) == sorted(f.gp['32']) == sorted(f.gp['64'])
    for k, p in model.named_parameters():
        assert f.gp['32'][k].shape == f.gp['64'][k].shape == p.shape and torch.equal(p.detach(), f.sd[k]), k
    assert not model.second_fusion and (f.meta['proj_pdrop'], f.meta['path_pdrop'], f.meta['refine_pdrop']) == (0.2, 0.3, 0.5)
    if f.name == 'drop_s1d':
        assert f.meta['level_lengths'] == [40, 20, 10] and model.vid_net.stride == 1 and not model.msf      # the last level: T % 4 != 0
    else:
        assert f.meta['level_lengths'] == [40, 20, 10] and f.meta['T'] == 80 and model.vid_net.stride == 2 and model.msf


def test_fixture_reference_error_and_non_zero_gradients(f):
    zero = 0
    for k, g64 in f.gp['64'].items():
        top, e_ref = f.top(k), float((f.gp['32'][k].double() - g64).abs().max())
        assert top > 0 and bool(torch.isfinite(g64).all()), k
        if k.endswith(SR.ZERO_BY_SYMMETRY):
            zero += 1
            continue
        assert float(g64.abs().max()) == top > 0, k                    # every parameter takes a non-zero gradient
        assert e_ref <= E_REF_CAP * top, (k, e_ref, top)
    assert zero > 0


def test_fixture_discrete_decisions_and_positive_points(f):
    kw, meta = f.opt_kwargs, f.meta
    for dt in (torch.float32, torch.float64):
        gate, mask = f.oracle_gate(dt)
        assert torch.equal(gate, f.gate) and torch.equal(mask, f.mask_gated), dt
    stride = kw['vid_stride']
    for l, m in enumerate(f.masks):
        assert torch.equal(m, f.mask_gated[:, ::stride << l]), l
    labels, gt = OR.annotate(meta['T'] // stride, f.L, kw['max_seq_len'], 4, 0.5, f.targets.tolist(), meta['center_sampling'], C.RADIUS)
    assert torch.equal(labels, f.labels) and torch.equal(gt, f.gt_offsets)
    pos = f.labels & torch.cat(f.masks, 1)
    lv = np.cumsum([0] + meta['level_lengths'])
    assert min(int(pos[:, lv[l]:lv[l + 1]].sum()) for l in range(f.L)) >= 1
    for t in ('32', '64'):
        assert int((OR.non_smooth(torch.cat(f.out[t]['offsets'], 1), f.gt_offsets) & pos).sum()) == 0 == meta['excluded'], t


def test_fixture_key_meets_the_drop_path_conditions(f):
    """no drop-path site drops all three rows, at least one drops a row, at least one keeps all three; the recorded kept counts are
    those of the stated stream"""
    nq = sum(f.text_size)
    keeps = [P.drop_path_keep(f.meta['seed'], s, nq, f.meta['path_pdrop']) for s in f.meta['path_sites']]
    assert len(keeps) == 10 and all(s & 15 in (P.PATH_ATTN, P.PATH_FFN) for s in f.meta['path_sites'])
    assert all(k.any() for k in keeps) and any(not k.all() for k in keeps) and any(k.all() for k in keeps)
    rate = {P.PROJ: 0.2, P.FFN_HID: 0.2, P.FFN_OUT: 0.2, P.PATH_ATTN: 0.3, P.PATH_FFN: 0.3, P.TCN: 0.5}
    for s in f.meta['sites']:
        shape, p = tuple(s['shape']), rate[s['site'] & 15]
        keep = P.drop_path_keep(f.meta['seed'], s['site'], shape[0], p) if len(shape) == 1 else P.dropout_mask(f.meta['seed'], s['site'], shape, p)
        assert int(keep.sum()) == s['kept'], s
