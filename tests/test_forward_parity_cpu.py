"""Pin the fp64 side of the forward's parity rule (tests/forward_parity.py): the CPU oracle run in fp64 against the reference's fp32
fixtures, same masks, same shapes, fp64 outputs.  CPU only.

Measured (profiles/forward_parity.md): logits, offsets and texts of every fixture within 3.3e-6 of the fp64 oracle; the vid_map taps
within 2.0e-6, the fused taps within 7.2e-6 (e2e_sfonly; max |fused| 5.3) -- all inside the 1e-5 of tests/test_oracle_golden.py.
"""
import pytest
import torch

import forward_parity as P

TOL = dict(rtol=1e-5, atol=1e-5)


def close64(tag, y64, y32):
    """every tensor of the fixture against the fp64 oracle at TOL; prints the pooled max |fixture - fp64|"""
    a, b = P.pool(y64), P.pool(y32)
    assert a.dtype == torch.float64 and a.shape == b.shape, tag
    print(f'FW64 {tag}: max|y64| {float(a.abs().max()):.3e} max|fixture - y64| {float((a - b).abs().max()):.3e}')
    torch.testing.assert_close(b, a, **TOL, msg=lambda m: f'{tag}: {m}')


@pytest.mark.parametrize('name', P.E2E + P.SECONDARY)
def test_fp64_oracle_matches_the_evaluation_fixtures(name):
    c = P.e2e_case(name)
    kinds = ['text', 'logits', 'offsets', 'vid_map', 'fused'] if name in P.E2E else ['logits', 'offsets']      # what the fixture holds
    assert set(kinds) == set(c.y32) <= set(c.y64)
    for kind in kinds:
        P.assert_fp64(c.y64[kind], kind)
        close64(f'e2e_{name} {kind}', c.y64[kind], c.y32[kind])


def test_fp64_oracle_matches_the_training_fixture():
    c = P.train_case()
    assert set(c.y64) == {'logits1', 'logits2', 'offsets'}
    for kind in c.y64:
        P.assert_fp64(c.y64[kind], kind)
        close64(f'train {kind}', c.y64[kind], c.y32[kind])


@pytest.mark.parametrize('name', P.TRAIN_SECONDARY)
def test_fp64_oracle_matches_the_single_head_training_fixtures(name):
    c = P.train_secondary_case(name)
    assert set(c.y64) == {'logits', 'offsets'}
    for kind in c.y64:
        P.assert_fp64(c.y64[kind], kind)
        close64(f'train_secondary {name} {kind}', c.y64[kind], c.y32[kind])


def test_fp64_oracle_matches_the_text_identity_fixture():
    for i, (c, y64, want) in enumerate(P.text_identity_cases()):
        P.assert_fp64(y64, f't{i}')
        close64(f'text_identity t{i}', y64, want)
    c = P.text_identity_model_case()
    for kind in ('text', 'logits', 'offsets'):
        P.assert_fp64(c.y64[kind], kind)
        close64(f'text_identity model {kind}', c.y64[kind], c.y32[kind])


def test_oracle64_refuses_a_downcast_and_leaves_masks_alone():
    sd = {'w': torch.ones(2, 2), 'n': torch.tensor([3])}
    got = P.to64([sd, torch.ones(2, dtype=torch.bool), (torch.ones(1),), 'late', [2, 1]])
    assert got[0]['w'].dtype == torch.float64 and got[0]['n'].dtype == torch.int64 and got[1].dtype == torch.bool
    assert got[2][0].dtype == torch.float64 and got[3] == 'late' and got[4] == [2, 1]
    P.assert_fp64(([torch.ones(1).double()], torch.ones(1, dtype=torch.bool)), 'ok')
    with pytest.raises(AssertionError):
        P.assert_fp64(([torch.ones(1).double(), [torch.ones(1)]],), 'downcast')


def test_the_rule(capsys):
    """check(): 4 x the reference's own error, or the 2^-21 floor where the reference is exact; non-finite results fail; the ratio is returned"""
    y64 = torch.tensor([1.0, -2.0, 0.5], dtype=torch.float64)
    y32 = y64 + torch.tensor([1e-6, 0.0, 0.0])
    assert P.check('four e_ref', y64 + torch.tensor([0.0, 3.9e-6, 0.0]), y64, y32) == pytest.approx(0.975)
    assert 'FWERR four e_ref: max|y64| 2.000e+00 e_ref 1.000e-06 e_gpu 3.900e-06 bound 4.000e-06 ratio 0.975' in capsys.readouterr().out
    with pytest.raises(AssertionError):
        P.check('beyond', y64 + torch.tensor([0.0, 4.1e-6, 0.0]), y64, y32)
    assert P.check('floor', y64 + 0.9 * P.FLOOR * 2.0, y64, y64) == pytest.approx(0.9)
    with pytest.raises(AssertionError):
        P.check('floor', y64 + 1.1 * P.FLOOR * 2.0, y64, y64)
    with pytest.raises(AssertionError):
        P.check('nan', torch.tensor([1.0, float('nan'), 0.5]), y64, y32)
    with pytest.raises(AssertionError):
        P.check('shape', y64[:2], y64, y32)
    assert P.pool([[torch.ones(1, 3)], [torch.zeros(2)]]).shape == (5,)
    assert P.pool([torch.arange(6.0).view(1, 2, 3)], [(slice(None), slice(None), torch.tensor([True, False, True]))]).tolist() == [0, 2, 3, 5]
