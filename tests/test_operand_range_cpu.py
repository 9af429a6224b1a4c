"""The operand envelope of the f16x3 GEMM mode on the CPU emulation (tests/f16x3_ref.py), and what every case of
tests/test_gpu_operand_range.py presupposes.  CPU only.

1. The claims of the envelope comment in csrc/gemm_bf16s.hip, on the emulated planes.
2. Input preconditions: for every GPU case judged under the parity rule the emulation alone -- exact planes, products summed in fp64 --
   sits at rule_ratio <= 0.5, so that a GPU failure is the kernel's and not the inputs'.
3. Flush detectability: for every GPU case judged against the emulation, flushing the fp16 subnormals of the planes moves the result
   by more than 8 e_ref, twice what the GPU test allows, so a kernel that flushes is caught.
4. The gate of the front-end cases is no tie: the pooled scores of the last kept and the first dropped block differ by more than
   64 e_ref of the scores.
5. The rule and the floor check reject two wrong splits (activation planes under a scale of 1, the mid plane of A left out) when
   applied to the emulation with the defect built in.
"""
import math

import pytest
import torch

import f16x3_ref as X
import operand_range_cases as C


def _log_uniform(n, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return C._log_uniform((n,), lo, hi, g)


def _edges(lo, hi):
    """powers of two of the range, their neighbours in fp32 and the odd 24-bit patterns beside them"""
    p = torch.exp2(torch.arange(lo, hi, dtype=torch.float32))
    up, down = torch.nextafter(p, p * 2), torch.nextafter(p, p / 2)
    return torch.cat([p, up, down[1:], p * (1 + 2.0 ** -11), p * (1 + 2.0 ** -12), p * (2 - 2.0 ** -11), -p])


# (plane scale, first exponent with normal low planes, one past the last exponent in range, absolute floor below)
ENVELOPE = [('activations', 16.0, -7, 12, 2.0 ** -29), ('weights', 256.0, -11, 8, 2.0 ** -33), ('vid_map', 1.0, -3, 16, 2.0 ** -25)]


@pytest.mark.parametrize('name,s,lo,hi,floor', ENVELOPE)
def test_relative_plane_error_inside_the_envelope(name, s, lo, hi, floor):
    """2^lo <= |x| < the largest value that converts: |x - (hi + mid) / s| <= 2^-22 |x|"""
    top = X.F16_MAX / s * (1 - 2.0 ** -12)                  # 4094 / 255.9 / 65504 less the rounding margin of the hi plane
    x = torch.cat([_log_uniform(200000, lo, math.log2(top), 11), _edges(lo, hi)])
    x = x[(x.abs() >= 2.0 ** lo) & (x.abs() <= top)]
    hi_p, mid_p = X.split(x, s)
    assert bool(torch.isfinite(hi_p).all()) and bool(torch.isfinite(mid_p).all())
    rel = ((X.value(x, s) - x.double()).abs() / x.double().abs()).max()
    print(f'OPRANGE planes {name}: max relative error 2^{math.log2(float(rel)):.2f}')
    assert float(rel) <= 2.0 ** -22


@pytest.mark.parametrize('name,s,lo,hi,floor', ENVELOPE)
def test_absolute_plane_error_below_the_envelope(name, s, lo, hi, floor):
    """|x| < 2^lo: the error is the rounding to the fp16 subnormal grid of the low plane, 2^-25 / s at most"""
    x = torch.cat([_log_uniform(200000, lo - 40, lo, 12), _edges(lo - 30, lo), torch.zeros(1)])
    x = x[x.abs() < 2.0 ** lo]
    err = (X.value(x, s) - x.double()).abs().max()
    print(f'OPRANGE floor {name}: max absolute error 2^{math.log2(float(err)):.2f}')
    assert float(err) <= floor
    assert floor == 2.0 ** -25 / s
    # ... and a flushing split loses the whole low plane there: the comparison the GPU test rests on
    assert float((X.value(x, s, flush=True) - x.double()).abs().max()) > 64 * floor


@pytest.mark.parametrize('name,s,lo,hi,floor', ENVELOPE)
def test_values_of_22_bits_round_trip_exactly(name, s, lo, hi, floor):
    g = torch.Generator().manual_seed(13)
    m = torch.randint(2 ** 21, 2 ** 22, (100000,), generator=g).double()            # 22 significant bits
    e = torch.randint(lo - 21, hi - 22, (100000,), generator=g).double()
    x = (m * torch.exp2(e) * torch.where(torch.rand(100000, generator=g) < 0.5, -1.0, 1.0)).float()
    assert float(x.abs().min()) >= 2.0 ** lo and float(x.abs().max()) * s < X.F16_MAX
    assert torch.equal(X.value(x, s), x.double())


def test_bf16_planes_hold_24_bits_at_any_exponent():
    x = _log_uniform(100000, -100.0, 100.0, 14)
    a = X.split_bf16(x)
    assert torch.equal(a[0] + a[1] + a[2], x.double())


# ---- preconditions of the GPU cases ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('op,shape,kind,e', C.gemm_ids())
def test_gemm_cases_leave_the_kernel_half_the_bound(op, shape, kind, e):
    c = C.gemm_case(op, shape, kind, e)
    assert float(c.W.abs().max()) < C.W_MAX and (abs(e) >= 20 or float(c.A.abs().max()) <= C.A_MAX)
    r6 = X.rule_ratio(c.emu6, c.y64, c.y32)
    r16 = X.rule_ratio(c.emu, c.y64, c.y32) if (kind, e) in C.variants(16) else float('nan')
    print(f'OPRANGE emu {op} {shape} {kind} {e}: e_ref {c.e_ref:.3e} ratio f16x3 {r16:.3f} bf16x6 {r6:.3f}')
    assert r6 <= 0.5
    assert not r16 > 0.5


@pytest.mark.parametrize('e', C.FLOOR_SCALES)
@pytest.mark.parametrize('op,shape', C.GEMM_SHAPES)
def test_floor_cases_would_show_a_flush(op, shape, e):
    c = C.gemm_case(op, shape, 'a', e)
    moved = float((c.emu_flush - c.emu).abs().max())
    print(f'OPRANGE flush {op} {shape} a {e}: e_ref {c.e_ref:.3e} flushed - kept {moved:.3e} = {moved / c.e_ref:.1f} e_ref')
    assert moved > 8 * c.e_ref


@pytest.mark.parametrize('t', C.CHAIN_SCALES)
@pytest.mark.parametrize('name', list(C.CHAIN_FORWARD))
def test_chain_cases_leave_the_kernel_half_the_bound(name, t):
    c = C.chain_case(name, t)
    top = max(float(w.abs().max()) for w in C.chain_weights(c.p))
    r = X.rule_ratio(c.emu, c.y64, c.y32)
    print(f'OPRANGE emu {name} 2^{t}: max|w| {top:.3e} ratio {r:.3f}')
    assert top < C.W_MAX
    assert r <= 0.5


@pytest.mark.parametrize('what,e', C.ATTN_VARIANTS)
@pytest.mark.parametrize('kind,shape', C.ATTN_SHAPES)
def test_attention_cases_leave_the_kernel_half_the_bound(kind, shape, what, e):
    c = C.attn_case(kind, shape, what, e)
    r = X.rule_ratio(c.emu[c.rows], c.y64[c.rows], c.y32[c.rows])
    print(f'OPRANGE emu {kind} {shape} {what} 2^{e}: ratio {r:.3f}')
    assert r <= 0.5


@pytest.mark.parametrize('kind', C.FRONT_KINDS)
@pytest.mark.parametrize('D', C.FRONT_DIMS)
def test_front_cases_leave_the_kernel_half_the_bound_and_the_gate_is_no_tie(D, kind):
    c = C.front_case(D, kind)
    # the planes of the vid_map launches are unscaled (a_scale = 1): features at 2^-10 spend half the bound on representation alone --
    # and only that little because the bias of vid_map dominates its output; the product by itself is 2^-15 off in relative terms
    r = X.rule_ratio(c.vidmap_emu, c.vidmap64, c.vidmap32)
    print(f'OPRANGE emu vid_map D={D} {kind}: ratio {r:.3f}')
    assert r <= 0.5
    # the gate keeps the k blocks of the largest pooled score: the margin between the last kept and the first dropped one
    k = int(c.kw['sratio'] * c.pooled64.numel())
    ranked = c.pooled64.sort().values
    margin = float(ranked[-k] - ranked[-k - 1])
    e_ref = float((c.pooled32.double() - c.pooled64).abs().max())
    print(f'OPRANGE gate D={D} {kind}: margin {margin:.3e} = {margin / e_ref:.0f} e_ref')
    assert margin > 64 * e_ref


@pytest.mark.parametrize('kind', C.FRONT_KINDS)
@pytest.mark.parametrize('D', C.FRONT_DIMS)
def test_front_cases_leave_the_kernels_half_the_bound_downstream(D, kind):
    """the `fused` tap and the logits: the fp64 oracle with every dense convolution on planes (vid_map unscaled, the rest under 2^4 /
    2^8), judged as the GPU's taps are"""
    f = C.front_forward_case(D, kind)
    for key in ('fused', 'logits'):
        r = X.rule_ratio(*getattr(f, key))
        print(f'OPRANGE emu front D={D} {kind} {key}: ratio {r:.3f}')
        assert r <= 0.5


@pytest.mark.parametrize('kind', C.TEXT_KINDS)
def test_text_cases_leave_the_kernel_half_the_bound(kind):
    c = C.text_case(kind)
    assert float(c.tok.abs().max()) <= C.A_MAX and bool(torch.isfinite(c.y32).all())
    r = X.rule_ratio(c.emu, c.y64, c.y32)
    print(f'OPRANGE emu text {kind}: ratio {r:.3f}')
    assert r <= 0.5


def test_unscaled_v_case_tells_unscaled_planes_from_scaled_ones():
    """the spike in a masked key changes no reference value, takes the emulation to unscaled planes, and those are more than 8 e_ref
    (twice what the GPU test allows) from the scaled ones"""
    c = C.attn_unscaled_case()
    base = C.attn_case(c.kind, c.shape, 'v', -8)
    y64 = C.attn_forward(c.q, c.k, c.v, c.mask, c.heads, 0, torch.float64, False).reshape(c.y64.shape)
    assert torch.equal(y64, base.y64)
    assert float(c.v.abs().max()) >= 0.25
    forced = C.attn_forward(base.q, base.k, base.v, base.mask, base.heads, 0, torch.float64, True, vs_fixed=1.0).reshape(c.y64.shape)
    assert torch.equal(c.emu_unscaled, forced)
    moved = float((c.emu_unscaled - c.emu_scaled).abs().max())
    print(f'OPRANGE xattn unscaled - scaled v planes: {moved:.3e} = {moved / c.e_ref:.1f} e_ref')
    assert moved > 8 * c.e_ref


# ---- the assertions bite: two wrong splits, on the emulation ------------------------------------------------------------------------
def _gemm_mid_a_zeroed(c):
    """f16x3_ref.gemm with the mid plane of A left out"""
    ah, _ = X.split(c.A, X.SA)
    wh, wm = X.split(c.W, X.SW)
    return (ah @ wh.t() + ah @ wm.t()) / (X.SA * X.SW) + (c.bias.double() if c.bias is not None else 0.0)


@pytest.mark.parametrize('op,shape', C.GEMM_SHAPES)
def test_the_rule_and_the_floor_check_reject_two_wrong_splits(op, shape):
    """what tests/test_gpu_operand_range.py asserts of the GPU, applied to two wrong emulations: activation planes under a scale of 1
    instead of 2^4 miss the rule at a * 2^-8 and the floor check; planes without the mid plane of A miss the rule at every scale and
    the floor check.  (A kernel with either defect adds its accumulation error to these figures.)"""
    b = lambda c: c.bias.double() if c.bias is not None else 0.0
    c8 = C.gemm_case(op, shape, 'a', -8)
    r = X.rule_ratio(X.gemm(c8.A, c8.W, sa=1.0) + b(c8), c8.y64, c8.y32)
    print(f'OPRANGE wrong sa=1 {op} {shape} a -8: ratio {r:.2f}')
    assert r > 1
    for kind, e in C.variants(16):
        c = C.gemm_case(op, shape, kind, e)
        r = X.rule_ratio(_gemm_mid_a_zeroed(c), c.y64, c.y32)
        print(f'OPRANGE wrong mid=0 {op} {shape} {kind} {e}: ratio {r:.1f}')
        assert r > 1
    for e in C.FLOOR_SCALES:
        c = C.gemm_case(op, shape, 'a', e)
        d1 = float((X.gemm(c.A, c.W, sa=1.0) + b(c) - c.emu).abs().max())
        d0 = float((_gemm_mid_a_zeroed(c) - c.emu).abs().max())
        print(f'OPRANGE wrong floor {op} {shape} a {e}: sa=1 {d1 / c.e_ref:.0f} e_ref, mid=0 {d0 / c.e_ref:.0f} e_ref')
        assert d1 > 4 * c.e_ref and d0 > 4 * c.e_ref
