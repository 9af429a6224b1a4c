"""The forward kernels across the operand range of their fp16 planes: scaled activations and weights, values below the envelope,
unit-length features and tokens.  GPU only; the cases and what they presuppose are tests/operand_range_cases.py and
tests/test_operand_range_cpu.py.

Every case takes y64 from fp64 torch and y32 from fp32 torch on the CPU and is judged by the project's rule
(tests/forward_parity.py: e_gpu <= max(4 e_ref, 2^-21 max |y64|)) -- except section (b), below the envelope, where the rule is not
expected to hold and the kernel is held to the plane emulation of tests/f16x3_ref.py within 4 e_ref: it may lose what fp32
accumulation loses and nothing else.  Every check prints an `FWERR` line; the figures measured on an MI355X are in
profiles/operand_range.md.
"""
import ctypes
import functools

import pytest
import torch

from conftest import load_pkg
import forward_parity as FP
import operand_range_cases as C
from test_gpu_e2e import build, gate_logits_vs_oracle
from test_gpu_ops import P, scratch_model, st, tok

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def L():
    pkg = load_pkg()
    lib = pkg._lib.lib()          # raises if the .so is missing: no silent fallback
    return pkg, lib


# ---- (a), (b) the split GEMMs at op level ---------------------------------------------------------------------------------------
def run_gemm(L, c, nterms, A=None, bias=True):
    """the operator of case c on the GPU; A: other rows than the case's (conv3: another x), bias=False: without the bias"""
    pkg, lib = L
    dev = []                                                                  # alive until the synchronising .cpu() below

    def d(t):
        dev.append(t.contiguous().cuda())
        return P(dev[-1])

    b = d(c.bias) if bias and c.bias is not None else None
    if c.op == 'conv3':
        B, T, Cin, N = c.shape
        Y = torch.full((B * T + 1, N), float('nan'), device='cuda')
        pkg._lib.check(lib.dcf_op_conv3_split(P(tok(c.x if A is None else A)), d(c.mask.reshape(-1)), d(c.w3), P(Y), B, T, Cin, N, nterms, st()))
    else:
        M, N, K = c.shape
        A = c.A if A is None else A
        Y = torch.full((M + 1, N), float('nan'), device='cuda')
        if c.op == 'linear':
            pkg._lib.check(lib.dcf_op_linear_split(d(A), d(c.W), b, P(Y), M, N, K, 0, nterms, st()))
        else:
            pkg._lib.check(lib.dcf_op_linear_cm_split(d(A.t()), d(c.W), b, P(Y), M, N, K, nterms, st()))
    out = Y.cpu()
    assert bool(torch.isnan(out[-1]).all()), 'wrote beyond the last row'
    return out[:-1]


@pytest.mark.parametrize('nterms', [16, 6])
@pytest.mark.parametrize('op,shape', C.GEMM_SHAPES)
def test_split_gemm_over_the_operand_range(L, op, shape, nterms):
    """A * 2^s, W * 2^t and magnitudes mixed over 2^-12 .. 2^10 under the rule, in both split modes (bf16x6 also at 2^-20 and 2^20)"""
    for kind, e in C.variants(nterms):
        c = C.gemm_case(op, shape, kind, e)
        FP.check(f'oprange {op} {shape} n{nterms} {kind} 2^{e}', run_gemm(L, c, nterms), c.y64, c.y32)


@pytest.mark.parametrize('op,shape', C.GEMM_SHAPES)
def test_bf16x6_commutes_with_power_of_two_scaling_bit_for_bit(L, op, shape):
    """no bias: C(2^s A) == 2^s C(A) in every bit (bf16 planes carry fp32's exponent)"""
    c = C.gemm_case(op, shape, 'a', 0)
    base_in = c.x if op == 'conv3' else c.A
    base = run_gemm(L, c, 6, bias=False)
    for s in C.A_SCALES + C.WIDE_SCALES:
        if s:
            got = run_gemm(L, c, 6, A=base_in * 2.0 ** s, bias=False)
            assert torch.equal(got.view(torch.int32), (base * 2.0 ** s).view(torch.int32)), f'2^{s}: {int((got != base * 2.0 ** s).sum())} values differ'


@pytest.mark.parametrize('e', C.FLOOR_SCALES)
@pytest.mark.parametrize('op,shape', C.GEMM_SHAPES)
def test_f16x3_below_the_envelope_keeps_its_subnormal_planes(L, op, shape, e):
    """activations at 2^-12 and 2^-14: the low plane is fp16-subnormal throughout.  The result equals the emulation with subnormals
    KEPT (sa = 16, sw = 256) within 4 e_ref; flushed planes are more than 8 e_ref away from it (tests/test_operand_range_cpu.py)."""
    c = C.gemm_case(op, shape, 'a', e)
    got = run_gemm(L, c, 16).double()
    assert bool(torch.isfinite(got).all())
    d_kept, d_flush = float((got - c.emu).abs().max()), float((got - c.emu_flush).abs().max())
    print(f'FWERR oprange floor {op} {shape} a 2^{e}: e_ref {c.e_ref:.3e} |gpu - emu| {d_kept:.3e} = {d_kept / c.e_ref:.2f} e_ref '
          f'(|gpu - flushed emu| {d_flush / c.e_ref:.0f} e_ref, rule ratio {FP.rule(got, c.y64, c.y32)[4]:.2f})')
    assert d_kept <= 4 * c.e_ref


# ---- (c) chain kernels with scaled weights ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('t', C.CHAIN_SCALES)
def test_head_chain_with_scaled_weights(L, t):
    pkg, lib = L
    c = C.chain_case('head', t)
    B, T, Cc, NO = 2, 100, 256, 2
    d = {k: (v.to(torch.uint8) if k == 'mask' else v).cuda() for k, v in c.p.items()}
    valid = c.p['mask'].view(-1)
    for chain in (1, 0):
        out = torch.full((B * T + 1, NO), float('nan'), device='cuda')
        pkg._lib.check(lib.dcf_op_head(P(d['X']), P(d['mask']), P(d['W1']), P(d['l1w']), P(d['l1b']), P(d['W2']), P(d['l2w']), P(d['l2b']),
                                       P(d['Wo']), P(d['bo']), P(out), B, T, Cc, NO, 0.0, chain, st()))
        oc = out.cpu()
        assert torch.isnan(oc[B * T]).all(), 'wrote beyond the last row'
        FP.check(f'oprange head chain={chain} w 2^{t}', oc[:B * T][valid], c.y64[valid], c.y32[valid])


@pytest.mark.parametrize('t', C.CHAIN_SCALES)
def test_ffn_chain_with_scaled_weights(L, t):
    pkg, lib = L
    c = C.chain_case('ffn', t)
    M, E = c.p['X'].shape
    d = {k: (v.to(torch.uint8) if k == 'mask' else v).cuda() for k, v in c.p.items()}
    for chain in (1, 2, 3, 0):
        out = torch.full((M + 1, E), float('nan'), device='cuda')
        pkg._lib.check(lib.dcf_op_ffn(P(d['X']), P(d['lw']), P(d['lb']), P(d['W1']), P(d['b1']), P(d['W2']), P(d['b2']), P(d['ls']), P(d['mask']),
                                      P(out), None, M, E, chain, st()))
        oc = out.cpu()
        assert torch.isnan(oc[M]).all(), 'wrote beyond the last row'
        FP.check(f'oprange ffn chain={chain} w 2^{t}', oc[:M], c.y64, c.y32)


@pytest.mark.parametrize('t', C.CHAIN_SCALES)
def test_tcn_with_scaled_weights(L, t):
    pkg, lib = L
    c = C.chain_case('tcn', t)
    bs, n_in, T = c.p['x'].shape
    h = scratch_model(pkg, lib, c.p['w'], 'r')
    try:
        Y = torch.empty(bs * T, c.y64.size(1), device='cuda')
        pkg._lib.check(lib.dcf_op_tcn(h, b'r', P(tok(c.p['x'])), P(c.p['mask'].reshape(-1).contiguous().cuda()), bs, T, n_in, c.p['n_layers'], P(Y),
                                      st()), 'dcf_op_tcn')
        FP.check(f'oprange tcn w 2^{t}', Y.cpu(), c.y64, c.y32)
    finally:
        lib.dcf_model_destroy(h)


# ---- (d) the front end on reference-shaped features, (e) the text path ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def front_model(D):
    pkg = load_pkg()
    opt, model, sd = build(pkg, dict(C.FRONT_KW, D=D), None, 77)
    return pkg, opt, model, sd


def front_forward(pkg, model, inp, text, tmask, taps=()):
    """one forward; taps: 1 = gate (T,), 2 = vid_map, 3 = fused (E, T) of the one query, copied out as the header of dcf_debug_copy says"""
    T, E = C.FRONT_T, C.FRONT_KW['E']
    args = (inp['vid'].cuda(), inp['shallow_vid'].cuda(), inp['vid_masks'].cuda(), (text,), inp['text_cls'].cuda(), (tmask,))
    out = model(*args, eval=True)
    eng, lib = model._engine, model._engine.lib
    got = {}
    if 1 in taps:
        gate = torch.full((T,), float('nan'), device='cuda')
        pkg._lib.check(lib.dcf_debug_copy(eng.handle, 1, ctypes.c_void_p(gate.data_ptr()), gate.numel(), None))
        torch.cuda.synchronize()
        got[1] = gate.cpu()
    armed = {what: torch.empty(T, E, device='cuda') for what in taps if what in (2, 3)}
    if armed:
        for what, dst in armed.items():
            pkg._lib.check(lib.dcf_debug_copy(eng.handle, what, ctypes.c_void_p(dst.data_ptr()), dst.numel(), None))
        model(*args, eval=True)
        torch.cuda.synchronize()
        got.update({what: dst.t().cpu() for what, dst in armed.items()})
    return out, got


@pytest.mark.parametrize('kind', C.FRONT_KINDS)
@pytest.mark.parametrize('D', C.FRONT_DIMS)
def test_front_end_on_reference_shaped_features(D, kind):
    """unit-length clips, heavy-tailed non-negative unit-length clips, features at 2^-10 and at 2^10: the gate is the fp64 oracle's, and
    vid_map, the fusion output (valid clips) and the logits hold the rule against the fp32 / fp64 oracle"""
    from oracle import decafnet_ref as R
    pkg, opt, model, sd = front_model(D)
    c = C.front_case(D, kind)
    inp, cfg = c.inp, opt.model
    text, tmask = model.encode_text(inp['tokens'][0][None].cuda(), torch.ones(1, 1, inp['tokens'][0].size(-1), dtype=torch.bool, device='cuda'))
    (logits, offsets, masks), taps = front_forward(pkg, model, inp, text, tmask, taps=(1, 2, 3))
    n = int(inp['vid_masks'].sum())
    assert torch.equal(taps[1][:n], c.gate64[:n]), f'the gate differs from the fp64 oracle in {int((taps[1][:n] != c.gate64[:n]).sum())} clips'
    args = (inp['vid'], inp['shallow_vid'], inp['vid_masks'], [text.cpu()], inp['text_cls'], [tmask.cpu()])
    with torch.no_grad():
        i32 = R.forward_eval(sd, cfg, *args, return_intermediates=True)[3]['per_query'][0]
    i64 = FP.oracle64.forward_eval(sd, cfg, *args, return_intermediates=True)[3]['per_query'][0]
    valid = inp['vid_masks'][0]
    for what, key in ((2, 'vid_map'), (3, 'fused')):
        FP.check(f'oprange front D={D} {kind} {key}', taps[what][:, valid], i64[key][0][:, valid], i32[key][0][:, valid])
    gate_logits_vs_oracle(f'oprange front D={D} {kind}', sd, cfg, inp['vid'], inp['shallow_vid'], inp['vid_masks'], [text], inp['text_cls'], [tmask], logits)
    assert model.numerics_status() & 1 == 0


@pytest.mark.parametrize('kind', C.TEXT_KINDS)
def test_text_encoder_on_unit_length_and_scaled_tokens(kind):
    pkg, opt, model, sd = front_model(C.FRONT_DIMS[0])
    c = C.text_case(kind)
    got, m = model.encode_text(c.tok.cuda(), c.mask.cuda())
    assert torch.equal(m.cpu(), c.out_mask)
    FP.check(f'oprange text {kind}', got.cpu(), c.y64, c.y32)
    assert model.numerics_status() & 1 == 0


# ---- (f) attention cores ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('what,e', C.ATTN_VARIANTS)
@pytest.mark.parametrize('kind,shape', C.ATTN_SHAPES)
def test_attention_cores_on_scaled_operands(L, kind, shape, what, e):
    """q, k * 8 (the softmax saturates: the max subtraction), q, k * 2^-6 (near-uniform), v * 2^8, v * 2^-8

    `xattn (1, 70, 17, 128, 4) v 2^-8` is the case that found a bug: on UNSCALED fp16 planes of v (the low plane subnormal below
    2^-14, its absolute floor of 2^-25 undamped in the output) k_xattn_mfma missed the rule at ratio 3.165, the emulation of exactly
    that predicting 3.20.  The kernel now scales the planes of a small v (max |v| < 2^-2) by a power of two: 0.198
    (profiles/operand_range.md)."""
    c = C.attn_case(kind, shape, what, e)
    FP.check(f'oprange {kind} {shape} {what} 2^{e}', run_attn(L, c)[c.rows], c.y64[c.rows], c.y32[c.rows])


def run_attn(L, c):
    """the attention core of case c on the GPU -> (B*T, C) on the CPU"""
    pkg, lib = L
    q, k, v, m = c.q.cuda(), c.k.cuda(), c.v.cuda(), c.mask.cuda()
    rows, Cc = c.y64.shape
    O = torch.full((rows + 1, Cc), float('nan'), device='cuda')
    if c.kind == 'xattn':
        B, T, Lk, _, heads = c.shape
        pkg._lib.check(lib.dcf_op_xattn(P(q), P(k), P(v), P(m), P(O), B, T, Lk, Cc, heads, st()))
    else:
        B, T, _, heads, w = c.shape
        pkg._lib.check(lib.dcf_op_local_attn(P(q), P(k), P(v), P(m), P(O), B, T, Cc, heads, w, st()))
    Oc = O.cpu()
    assert torch.isnan(Oc[rows]).all(), 'wrote beyond the last row'
    return Oc[:rows]


def test_cross_attention_keeps_a_v_of_ordinary_size_on_unscaled_planes(L):
    """max |v| >= 2^-2 over the MFMA keys of a (batch, head): no plane scale, the arithmetic (and the bits) of unscaled planes.  The
    case (operand_range_cases.attn_unscaled_case) is `v 2^-8` with one element of 1.0 per head in a masked key, so that the two
    paths are far apart: the result equals the emulation of UNSCALED planes within 4 e_ref, and scaled planes are more than 8 e_ref
    from that (tests/test_operand_range_cpu.py).  The rule is not expected to hold here."""
    c = C.attn_unscaled_case()
    got = run_attn(L, c).double()
    assert bool(torch.isfinite(got).all())
    d_un, d_sc = float((got - c.emu_unscaled).abs().max()), float((got - c.emu_scaled).abs().max())
    print(f'FWERR oprange xattn unscaled path: e_ref {c.e_ref:.3e} |gpu - unscaled emu| {d_un:.3e} = {d_un / c.e_ref:.2f} e_ref '
          f'(|gpu - scaled emu| {d_sc / c.e_ref:.1f} e_ref, rule ratio {FP.rule(got, c.y64, c.y32)[4]:.2f})')
    assert d_un <= 4 * c.e_ref
