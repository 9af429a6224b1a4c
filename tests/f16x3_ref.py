"""CPU restatement of the operand split of the f16x3 GEMM mode (csrc/gemm_bf16s.hip, split2_f16) and of the bf16x6 mode beside it.

An fp32 operand x enters the fp16 matrix cores as two planes under a power-of-two scale s (activations 2^4, weights 2^8, the vid_map
launches take a scale of their own):

    hi = fp16(s x),   mid = fp16(fma(x, s, -hi))        round to nearest even, fp16 subnormals KEPT

and a product is  (hi_a hi_w + hi_a mid_w + mid_a hi_w) / (s_a s_w).  `gemm` sums these products of fp16 values in fp64, so what it
returns differs from the exact product by the REPRESENTATION error of the planes alone; the kernel adds what fp32 accumulation adds.
`flush=True` zeroes every fp16 subnormal of both planes: what a convert or a matrix core that flushes denormals would make of them.
"""
import torch

import forward_parity as P

SA, SW = 16.0, 256.0            # F16_SA, F16_SW of gemm_bf16s.hip
F16_MIN_NORMAL = 2.0 ** -14
F16_MAX = 65504.0


def _fp16(x64, flush):
    """fp64 values that are exact fp32 numbers -> fp16 (RTNE, subnormals kept or flushed) -> fp64"""
    h = x64.to(torch.float32).to(torch.float16)
    if flush:
        h = torch.where(h.abs().double() < F16_MIN_NORMAL, torch.zeros_like(h), h)
    return h.double()


def split(x, s, flush=False):
    """(hi, mid) of the fp32 tensor x under the power-of-two scale s, as fp64 tensors holding fp16 values"""
    x = x.to(torch.float32).double()
    hi_kept = _fp16(x * s, False)
    mid = _fp16(x * s - hi_kept, flush)          # the residual is exact in fp32 (and so in fp64) wherever s x is a normal fp32 number
    return (_fp16(x * s, flush) if flush else hi_kept), mid


def value(x, s, flush=False):
    """what the two planes stand for: (hi + mid) / s, fp64"""
    hi, mid = split(x, s, flush)
    return (hi + mid) / s


def gemm(A, W, sa=SA, sw=SW, flush=False):
    """A (M, K), W (N, K) fp32 -> (M, N) fp64: hh + hm + mh of the planes, summed in fp64, un-scaled"""
    ah, am = split(A, sa, flush)
    wh, wm = split(W, sw, flush)
    return (ah @ wh.t() + ah @ wm.t() + am @ wh.t()) / (sa * sw)


def split_bf16(x):
    """(hi, mid, lo) of the bf16x6 mode (split2): three bf16 roundings of the running residual, as fp64 tensors"""
    r = x.to(torch.float32)
    planes = []
    for _ in range(3):
        p = r.to(torch.bfloat16).to(torch.float32)
        planes.append(p.double())
        r = r - p                                # exact: the residual of an fp32 number against its bf16 rounding
    return planes


def gemm_bf16x6(A, W):
    """the six products with i + j <= 2 of the three bf16 planes, summed in fp64"""
    a, w = split_bf16(A), split_bf16(W)
    out = 0
    for i in range(3):
        for j in range(3 - i):
            out = out + a[i] @ w[j].t()
    return out


def rule_ratio(got, y64, y32):
    """e / bound of the project's parity rule (forward_parity.rule): e <= max(4 e_ref, FLOOR max |y64|)"""
    return P.rule(got, y64, y32)[4]


def e_ref(y64, y32):
    """max |y32 - y64|: the error of the fp32 CPU reference of a case"""
    return float((y32.double() - y64.double()).abs().max())
