"""The cases of the batch-assembly extension (include/decafnet_hip_batch.h, ``_lib.BATCH_TABLE``) for
tests/test_gpu_batch_assemble.py, in the format of tests/abi_cases.py: ``Case(export, tag, make, options)`` with ``make()`` ->
``(specs, call, None, verify)``; ``verify(outputs)`` compares ``out`` and ``mask`` with torch slicing on the CPU as integers -- the
operator is a copy, there is no tolerance.

The bank, ``desc``, ``out`` and ``mask`` are the operands between the borders.  A bank of 4-byte elements is placed as int32 bits, one
of 2-byte elements as the bytes of its rows (uint8, row pitch 2 C): what surrounds it then reads as half NaNs (fill 1) or zeros
(fill 2).  Every bank holds NaNs with non-default payload bits, negative NaNs and -0.0 among random bits.

Shapes: C in {1, 33, 64, 70} (a lone channel; odd, so that consecutive binary16 rows alternate between 4- and 2-byte alignment; one
tile of the fp32 kernel exactly; a second channel tile with a tail) times T_out in {1, 64, 65, 200} (a lone column; one fp32 tile; one
column past it, odd, so that binary16 output rows alternate likewise; a second tile of the binary16 kernel with a tail), both element
widths, and in each of them one window per n in {0, 1, 63, 64, 65, T_out} that fits T_out.  Window starts run 1, 4, 5, 8, ...: odd and
even first rows, windows that overlap, the largest ending on the bank's last row.  Then by name: binary16 with odd C and an odd first
row alone; B = 3 with two overlapping windows of one video and one ending on the last row of the bank's last video; n > T_out and
n < 0, which the operator clamps."""
import torch

from abi_cases import Case, gen, p

CASES = []
SPECIAL32 = (0x7fc12345, 0xffc01234 - (1 << 32), -0x80000000, 0x7f800001, 0x7fc00000)      # NaN payloads, a negative NaN, -0.0, a signalling NaN
SPECIAL16 = (0x7e01, 0xfe55, 0x8000, 0x7c01, 0x7e00)


def case(tag, make):
    CASES.append(Case('dcf_op_assemble_rows', tag, make, ()))


def bank_bits(g, rows, C, elem_bytes):
    """(rows, C) random bits with the special values scattered: int32, or int16 values in an int32 tensor"""
    if elem_bytes == 4:
        a = torch.randint(-2 ** 31, 2 ** 31, (rows, C), generator=g, dtype=torch.int64).to(torch.int32)
        special = SPECIAL32
    else:
        a = torch.randint(0, 2 ** 16, (rows, C), generator=g, dtype=torch.int64).to(torch.int32)
        special = SPECIAL16
    flat = a.view(-1)
    for i, s in enumerate(special):
        flat[(7 * i + 3) % flat.numel()] = s
    return a


def expected(bits, windows, C, T_out):
    """torch slicing on the CPU: -> (out (B, C, T_out) of the bank's integers, mask (B, T_out) uint8); n clamped to [0, T_out]"""
    out = torch.zeros(len(windows), C, T_out, dtype=bits.dtype)
    mask = torch.zeros(len(windows), T_out, dtype=torch.uint8)
    for b, (r0, n) in enumerate(windows):
        n = min(max(n, 0), T_out)
        out[b, :, :n] = bits[r0:r0 + n].t()
        mask[b, :n] = 1
    return out, mask


def as_bytes(bits16):
    """int16 values held in int32 -> their little-endian bytes, (..., 2 * last)"""
    return torch.stack((bits16 & 0xff, (bits16 >> 8) & 0xff), dim=-1).to(torch.uint8).flatten(-2)


def assemble(elem_bytes, C, T_out, windows, rows=None, with_mask=True):
    """windows: [(first row, n)]; the bank has ``rows`` rows (default: up to the end of the furthest window that is read)"""
    def make():
        g = gen(71, elem_bytes, C, T_out, len(windows), sum(r for r, _ in windows))
        B = len(windows)
        R = rows or max(max(r0 + min(max(n, 0), T_out) for r0, n in windows), 1)
        bits = bank_bits(g, R, C, elem_bytes)
        want_out, want_mask = expected(bits, windows, C, T_out)
        desc = torch.tensor([[r0 * C, n] for r0, n in windows], dtype=torch.int64)
        if elem_bytes == 4:
            specs = [('bank', bits, 'in'), ('desc', desc, 'in'), ('out', torch.zeros(B * C, T_out, dtype=torch.int32), 'out')]
            want_out = want_out.view(B * C, T_out)
        else:
            specs = [('bank', as_bytes(bits), 'in', 2 * C), ('desc', desc, 'in'),
                     ('out', torch.zeros(B * C, 2 * T_out, dtype=torch.uint8), 'out', 2 * T_out)]
            want_out = as_bytes(want_out).view(B * C, 2 * T_out)
        if with_mask:
            specs.append(('mask', torch.zeros(B, T_out, dtype=torch.uint8), 'out'))

        def call(c, v):
            return c.lib.dcf_op_assemble_rows(p(v['bank']), elem_bytes, p(v['desc']), B, C, T_out, p(v['out']), p(v.get('mask')), c.stream())

        def verify(got):
            assert got['out'].dtype == want_out.dtype and torch.equal(got['out'].cpu(), want_out), 'out differs from torch slicing'
            if with_mask:
                assert torch.equal(got['mask'].cpu().view(torch.uint8), want_mask), 'mask differs from t < n'
        return specs, call, None, verify
    return make


def _windows(T_out):
    ns = sorted({n for n in (0, 1, 63, 64, 65, T_out) if n <= T_out})
    return [(1 + 4 * (i // 2) + 3 * (i % 2), n) for i, n in enumerate(ns)]             # first rows 1, 4, 5, 8, 9, 12


for eb in (2, 4):
    for C in (1, 33, 64, 70):
        for T_out in (1, 64, 65, 200):
            case(f'e{eb}-C{C}-T{T_out}', assemble(eb, C, T_out, _windows(T_out)))
case('e2-C33-T65-odd-row-alone', assemble(2, 33, 65, [(3, 40)]))
case('e2-C33-T200-odd-row-alone', assemble(2, 33, 200, [(7, 200)], with_mask=False))
for eb in (2, 4):
    # one "video" of rows 0..89 with two overlapping windows, then the bank's last video, rows 90..129, read to its last row
    case(f'e{eb}-C70-T65-overlap-and-last-row', assemble(eb, 70, 65, [(10, 65), (40, 50), (90, 40)], rows=130))
    case(f'e{eb}-C33-T64-clamped', assemble(eb, 33, 64, [(1, 65), (2, 1 << 40), (3, -5), (0, 64)], rows=80))

EXCLUDED = {'dcf_batch_ext_version': 'no device operand: returns a constant'}
