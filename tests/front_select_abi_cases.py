"""One entry per operator of the selected-clip training extension (include/decafnet_hip_front_select.h, ``_lib.FRONT_SELECT_TABLE``) for
tests/test_gpu_front_select_borders.py, in the format of tests/abi_cases.py: ``Case(export, tag, make, options)`` with ``make()`` ->
``(specs, call)``.

The gate, the mask and the other operands are those of tests/front_abi_cases.py (T = 65: one clip past a gate tile, T % 4 != 0; T = 136:
two tiles and a tail of eight; one video of one query and two videos of [3, 1] queries; D = 32; E = 64, the fp32 tile GEMM of the
expert rows, or E = 128, the split row GEMM); the expert operand is ``rows``: the dense features gathered at the union of a video's
gate rows AND its mask (tests/front_select_ref.py), so the packed rows end where the border begins -- no capacity rows -- and a read
past row_first[nvid] is a read of the fill.  With and without ``shallow`` / ``correl``; the backward with db NULL and with accumulate
0 / 1.  The half operands lie in the arena as the BYTES of their binary16 values, as in tests/front_half_abi_cases.py; the backward
runs under half_native = 2 (it never upcasts), the forward's shallow product natively at E = 128 and upcast at E = 64.
``row_first`` and ``nq`` are host arrays: no operands of the arena."""
import torch

from abi_cases import Case, gen, out, p, rn
from front_abi_cases import _operands
from half_abi_cases import half_bytes
import front_select_ref as FS

CASES = []
NATIVE = (('half_native', 2),)


def case(export, tag, make, options=()):
    CASES.append(Case(export, tag, make, tuple(options)))


def _sel_operands(g, nq, D, T, E, shallow, correl, half):
    """the operands of front_abi_cases with the dense ``vid`` replaced by its packed rows and ``pos`` -> (specs, cin, row_first)"""
    specs, cin = _operands(g, nq, D, T, E, shallow, correl)
    ops = {s[0]: s[1] for s in specs}
    q_first = [sum(nq[:v]) for v in range(len(nq))]
    vid_masks = torch.stack([ops['mask'][q] for q in q_first]).bool()
    rows, first, pos, _, counts = FS.pack(ops['vid'], ops['gate'], vid_masks, nq)
    assert min(counts) >= 1
    new = [('rows', half_bytes(rows) if half else rows, 'in'), ('pos', pos, 'in')]
    for s in specs[1:]:
        new.append((s[0], half_bytes(s[1].reshape(-1, T)), s[2], T * 2) if half and s[0] == 'shallow' else s)
    return new, cin, first


def _forward(nq, D, T, E, shallow, correl, half):
    def make():
        g = gen(101, len(nq), sum(nq), D, T, E, shallow, correl, half)
        specs, cin, first = _sel_operands(g, nq, D, T, E, shallow, correl, half)
        specs += [('W', rn(g, E, cin, scale=cin ** -0.5), 'in'), ('bias', rn(g, E), 'in'), ('Y', out(sum(nq) * T, E), 'out')]
        host_nq, host_first = torch.tensor(nq, dtype=torch.int32), torch.tensor(first, dtype=torch.int32)
        name = 'dcf_op_vidmap_selected_h' if half else 'dcf_op_vidmap_selected'

        def call(c, v):
            o = lambda n: p(v[n]) if n in v else None
            return getattr(c.lib, name)(p(v['rows']), p(host_first), p(v['pos']), o('shallow'), p(v['W']), p(v['bias']), p(v['gate']),
                                        p(v['mask']), o('correl'), p(host_nq), p(v['Y']), len(nq), D, T, E, c.stream())
        return specs, call
    return make


def _backward(nq, D, T, E, shallow, correl, with_db, accumulate, half):
    def make():
        g = gen(102, len(nq), sum(nq), D, T, E, shallow, correl, with_db, accumulate, half)
        specs, cin, first = _sel_operands(g, nq, D, T, E, shallow, correl, half)
        specs.append(('dY', rn(g, sum(nq) * T, E, scale=1e-3), 'in'))
        role = 'inout' if accumulate else 'out'
        specs.append(('dW', rn(g, E, cin) if accumulate else out(E, cin), role))
        if with_db:
            specs.append(('db', rn(g, E) if accumulate else out(E), role))
        host_nq, host_first = torch.tensor(nq, dtype=torch.int32), torch.tensor(first, dtype=torch.int32)
        name = 'dcf_op_vidmap_selected_bwd_h' if half else 'dcf_op_vidmap_selected_bwd'

        def call(c, v):
            o = lambda n: p(v[n]) if n in v else None
            return getattr(c.lib, name)(p(v['rows']), p(host_first), p(v['pos']), o('shallow'), p(v['gate']), p(v['mask']), o('correl'),
                                        p(host_nq), p(v['dY']), p(v['dW']), o('db'), len(nq), D, T, E, accumulate, c.stream())
        return specs, call
    return make


def _tag(nq, T, E, shallow, correl):
    return f'T{T}-E{E}-nq{"_".join(map(str, nq))}-{"msf" if shallow else "nomsf"}{"-scat" if correl else ""}'


for T, E in ((65, 64), (136, 128)):
    for nq in ([1], [3, 1]):
        for shallow, correl in ((True, True), (True, False), (False, True), (False, False)):
            acc = int(shallow != correl)                             # accumulate 0 / 1 and db NULL / given spread over the variants
            half = (len(nq) == 1) == shallow                         # ... and so are the fp32 and the binary16 forms
            sfx = '_h' if half else ''
            case('dcf_op_vidmap_selected' + sfx, _tag(nq, T, E, shallow, correl), _forward(nq, 32, T, E, shallow, correl, half),
                 NATIVE if half and E == 128 else ())
            case('dcf_op_vidmap_selected_bwd' + sfx, _tag(nq, T, E, shallow, correl) + f'-{"db" if shallow else "nodb"}-acc{acc}',
                 _backward(nq, 32, T, E, shallow, correl, shallow, acc, half), NATIVE if half else ())

EXCLUDED = {'dcf_front_select_ext_version': 'no device operand: returns a constant'}
