"""One entry per operator of the training-front-end extension (include/decafnet_hip_front.h, ``_lib.FRONT_SIGNATURES``) for
tests/test_gpu_front_borders.py, in the format of tests/abi_cases.py: ``Case(export, tag, make, options)`` with ``make()`` ->
``(specs, call)``.

Both exports at T = 65 (one clip past a gate tile: the second tile holds one clip and 63 that must not be read; T % 4 != 0) and
T = 136 (two tiles and a tail of eight; T % 4 == 0, the 16-byte loads along T), with one video of one query and with two videos of
[3, 1] queries; with and without ``shallow``, with and without ``correl``; the backward with db NULL and with accumulate 0 / 1.
D = 32 and E = 64 (the generic channel-major GEMM) or E = 128 (the split tile path, T = 136 alone admits it).  The gate keeps blocks
of eight clips so that whole tiles stay closed; the mask has a padded tail.  ``nq`` is a host array: it is no operand of the arena."""
import torch

from abi_cases import Case, gen, out, p, rn

CASES = []


def case(export, tag, make):
    CASES.append(Case(export, tag, make, ()))


def _operands(g, nq, D, T, E, shallow, correl):
    nvid, rows = len(nq), sum(nq)
    gate = torch.zeros(rows, T)
    for q in range(rows):
        for t0 in range(8 * (q % 3), T, 40):                       # blocks of eight, 40 apart: tile 1 of T = 136 stays closed for some videos
            gate[q, t0:t0 + 8] = 1.0
    if T > 64:
        gate[:, 64:] = gate[:, 64:] * (torch.arange(rows)[:, None] % 2 == 0)
    mask = torch.ones(rows, T, dtype=torch.uint8)
    mask[-1, T - max(T // 5, 1):] = 0
    specs = [('vid', rn(g, nvid, D, T), 'in', T * 4)]
    if shallow:
        specs.append(('shallow', rn(g, nvid, D, T), 'in', T * 4))
    specs += [('gate', gate, 'in'), ('mask', mask, 'in')]
    if correl:
        specs.append(('correl', rn(g, rows, T), 'in'))
    return specs, D * (2 if shallow else 1) + int(correl)


def _forward(nq, D, T, E, shallow, correl):
    def make():
        g = gen(61, len(nq), sum(nq), D, T, E, shallow, correl)
        specs, cin = _operands(g, nq, D, T, E, shallow, correl)
        specs += [('W', rn(g, E, cin, scale=cin ** -0.5), 'in'), ('bias', rn(g, E), 'in'), ('Y', out(sum(nq) * T, E), 'out')]
        host_nq = torch.tensor(nq, dtype=torch.int32)

        def call(c, v):
            o = lambda n: p(v[n]) if n in v else None
            return c.lib.dcf_op_vidmap_shared(p(v['vid']), o('shallow'), p(v['W']), p(v['bias']), p(v['gate']), p(v['mask']), o('correl'),
                                              p(host_nq), p(v['Y']), len(nq), D, T, E, 0, c.stream())
        return specs, call
    return make


def _backward(nq, D, T, E, shallow, correl, with_db, accumulate):
    def make():
        g = gen(62, len(nq), sum(nq), D, T, E, shallow, correl, with_db, accumulate)
        specs, cin = _operands(g, nq, D, T, E, shallow, correl)
        specs.append(('dY', rn(g, sum(nq) * T, E, scale=1e-3), 'in'))
        role = 'inout' if accumulate else 'out'
        specs.append(('dW', rn(g, E, cin) if accumulate else out(E, cin), role))
        if with_db:
            specs.append(('db', rn(g, E) if accumulate else out(E), role))
        host_nq = torch.tensor(nq, dtype=torch.int32)

        def call(c, v):
            o = lambda n: p(v[n]) if n in v else None
            return c.lib.dcf_op_vidmap_shared_bwd(p(v['vid']), o('shallow'), p(v['gate']), p(v['mask']), o('correl'), p(host_nq), p(v['dY']),
                                                  p(v['dW']), o('db'), len(nq), D, T, E, 0, accumulate, c.stream())
        return specs, call
    return make


def _tag(nq, T, E, shallow, correl):
    return f'T{T}-E{E}-nq{"_".join(map(str, nq))}-{"msf" if shallow else "nomsf"}{"-scat" if correl else ""}'


for T in (65, 136):
    for nq in ([1], [3, 1]):
        for shallow, correl in ((True, True), (True, False), (False, True), (False, False)):
            case('dcf_op_vidmap_shared', _tag(nq, T, 64, shallow, correl), _forward(nq, 32, T, 64, shallow, correl))
            acc = int(shallow != correl)                             # accumulate 0 / 1 and db NULL / given spread over the variants
            case('dcf_op_vidmap_shared_bwd', _tag(nq, T, 64, shallow, correl) + f'-{"db" if shallow else "nodb"}-acc{acc}',
                 _backward(nq, 32, T, 64, shallow, correl, shallow, acc))
case('dcf_op_vidmap_shared', _tag([3, 1], 136, 128, True, True) + '-split', _forward([3, 1], 32, 136, 128, True, True))
case('dcf_op_vidmap_shared', _tag([1], 136, 128, False, False) + '-split', _forward([1], 32, 136, 128, False, False))
case('dcf_op_vidmap_shared_bwd', _tag([3, 1], 136, 128, True, True) + '-db-acc1', _backward([3, 1], 32, 136, 128, True, True, True, 1))
case('dcf_op_vidmap_shared_bwd', _tag([3, 1], 65, 64, True, True) + '-nodb-acc0', _backward([3, 1], 32, 65, 64, True, True, False, 0))

EXCLUDED = {'dcf_front_ext_version': 'no device operand: returns a constant'}
