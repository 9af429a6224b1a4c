"""One entry per operator of the half-feature training-front-end extension (include/decafnet_hip_front_half.h,
``_lib.FRONT_HALF_SIGNATURES``) for tests/test_gpu_front_half_borders.py, in the format of tests/abi_cases.py:
``Case(export, tag, make, options)`` with ``make()`` -> ``(specs, call)``.

The half operands lie in the arena as the BYTES of their binary16 values, as in tests/half_abi_cases.py: a uint8 tensor of shape
(nvid D, 2 T) with the row pitch 2 T, so that what surrounds them reads as half NaNs (fill 1) or zeros (fill 2).  The gate, the mask and
the other operands are those of tests/front_abi_cases.py.

The forward on the split tile path at two videos of [3, 1] queries, D = 32, T = 136 (two gate tiles and a tail of eight clips),
E = 128, with ``shallow`` and ``correl``, under half_native = 2 (native, or the call fails); the forward on the upcast path at T = 65,
E = 64.  The backward at T = 136 with ``db`` and accumulate = 1 (16-byte loads of eight clips) and at T = 65 without ``db``, accumulate
= 0 (rows off the 16-byte grid, one clip in the second tile), both under half_native = 2: the backward never upcasts.  ``nq`` is a
host array: it is no operand of the arena."""
import torch

from abi_cases import Case, out, p, rn, gen
from front_abi_cases import _operands
from half_abi_cases import half_bytes

CASES = []
NATIVE = (('half_native', 2),)


def case(export, tag, make, options=()):
    CASES.append(Case(export, tag, make, tuple(options)))


def _half_operands(g, nq, D, T, E, shallow, correl):
    """the operands of front_abi_cases with ``vid`` / ``shallow`` as the bytes of their binary16 rounding"""
    specs, cin = _operands(g, nq, D, T, E, shallow, correl)
    specs = [(s[0], half_bytes(s[1].reshape(-1, T)), s[2], T * 2) if s[0] in ('vid', 'shallow') else s for s in specs]
    return specs, cin


def _forward(nq, D, T, E, shallow, correl):
    def make():
        g = gen(81, len(nq), sum(nq), D, T, E, shallow, correl)
        specs, cin = _half_operands(g, nq, D, T, E, shallow, correl)
        specs += [('W', rn(g, E, cin, scale=cin ** -0.5), 'in'), ('bias', rn(g, E), 'in'), ('Y', out(sum(nq) * T, E), 'out')]
        host_nq = torch.tensor(nq, dtype=torch.int32)

        def call(c, v):
            o = lambda n: p(v[n]) if n in v else None
            return c.lib.dcf_op_vidmap_shared_h(p(v['vid']), o('shallow'), p(v['W']), p(v['bias']), p(v['gate']), p(v['mask']), o('correl'),
                                                p(host_nq), p(v['Y']), len(nq), D, T, E, 0, c.stream())
        return specs, call
    return make


def _backward(nq, D, T, E, shallow, correl, with_db, accumulate):
    def make():
        g = gen(82, len(nq), sum(nq), D, T, E, shallow, correl, with_db, accumulate)
        specs, cin = _half_operands(g, nq, D, T, E, shallow, correl)
        specs.append(('dY', rn(g, sum(nq) * T, E, scale=1e-3), 'in'))
        role = 'inout' if accumulate else 'out'
        specs.append(('dW', rn(g, E, cin) if accumulate else out(E, cin), role))
        if with_db:
            specs.append(('db', rn(g, E) if accumulate else out(E), role))
        host_nq = torch.tensor(nq, dtype=torch.int32)

        def call(c, v):
            o = lambda n: p(v[n]) if n in v else None
            return c.lib.dcf_op_vidmap_shared_bwd_h(p(v['vid']), o('shallow'), p(v['gate']), p(v['mask']), o('correl'), p(host_nq), p(v['dY']),
                                                    p(v['dW']), o('db'), len(nq), D, T, E, 0, accumulate, c.stream())
        return specs, call
    return make


case('dcf_op_vidmap_shared_h', 'T136-E128-nq3_1-msf-scat-split', _forward([3, 1], 32, 136, 128, True, True), NATIVE)
case('dcf_op_vidmap_shared_h', 'T65-E64-nq3_1-msf-scat-upcast', _forward([3, 1], 32, 65, 64, True, True))
case('dcf_op_vidmap_shared_bwd_h', 'T136-E128-nq3_1-msf-scat-db-acc1', _backward([3, 1], 32, 136, 128, True, True, True, 1), NATIVE)
case('dcf_op_vidmap_shared_bwd_h', 'T65-E64-nq3_1-msf-scat-nodb-acc0', _backward([3, 1], 32, 65, 64, True, True, False, 0), NATIVE)

EXCLUDED = {'dcf_front_half_ext_version': 'no device operand: returns a constant'}
