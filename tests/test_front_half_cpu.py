"""CPU checks that go with the half-feature training-front-end extension (include/decafnet_hip_front_half.h; its header and table:
tests/test_abi_headers.py): the names of ``_lib.FRONT_HALF_SIGNATURES`` and its parameters against the fp32 operators'; what the
two operators and ``autograd.gated_vid_map`` refuse before a GPU is touched; and, on the emulation of tests/f16x3_ref.py, the property
the half form of the weight-gradient kernel rests on: for binary16-representable features X the lo plane under the scale 2^4 is
exactly zero, so ``r_lo . x_hi + r_hi . x_hi`` equals the three-product sum bit for bit -- and for features that are not representable
it does not.  No GPU."""
import ctypes

import pytest
import torch

import abi_headers as H
from conftest import load_pkg
import f16x3_ref as F

NAMES = ['dcf_front_half_ext_version', 'dcf_op_vidmap_shared_bwd_h', 'dcf_op_vidmap_shared_h']
PAIRS = {'dcf_op_vidmap_shared_h': 'dcf_op_vidmap_shared', 'dcf_op_vidmap_shared_bwd_h': 'dcf_op_vidmap_shared_bwd'}


def params_of(name, header='decafnet_hip_front_half.h'):
    return H.params_of(header, name)[0]


# ---------------------------------------------------------------------------------------------- the ABI
def test_front_half_table_names_and_half_operands():
    pkg = load_pkg()
    table = pkg._lib.FRONT_HALF_SIGNATURES
    assert sorted(table) == NAMES
    assert 'front_grad.hip' in pkg.build.SOURCES                  # the operators live beside their fp32 forms: no new source file
    for name, base in PAIRS.items():
        assert table[name] == pkg._lib.FRONT_SIGNATURES[base], name
        mine, theirs = params_of(name), params_of(base, 'decafnet_hip_front.h')
        assert len(mine) == len(theirs)
        for p, q in zip(mine, theirs):                    # uint16_t exactly on vid and shallow; every other parameter as it was
            arg = p.split()[-1].lstrip('*')
            if arg in ('vid', 'shallow'):
                assert p == f'const uint16_t* {arg}' and q == f'const float* {arg}', (name, p, q)
            else:
                assert p == q, (name, p, q)
        assert [p for p in mine if 'nq' in p.split()[-1]] == ['const int32_t* nq']          # a HOST int32 array
    order = [p.split()[-1].lstrip('*') for p in params_of('dcf_op_vidmap_shared_h')]
    assert order == ['vid', 'shallow', 'W', 'bias', 'gate', 'mask', 'correl', 'nq', 'Y', 'nvid', 'D', 'T', 'E', 'flags', 'stream']
    order = [p.split()[-1].lstrip('*') for p in params_of('dcf_op_vidmap_shared_bwd_h')]
    assert order == ['vid', 'shallow', 'gate', 'mask', 'correl', 'nq', 'dY', 'dW', 'db', 'nvid', 'D', 'T', 'E', 'flags', 'accumulate', 'stream']


# ---------------------------------------------------------------------------------------------- refused before a launch
A = ctypes.c_void_p(4096)                                  # never dereferenced: the calls fail in their argument checks


@pytest.mark.parametrize('D,E,nq,null,msg', [
    (48, 64, [1], None, 'D = 48'),
    (32, 48, [1], None, 'E = 48'),
    (32, 64, [0], None, 'nq[0] = 0'),
    (32, 64, [1], 'W', 'null argument'),
    (32, 64, [1], 'Y', 'null argument'),
])
def test_the_half_forward_refuses_bad_operands_before_a_launch(D, E, nq, null, msg):
    pkg = load_pkg()
    lib = pkg._lib.lib()
    host_nq = (ctypes.c_int32 * len(nq))(*nq)
    ops = dict(W=A, Y=A)
    if null:
        ops[null] = None
    rc = lib.dcf_op_vidmap_shared_h(A, None, ops['W'], A, A, A, None, ctypes.cast(host_nq, ctypes.c_void_p), ops['Y'], 1, D, 1, E, 0, None)
    assert rc == -1
    err = lib.dcf_last_error().decode()
    assert 'dcf_op_vidmap_shared_h' in err and msg in err, err


@pytest.mark.parametrize('D,E,nq,null,msg', [
    (48, 64, [1], None, 'D = 48'),
    (32, 48, [1], None, 'E = 48'),
    (32, 64, [0], None, 'nq[0] = 0'),
    (32, 64, [1], 'dY', 'null argument'),
    (32, 64, [1], 'dW', 'null argument'),
])
def test_the_half_backward_refuses_bad_operands_before_a_launch(D, E, nq, null, msg):
    pkg = load_pkg()
    lib = pkg._lib.lib()
    host_nq = (ctypes.c_int32 * len(nq))(*nq)
    ops = dict(dY=A, dW=A)
    if null:
        ops[null] = None
    rc = lib.dcf_op_vidmap_shared_bwd_h(A, None, A, A, None, ctypes.cast(host_nq, ctypes.c_void_p), ops['dY'], ops['dW'], None, 1, D, 1, E, 0, 0, None)
    assert rc == -1
    err = lib.dcf_last_error().decode()
    assert 'dcf_op_vidmap_shared_bwd_h' in err and msg in err, err


@pytest.mark.parametrize('which', ['vid', 'shallow'])
def test_a_mixed_pair_into_gated_vid_map_is_a_value_error(which):
    """on CPU tensors: the dtype check comes before the device check"""
    pkg = load_pkg()
    nvid, D, T, E = 1, 32, 8, 32
    vid, shallow = torch.zeros(nvid, D, T), torch.zeros(nvid, D, T)
    gate, mask = torch.ones(1, T), torch.ones(1, T, dtype=torch.bool)
    w, b = torch.zeros(E, 2 * D, 1, requires_grad=True), torch.zeros(E, requires_grad=True)
    ops = dict(vid=vid, shallow=shallow)
    ops[which] = ops[which].half()
    with pytest.raises(ValueError, match='float16 clip features come as a pair'):
        pkg.autograd.gated_vid_map(ops['vid'], ops['shallow'], gate, mask, None, [1], w, b)
    with pytest.raises(RuntimeError, match='no CPU path'):        # a float16 pair passes the dtype check and meets the device check
        pkg.autograd.gated_vid_map(vid.half(), shallow.half(), gate, mask, None, [1], w, b)
    with pytest.raises(RuntimeError, match='no CPU path'):
        pkg.autograd.gated_vid_map(vid, shallow, gate, mask, None, [1], w, b)


def test_the_model_names_what_the_training_forward_read():
    pkg = load_pkg()
    assert pkg.modeling.PtTransformerEarlyFusionIterative.last_train_feature_dtype is None
    assert pkg.modeling.PtTransformerEarlyFusionIterative.half_features is True


# ---------------------------------------------------------------------------------------------- the plane property
SX = 16.0                                                  # FG_SX of csrc/front_grad.hip
N, C, T = 32, 64, 68


def _r(g):
    """R (T, N) = N(0, 1) 1e-3 -- not representable -- and the power-of-two scale that brings its maximum below 2^15"""
    R = torch.randn(T, N, generator=g) * 1e-3
    s = 2.0 ** (14 - int(torch.floor(torch.log2(R.abs().max()))))
    assert not torch.equal(R.half().float(), R) and 2.0 ** 14 <= float(R.abs().max()) * s < 2.0 ** 15
    return R, s


def _products(R, s, X):
    """dW (N, C) = R^T X^T on the planes, un-scaled: (the two products of the half form, the three of the fp32 form, the lo plane of X)"""
    rh, rl = F.split(R, s)
    xh, xl = F.split(X, SX)
    two = (rl.t() @ xh.t() + rh.t() @ xh.t()) / (s * SX)
    three = (rl.t() @ xh.t() + rh.t() @ xl.t() + rh.t() @ xh.t()) / (s * SX)
    return two, three, xl


@pytest.mark.parametrize('kind', ['normal', 'subnormal', 'zero-channel', 'large'])
def test_representable_features_have_no_lo_plane(kind):
    g = torch.Generator().manual_seed(31)
    R, s = _r(g)
    X = torch.randn(C, T, generator=g)
    if kind == 'subnormal':
        X = X * 2.0 ** -17
    elif kind == 'large':
        X = X * (4000.0 / float(X.abs().max()))
    X = X.half().float()                                   # binary16-representable
    if kind == 'zero-channel':
        X[5] = 0.0
    assert float(X.abs().max()) < 4094.0
    if kind == 'subnormal':
        assert int(((X != 0) & (X.abs() < F.F16_MIN_NORMAL)).sum()) > C * T // 2
    two, three, xl = _products(R, s, X)
    assert torch.equal(F.split(X, SX)[0], X.double() * SX), 'the hi plane is the stored value times 2^4'
    assert int((xl != 0).sum()) == 0, 'the lo plane of representable features is all zero'
    assert torch.equal(two, three), 'dropping r_hi . x_lo changes no bit'


def test_features_that_are_not_representable_need_their_lo_plane():
    g = torch.Generator().manual_seed(32)
    R, s = _r(g)
    X = torch.randn(C, T, generator=g)
    assert not torch.equal(X.half().float(), X)
    two, three, xl = _products(R, s, X)
    assert int((xl != 0).sum()) > X.numel() // 2
    assert not torch.equal(two, three)
    assert float((two - three).abs().max()) > 2.0 ** -14 * float(three.abs().max()), 'an error of fp16 size, not of fp32 size'
