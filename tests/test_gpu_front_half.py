"""GPU checks of the half-feature training-front-end operators (include/decafnet_hip_front_half.h) and of ``autograd.gated_vid_map``
on a float16 pair.  The contract is equality: every case takes the same binary16 values to the ``_h`` operator and, upcast, to the
fp32 operator of include/decafnet_hip_front.h and compares Y, dW and db with ``torch.equal`` (equal numbers; a zero may differ in
sign).  The fp32 results are asserted finite, so that the comparison is one of numbers.

That alone would let both paths be wrong together; the orientation case on exact small-integer data pins both to the fp64 integer answer
of tests/front_grad_ref.py bit for bit, and one case meets the project's rule  e_gpu <= max(4 e_ref, 2^-21 max |x_64|)  against the
fp64 restatement on the binary16-rounded features."""
import contextlib

import pytest
import torch

from conftest import load_pkg
import front_grad_ref as R
import test_gpu_front_grad as FG

pytestmark = pytest.mark.gpu
KINDS = ['normal', 'subnormal', 'zero-channel', 'large']
TILE = 64


@pytest.fixture(scope='module')
def pkg():
    return load_pkg()


@contextlib.contextmanager
def half_native(pkg, value):
    lb = pkg._lib
    lb.check(lb.lib().dcf_debug_set_option(b'half_native', value), 'dcf_debug_set_option')
    try:
        yield
    finally:
        lb.check(lb.lib().dcf_debug_set_option(b'half_native', -1), 'dcf_debug_set_option')


def features(g, kind, nvid, D, T):
    """(nvid, D, T) float16 on the CPU"""
    x = torch.randn(nvid, D, T, generator=g)
    if kind == 'subnormal':
        x = x * 2.0 ** -17                                 # mostly below 2^-14, down to the last bit 2^-24
    elif kind == 'large':
        x = x * (4000.0 / float(x.abs().max()))            # the fp32 operator's range under its scale 2^4: |x| < 4094
    x = x.half()
    if kind == 'zero-channel':
        x[:, 5] = 0
    if kind == 'subnormal':
        assert int(((x != 0) & (x.float().abs() < 2.0 ** -14)).sum()) > x.numel() // 2
    assert float(x.float().abs().max()) < 4094.0
    return x


class Operands:
    """one call's operands on the GPU.  Video b keeps clips of gate tile b % ntiles alone: every other tile of it is closed."""

    def __init__(self, kind, nvid, sizes, D, T, E, msf=True, scat=False, seed=41):
        g = torch.Generator().manual_seed(seed)
        self.nvid, self.sizes, self.D, self.T, self.E, self.msf, self.scat = nvid, sizes, D, T, E, msf, scat
        rows, ntiles = sum(sizes), (T + TILE - 1) // TILE
        self.vid = features(g, kind, nvid, D, T).cuda()
        self.shallow = features(g, kind, nvid, D, T).cuda() if msf else None
        gate, self.closed, q = torch.zeros(rows, T), [], 0
        for b, k in enumerate(sizes):
            lo = TILE * (b % ntiles)
            for j in range(k):
                a = min(lo + 8 + 4 * j, T - 1)
                gate[q, a:min(a + 16, lo + TILE, T)] = 1.0
                q += 1
            self.closed += [(b, TILE * f, min(TILE * f + TILE, T)) for f in range(ntiles) if f != b % ntiles]
        mask = torch.ones(rows, T, dtype=torch.bool)
        mask[-1, T - T // 5:] = False
        cin = D * (2 if msf else 1) + int(scat)
        self.gate, self.mask = gate.cuda(), mask.cuda()
        self.correl = torch.randn(rows, T, generator=g).cuda() if scat else None
        self.W = (torch.randn(E, cin, generator=g) * 0.1).cuda()
        self.bias = (torch.randn(E, generator=g) * 0.1).cuda()
        self.dY = (torch.randn(rows, T, E, generator=g) * 1e-3).cuda()
        self.nq = torch.tensor(sizes, dtype=torch.int32)          # a HOST array, held for the calls

    def other_content(self):
        """(vid, shallow) with other finite halves in the closed tiles of vid"""
        vid = self.vid.clone()
        for i, (b, t0, t1) in enumerate(self.closed):
            vid[b, :, t0:t1] = 777.0 if i % 2 == 0 else -555.0
        assert not self.closed or not torch.equal(vid, self.vid)
        return vid


def forward(pkg, o, half, flags=0, vid=None):
    lb = pkg._lib
    cast = (lambda z: z) if half else (lambda z: None if z is None else z.float())
    v, sh = cast(o.vid if vid is None else vid), cast(o.shallow)
    y = torch.full((sum(o.sizes), o.T, o.E), float('nan'), device='cuda')
    name = 'dcf_op_vidmap_shared_h' if half else 'dcf_op_vidmap_shared'
    rc = getattr(lb.lib(), name)(lb.ptr(v), lb.ptr(sh), lb.ptr(o.W), lb.ptr(o.bias), lb.ptr(o.gate), lb.ptr(o.mask), lb.ptr(o.correl), lb.ptr(o.nq),
                                 lb.ptr(y), o.nvid, o.D, o.T, o.E, flags, lb.current_stream())
    lb.check(rc, name)
    return y


def backward(pkg, o, half, flags=0, vid=None, shallow=None, dY=None, with_db=True, onto=None):
    """-> (dW, db or None); ``onto`` = (dW, db): accumulate = 1 onto copies of them"""
    lb = pkg._lib
    cast = (lambda z: z) if half else (lambda z: None if z is None else z.float())
    v, sh = cast(o.vid if vid is None else vid), cast(o.shallow if shallow is None else shallow)
    dw = torch.full_like(o.W, float('nan')) if onto is None else onto[0].clone()
    db = None if not with_db else torch.full_like(o.bias, float('nan')) if onto is None else onto[1].clone()
    name = 'dcf_op_vidmap_shared_bwd_h' if half else 'dcf_op_vidmap_shared_bwd'
    rc = getattr(lb.lib(), name)(lb.ptr(v), lb.ptr(sh), lb.ptr(o.gate), lb.ptr(o.mask), lb.ptr(o.correl), lb.ptr(o.nq),
                                 lb.ptr(o.dY if dY is None else dY), lb.ptr(dw), lb.ptr(db), o.nvid, o.D, o.T, o.E, flags, int(onto is not None),
                                 lb.current_stream())
    lb.check(rc, name)
    return dw, db


def same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------- the forward
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('nvid,sizes,D,T,E', [(2, [2, 1], 64, 136, 128), (4, [1, 2, 1, 1], 32, 136, 128)], ids=['two-videos', 'grid-of-three-and-one'])
def test_the_native_forward_equals_the_fp32_operator(pkg, kind, nvid, sizes, D, T, E):
    """E % 128 == 0, T % 4 == 0: the split tile path reads the halves (half_native = 2: or the call fails)"""
    o = Operands(kind, nvid, sizes, D, T, E, scat=True)
    assert o.closed
    y32 = forward(pkg, o, False)
    assert bool(torch.isfinite(y32).all())
    with half_native(pkg, 2):
        y = forward(pkg, o, True)
        assert torch.equal(y, y32)
        assert torch.equal(forward(pkg, o, True, flags=pkg._lib.FRONT_NO_SKIP), y)
        assert torch.equal(forward(pkg, o, True, vid=o.other_content()), y)
    with half_native(pkg, 0):                              # the upcast path of the same shape
        assert torch.equal(forward(pkg, o, True), y32)


@pytest.mark.parametrize('kind', KINDS)
def test_the_upcast_forward_equals_the_fp32_operator(pkg, kind):
    """T % 4 != 0 and E % 128 != 0: the features are upcast into scratch; half_native = 2 refuses that before a launch"""
    o = Operands(kind, 2, [2, 1], 64, 70, 96, scat=True)
    y32 = forward(pkg, o, False)
    assert bool(torch.isfinite(y32).all())
    with half_native(pkg, 1):
        y = forward(pkg, o, True)
        assert torch.equal(y, y32)
        assert torch.equal(forward(pkg, o, True, flags=pkg._lib.FRONT_NO_SKIP), y)
        assert torch.equal(forward(pkg, o, True, vid=o.other_content()), y)
    with half_native(pkg, 2):
        with pytest.raises(RuntimeError, match=r'dcf_op_vidmap_shared_h.*half_native = 2 forbids the upcast'):
            forward(pkg, o, True)


# ---------------------------------------------------------------------------------------------- the backward
BACKWARD = {
    'T136': dict(D=64, T=136, E=128),                      # 16-byte loads; three 64-clip slices per video, the last of eight clips
    'T70': dict(D=64, T=70, E=128),                        # rows off the 16-byte grid, a partial 32-clip chunk
    'T1': dict(D=32, T=1, E=32),
    'D96-E96': dict(D=96, T=70, E=96),                     # a partial 64 x 64 tile in both directions
    'no-shallow': dict(D=64, T=136, E=128, msf=False),
    'correl': dict(D=64, T=136, E=128, scat=True),
    'no-db': dict(D=64, T=136, E=128, with_db=False),
    'accumulate': dict(D=64, T=136, E=128, accumulate=True),
    'offset-pointer': dict(D=64, T=136, E=128, offset=True),
}


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('case', list(BACKWARD))
def test_the_half_backward_equals_the_fp32_operator(pkg, kind, case):
    kw = dict(BACKWARD[case])
    with_db, accumulate, offset = kw.pop('with_db', True), kw.pop('accumulate', False), kw.pop('offset', False)
    o = Operands(kind, 2, [2, 1], **kw)
    want = backward(pkg, o, False, with_db=with_db)
    assert all(z is None or bool(torch.isfinite(z).all()) for z in want)
    vid_h, shallow_h, keep = None, None, []
    if offset:                                             # the features one half behind a 16-byte boundary: address = 2 mod 16
        for z in (o.vid, o.shallow):
            buf = torch.zeros(z.numel() + 8, dtype=torch.float16, device='cuda')
            buf[1:1 + z.numel()] = z.reshape(-1)
            keep.append(buf)
        vid_h, shallow_h = (b[1:1 + o.vid.numel()].view(o.vid.shape) for b in keep)
        assert vid_h.data_ptr() % 16 == 2 and shallow_h.data_ptr() % 16 == 2
    with half_native(pkg, 2):                              # the backward is native for every shape: it never upcasts
        got = backward(pkg, o, True, vid=vid_h, shallow=shallow_h, with_db=with_db)
        assert same(got, want)
        assert same(backward(pkg, o, True, vid=vid_h, shallow=shallow_h, with_db=with_db), got), 'equal inputs give equal bits'
        assert same(backward(pkg, o, True, flags=pkg._lib.FRONT_NO_SKIP, with_db=with_db), got)
        assert same(backward(pkg, o, True, vid=o.other_content(), with_db=with_db), got)
        dw32, db32 = backward(pkg, o, True, dY=o.dY * 32.0, with_db=with_db)
        assert torch.equal(dw32, got[0] * 32.0) and (db32 is None or torch.equal(db32, got[1] * 32.0))
        if accumulate:
            dw2, db2 = backward(pkg, o, True, onto=got)
            assert torch.equal(dw2, got[0] * 2.0) and torch.equal(db2, got[1] * 2.0)
            assert same(backward(pkg, o, False, onto=want), (dw2, db2))


# ---------------------------------------------------------------------------------------------- both paths against an exact answer
def test_operand_orientation_on_exact_integer_data_in_half(pkg):
    """test_gpu_front_grad.test_operand_orientation_on_exact_integer_data with the features as float16: the integers are
    representable, every product and every sum is exact, and the result equals the fp64 integer answer bit for bit"""
    nvid, D, T, E, sizes = 2, 64, 70, 96, [2, 1]
    t, d, e = torch.arange(T), torch.arange(D), torch.arange(E)
    vid = ((3 * d[None, :, None] + 5 * t[None, None, :] + 7 * torch.arange(nvid)[:, None, None]) % 11 - 4).float()
    shallow = ((2 * d[None, :, None] + 3 * t[None, None, :] + torch.arange(nvid)[:, None, None]) % 7 - 2).float()
    assert torch.equal(vid.half().float(), vid) and torch.equal(shallow.half().float(), shallow)
    dY = ((5 * e[None, None, :] + 2 * t[None, :, None] + 3 * torch.arange(3)[:, None, None]) % 9 - 3).float()
    gate = ((t[None, :] // 8 + torch.arange(3)[:, None]) % 3 == 0).float()
    mask = torch.ones(3, T, dtype=torch.bool)
    mask[2, 50:] = False
    correl = ((t[None, :] + 2 * torch.arange(3)[:, None]) % 5 - 2).float()
    W = ((e[:, None] + 2 * torch.arange(2 * D + 1)[None, :]) % 5 - 2).float()
    bias = (e % 3 - 1).float()
    w, b = torch.nn.Parameter(W[:, :, None].cuda()), torch.nn.Parameter(bias.cuda())
    y = pkg.autograd.gated_vid_map(vid.half().cuda(), shallow.half().cuda(), gate.cuda(), mask.cuda(), correl.cuda(), sizes, w, b)
    assert all(z.dtype == torch.float16 for z in y.grad_fn.saved_tensors if z.shape == (nvid, D, T))
    y.backward(dY.cuda())
    y64 = R.shared_forward(vid.double(), shallow.double(), gate.double(), mask, correl.double(), sizes, W.double(), bias.double())
    dw64, db64 = R.shared_grads(vid.double(), shallow.double(), gate.double(), mask, correl.double(), sizes, dY.double())
    assert float(dw64.abs().max()) < 2 ** 24 and float(y64.abs().max()) < 2 ** 24
    assert torch.equal(y.detach().cpu().double(), y64)
    assert torch.equal(w.grad[:, :, 0].cpu().double(), dw64)
    assert torch.equal(b.grad.cpu().double(), db64)


def test_the_half_operators_meet_the_rule_against_the_fp64_restatement(pkg):
    """test_gpu_front_grad.test_the_split_tile_path_of_the_forward_products on binary16-rounded features: x_64 the fp64 restatement,
    e_ref the error of the dense formula evaluated by torch in fp32 on the CPU, both on the values the GPU read"""
    gen = torch.Generator().manual_seed(23)
    nvid, D, T, E, sizes = 2, 64, 136, 128, [2, 1]
    grid = lambda *s, scale=1.0: torch.round(torch.randn(*s, generator=gen) * scale * 1024) / 1024
    vid_h, shallow_h = torch.randn(nvid, D, T, generator=gen).half(), torch.randn(nvid, D, T, generator=gen).half()
    vid, shallow = vid_h.float(), shallow_h.float()
    correl, W, bias = grid(3, T), grid(E, 2 * D + 1, scale=0.1), grid(E, scale=0.1)
    dY = torch.randn(3, T, E, generator=gen) * 1e-3
    gate = torch.zeros(3, T)
    gate[0, 8:24], gate[1, 16:40], gate[2, 70:94] = 1.0, 1.0, 1.0          # video 0: tiles 1 and 2 closed; video 1: tiles 0 and 2
    mask = torch.ones(3, T, dtype=torch.bool)
    mask[2, 120:] = False
    c = lambda z: z.cuda()
    w, b = torch.nn.Parameter(c(W[:, :, None].clone())), torch.nn.Parameter(c(bias.clone()))
    with half_native(pkg, 2):
        y = pkg.autograd.gated_vid_map(c(vid_h), c(shallow_h), c(gate), c(mask), c(correl), sizes, w, b)
        y.backward(c(dY))
    d = lambda z: z.double()
    y64 = R.shared_forward(d(vid), d(shallow), d(gate), mask, d(correl), sizes, d(W), d(bias))
    dw64, db64 = R.shared_grads(d(vid), d(shallow), d(gate), mask, d(correl), sizes, d(dY))
    x32 = R.dense_input(vid, shallow, gate, correl, sizes)
    y32, (dw32, db32) = R.dense_forward(x32, mask, W, bias), R.dense_grads(x32, mask, dY)
    missed = [FG.check('half Y', y, y64, y32), FG.check('half dW', w.grad[:, :, 0], dw64, dw32), FG.check('half db', b.grad, db64, db32)]
    assert not [m for m in missed if m is not None], missed


# ---------------------------------------------------------------------------------------------- gated_vid_map
def test_gated_vid_map_keeps_the_float16_tensors_and_gives_the_fp32_bits(pkg):
    o = Operands('normal', 2, [2, 1], 64, 136, 128, scat=True)

    def once(vid, shallow, weight_grad=True):
        w = torch.nn.Parameter(o.W[:, :, None].clone(), requires_grad=weight_grad)
        b = torch.nn.Parameter(o.bias.clone())
        y = pkg.autograd.gated_vid_map(vid, shallow, o.gate, o.mask, o.correl, o.sizes, w, b)
        saved = y.grad_fn.saved_tensors
        y.backward(o.dY)
        return y.detach(), (None if w.grad is None else w.grad.clone()), b.grad.clone(), saved

    y32, dw32, db32, saved32 = once(o.vid.float(), o.shallow.float())
    assert not any(z.dtype == torch.float16 for z in saved32)
    with half_native(pkg, 2):
        y, dw, db, saved = once(o.vid, o.shallow)
        halves = [z for z in saved if z.dtype == torch.float16]
        assert sorted(z.data_ptr() for z in halves) == sorted((o.vid.data_ptr(), o.shallow.data_ptr())), 'saved as stored: no copy'
        assert not any(z.dtype == torch.float32 and z.shape == o.vid.shape for z in saved)
        assert torch.equal(y, y32) and torch.equal(dw, dw32) and torch.equal(db, db32)
        _, none, db_frozen, _ = once(o.vid, o.shallow, weight_grad=False)
        assert none is None and torch.equal(db_frozen, db)
    with pytest.raises(ValueError, match='float16 clip features come as a pair'):
        pkg.autograd.gated_vid_map(o.vid, o.shallow.float(), o.gate, o.mask, o.correl, o.sizes, torch.nn.Parameter(o.W[:, :, None].clone()),
                                   torch.nn.Parameter(o.bias.clone()))
