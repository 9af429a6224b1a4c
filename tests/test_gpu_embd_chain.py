"""The embedding stage as one kernel (dcf_op_embd_chain, include/decafnet_hip_embd.h) against the launch sequence it replaces
(dcf_op_embd_launches) and the fp64 restatement of tests/embd_chain_ref.py, on a finalized model's own parameters.

On the valid rows of every shape of embd_chain_cases.SHAPES, with and without a position encoding, with the kernel normalising its
rows (ln_in) and without:

    e_chain <= max(2 * e_launch, 2^-21 * max |ref|),   e = max |y - ref|

Both sides are f16x3 chains of the same length on the same inputs and the new one has one rounded intermediate fewer, so it should
not be worse; the factor 2 is the room two such chains have against each other.  Every check prints an `EMBDERR` line; the pairs
measured on an MI355X are in profiles/embd_chain.md.  Further: every padded row finite, 20 repeats bit-identical, the sticky range flag
clean -- and raised when an input row leaves the scaled fp16 operand range.  GPU only."""
import pytest
import torch

import embd_chain_cases as C
import embd_chain_ref as ER

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    pkg, model, sd, handle = C.make_model()
    return dict(pkg=pkg, model=model, handle=handle, params=ER.params_of(sd, C.E))


@pytest.mark.parametrize('ln_in', [1, 0])
@pytest.mark.parametrize('with_pe', [1, 0])
@pytest.mark.parametrize('B,T', C.SHAPES)
def test_chain_against_the_launches_and_fp64(ctx, B, T, with_pe, ln_in):
    pkg, model, handle, p = ctx['pkg'], ctx['model'], ctx['handle'], ctx['params']
    mask = C.masks_of(B, T, 100 + B * T)
    X = C.rows_of(B, T, ln_in, 7 + B + T, p)
    pe = torch.randn(T + 5, C.E, generator=torch.Generator().manual_seed(3)) if with_pe else None
    ref = ER.stage_unfolded(X, mask, p, bool(ln_in), pe)
    Xd, md, ped = X.cuda(), mask.cuda(), None if pe is None else pe.cuda()
    model.numerics_status(reset=True)
    Yl = torch.full((B, T, C.E), float('nan'), device='cuda')
    C.call(pkg, handle, 'dcf_op_embd_launches', Xd, md, ln_in, ped, Yl)
    runs = []
    for _ in range(20):
        Y = torch.full((B, T, C.E), float('nan'), device='cuda')
        C.call(pkg, handle, 'dcf_op_embd_chain', Xd, md, ln_in, ped, Y)
        runs.append(Y)
    assert model.numerics_status() & 1 == 0
    for Y in runs[1:]:
        assert torch.equal(Y.view(torch.int32), runs[0].view(torch.int32))
    got, launch = runs[0].cpu().double(), Yl.cpu().double()
    assert torch.isfinite(got).all()                          # the padded rows too: finite values nobody reads
    assert mask.any()
    e_chain = float((got - ref)[mask].abs().max())
    e_launch = float((launch - ref)[mask].abs().max())
    scale = float(ref[mask].abs().max())
    bound = max(2 * e_launch, 2.0 ** -21 * scale)
    print(f'EMBDERR B={B} T={T} pe={with_pe} ln_in={ln_in} e_chain={e_chain:.3e} e_launch={e_launch:.3e} max_ref={scale:.3e} bound={bound:.3e}')
    assert e_chain <= bound, (e_chain, e_launch, scale)


@pytest.mark.parametrize('ln_in', [1, 0])
def test_a_row_has_the_same_bits_alone_and_among_eight_sequences(ctx, ln_in):
    """the kernel is bit-identical to itself across batch sizes: sequence i of an eight-sequence call (its window seams fall elsewhere:
    T = 100 is no multiple of 124) equals the one-sequence call on the same rows, every row, padded ones included"""
    pkg, handle, p = ctx['pkg'], ctx['handle'], ctx['params']
    B, T = 8, 100
    mask = C.masks_of(B, T, 77)
    X = C.rows_of(B, T, ln_in, 78, p)
    pe = torch.randn(T, C.E, generator=torch.Generator().manual_seed(4)).cuda()
    Y8 = torch.full((B, T, C.E), float('nan'), device='cuda')
    C.call(pkg, handle, 'dcf_op_embd_chain', X.cuda(), mask.cuda(), ln_in, pe, Y8)
    for b in range(B):
        Y1 = torch.full((1, T, C.E), float('nan'), device='cuda')
        C.call(pkg, handle, 'dcf_op_embd_chain', X[b:b + 1].cuda(), mask[b:b + 1].cuda(), ln_in, pe, Y1)
        assert torch.equal(Y1[0].view(torch.int32), Y8[b].view(torch.int32)), b


def test_a_row_beyond_the_operand_range_raises_the_flag(ctx):
    """an input row scaled beyond the fp16 operand range (|x| * 2^4 > 65504): its products are not finite, the first LayerNorm's row
    sum sees it and the sticky word reports it, as the operand-range tests require of the other f16x3 kernels.  (With ln_in the rows
    are normalised before they are split: no input can leave the range.)"""
    pkg, model, handle, p = ctx['pkg'], ctx['model'], ctx['handle'], ctx['params']
    B, T = 2, 100
    mask = torch.ones(B, T, dtype=torch.bool)
    X = C.rows_of(B, T, 0, 5, p)
    X[1, 40] *= 1e4
    assert float(X[1, 40].abs().max()) > 4094
    model.numerics_status(reset=True)
    Y = torch.empty(B, T, C.E, device='cuda')
    C.call(pkg, handle, 'dcf_op_embd_chain', X.cuda(), mask.cuda(), 0, None, Y)
    assert model.numerics_status(reset=True) & 1 == 1
    C.call(pkg, handle, 'dcf_op_embd_chain', X.cuda(), mask.cuda(), 1, None, Y)      # normalised in the kernel: in range again
    assert model.numerics_status(reset=True) & 1 == 0
    assert torch.isfinite(Y).all()


def test_a_folded_weight_beyond_the_range_keeps_the_launch_path():
    """embd_fc and embd_convs.0 scaled so that each fits the scaled fp16 range (|w| < 255.9: the model stays in the f16x3 mode) and
    their folded product does not: the model builds no images, the one-kernel export says so, the launch sequence still runs"""
    def mutate(sd):
        sd['vid_net.embd_fc.conv.weight'] *= 20.0 / float(sd['vid_net.embd_fc.conv.weight'].abs().max())
        sd['vid_net.embd_convs.0.conv.weight'] *= 100.0 / float(sd['vid_net.embd_convs.0.conv.weight'].abs().max())

    pkg, model, sd, handle = C.make_model(seed=43, mutate=mutate)
    p = ER.params_of(sd, C.E)
    Wp, _ = ER.fold(p, False)
    assert float(Wp.abs().max()) > 256 and float(p['Wc'][0].abs().max()) < 255 and float(p['Wfc'].abs().max()) < 255
    assert model.numerics_status() & 4 == 0                  # (4 = the model fell back to bf16x6)
    B, T = 2, 64
    mask = C.masks_of(B, T, 5)
    X = C.rows_of(B, T, 0, 6, p).cuda()
    Y = torch.full((B, T, C.E), float('nan'), device='cuda')
    lib = pkg._lib.lib()
    rc = lib.dcf_op_embd_chain(handle, pkg._lib.ptr(X), C.E, pkg._lib.ptr(mask.cuda()), B, T, 0, None, pkg._lib.ptr(Y), C.E, pkg._lib.current_stream())
    assert rc == -1 and b'no images' in lib.dcf_last_error()
    C.call(pkg, handle, 'dcf_op_embd_launches', X, mask.cuda(), 0, None, Y)
    assert torch.isfinite(Y).all()
