"""Which memory do the kernels touch?  Every operator export of the C ABI on operands between poisoned borders (tests/arena.py), at the
shapes of tests/abi_cases.py: a plain run on separately allocated tensors, an arena run with fill 1 (quiet NaN / mask bytes 0xFF /
integers 0x7f..ff) and one with fill 2 (the largest finite float / 0x00 / 0).  Every output of both arena runs must equal the plain run
bit for bit (the kernels are bit-deterministic from run to run, which the value tests assert), every border byte must still be its fill
and every input untouched.  GPU only; no tolerance anywhere.

What this cannot see: a stray read whose value a select discards, and the library's own scratch.  It bounds which memory can
influence a result or be written; it is no proof of memory safety (profiles/abi_borders.md)."""
import pytest
import torch

import abi_cases
import arena
import borders
from borders import ctx, export_test  # noqa: F401  (ctx: the module's fixture)
from conftest import load_pkg

pytestmark = pytest.mark.gpu

test_export_between_poisoned_borders = export_test('base')


def test_every_extension_has_a_row_of_the_borders_table():
    keys = [e.key for e in load_pkg()._lib.EXTENSIONS]
    assert sorted(keys) == sorted(list(borders.TABLE) + list(borders.NO_CASE_TABLE))


def test_every_export_is_assigned():
    """every dcf_ name of the signature table is either in the case table or excluded with a reason; a new export fails here until
    someone decides where it belongs"""
    pkg = load_pkg()
    names = [n for n in pkg._lib.SIGNATURES if n.startswith('dcf_')]
    assert len(names) == len(pkg._lib.SIGNATURES)
    covered = {c.export for c in abi_cases.CASES}
    excluded = abi_cases.EXCLUDED
    assert all(isinstance(r, str) and r.strip() and '\n' not in r for r in excluded.values())
    unassigned = [n for n in names if n not in covered and n not in excluded]
    assert not unassigned, f'exports neither in abi_cases.CASES nor in abi_cases.EXCLUDED: {unassigned}'
    assert not covered & set(excluded), f'both covered and excluded: {sorted(covered & set(excluded))}'
    stale = [n for n in list(covered) + list(excluded) if n not in pkg._lib.SIGNATURES]
    assert not stale, f'not in the signature table: {stale}'
    # the operator, loss, objective, optimizer, dropout and post-processing exports may not be excluded
    mandatory = [n for n in names if n.startswith(('dcf_op_', 'dcf_optim_'))] + [
        'dcf_sigmoid_focal_loss', 'dcf_ctr_iou_loss', 'dcf_sigmoid_focal_loss_grad', 'dcf_ctr_iou_loss_grad', 'dcf_annotate_points',
        'dcf_point_objective', 'dcf_point_objective_grad', 'dcf_collect_segments', 'dcf_collect_segments_ext', 'dcf_nms_1d', 'dcf_softnms_1d',
        'dcf_segment_voting', 'dcf_debug_dropout_keep']
    assert not [n for n in mandatory if n not in covered]
    # ... and only exports without a caller-owned device extent, or the forward / hybrid entry points, may be
    allowed = ('dcf_last_error', 'dcf_abi_version', 'dcf_model_', 'dcf_numerics_status', 'dcf_points_per_query', 'dcf_graph_active',
               'dcf_debug_set_option', 'dcf_debug_copy', 'dcf_profile_', 'dcf_calib_mfma_rate', 'dcf_forward_', 'dcf_text_encode', 'dcf_hybrid_phase')
    assert not [n for n in excluded if not n.startswith(allowed)]


# ---------------------------------------------------------------------------------------------- the engine's inputs
PROBE = dict(D=1024, E=256, TE=256, text_in=128, n_levels=8, win=9, n_heads=4, sn=60, sratio=0.3, msf=True, norm=True, max_seq_len=1024,
             text_layers=2, text_max_len=48)
PROBE_T, PROBE_LEN, PROBE_LQ = 2048, (1900, 1333), ((32, 19), (7, 25))


def _engine_specs():
    """two videos shorter than their padded T = 2048, two queries of different token counts each: everything the forward reads from
    the caller"""
    g = torch.Generator().manual_seed(8)
    D, T, C_t = PROBE['D'], PROBE_T, PROBE['text_in']
    specs = []
    for v, (vl, lqs) in enumerate(zip(PROBE_LEN, PROBE_LQ)):
        vid, shallow = torch.randn(1, D, T, generator=g), torch.randn(1, D, T, generator=g)
        vid[..., vl:] = 0
        shallow[..., vl:] = 0
        specs += [(f'vid{v}', vid, 'in', T * 4), (f'shallow{v}', shallow, 'in', T * 4), (f'mask{v}', (torch.arange(T) < vl).view(1, T), 'in'),
                  (f'cls{v}', torch.randn(len(lqs), D, generator=g), 'in')]
        for q, lq in enumerate(lqs):
            specs += [(f'tok{v}_{q}', torch.randn(1, C_t, lq, generator=g), 'in', lq * 4), (f'tmask{v}_{q}', torch.ones(1, 1, lq, dtype=torch.bool), 'in')]
    return specs


def _engine_run(model, v):
    """encode_text per query, model(..., eval=True) on video 0, forward_videos on both; -> the flat outputs of the two forwards"""
    videos = []
    for vi, lqs in enumerate(PROBE_LQ):
        tm = [model.encode_text(v[f'tok{vi}_{q}'], v[f'tmask{vi}_{q}']) for q in range(len(lqs))]
        videos.append((v[f'vid{vi}'], v[f'shallow{vi}'], v[f'mask{vi}'], tuple(t for t, _ in tm), v[f'cls{vi}'], tuple(m for _, m in tm)))
    model(*videos[0], eval=True)
    torch.cuda.synchronize()
    one = [x.clone() for x in model._last_flat]
    model.forward_videos(videos)
    torch.cuda.synchronize()
    return one + [x.clone() for x in model._last_flat]


def test_engine_inputs_between_poisoned_borders():
    """the whole forward at the probe configuration of test_probe_config_vs_oracle with vid, shallow_vid, vid_masks, the tokens handed to
    encode_text and text_cls placed in an arena as views: with both fills model._last_flat (logits, offsets, masks) of model(...,
    eval=True) and of forward_videos over two videos is bit-identical to the run on plain tensors, the borders keep their fill and the
    inputs their bits.  (The outputs are allocated inside modeling.py and stay there.)"""
    pkg = load_pkg()
    opt = pkg.config.make_opt(**PROBE)
    model = pkg.modeling.create_model(opt)
    model.load_state_dict(pkg.synth.make_state_dict({k: list(t.shape) for k, t in model.state_dict().items()}, 7))
    model = model.cuda().eval().requires_grad_(False)
    specs = _engine_specs()
    views, keep = arena.plain_operands(specs, 'cuda')
    plain = _engine_run(model, views)
    assert all(bool(torch.isfinite(x).all()) for x in plain if x.is_floating_point())
    assert model.numerics_status() & 1 == 0
    for fill in arena.FILLS:
        ar = arena.Arena('cuda', fill)
        for s in specs:
            ar.place(*s)
        v = ar.build()
        for name, t in v.items():               # the forward gets the arena's memory itself, not a copy
            assert ar.buf.data_ptr() < t.data_ptr() < ar.buf.data_ptr() + ar.buf.numel() and t.is_contiguous(), name
        got = _engine_run(model, v)
        names = ('logits', 'offsets', 'masks', 'logits (two videos)', 'offsets (two videos)', 'masks (two videos)')
        for name, a, b in zip(names, got, plain):
            assert a.shape == b.shape and torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8)), \
                f'fill {fill}: {name} differ from the run on plain tensors'
        ar.verify()
