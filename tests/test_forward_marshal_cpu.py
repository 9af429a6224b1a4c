"""The marshalling helpers of modeling.py that every engine forward goes through, on CPU tensors (no GPU, no library load):
``_text_table``, ``_video_tables``, ``_per_query_levels``, ``_alloc_outputs``, and the order of the refusals of the entry points.

What the helpers must keep: a tensor that is contiguous and of the engine's type goes to the engine AS ITSELF (the HIP graph of a
forward is keyed on the pointers, so a silent copy would end every replay); whatever had to be converted is held in ``keep``; the nested
outputs are views of the flat buffers; every refusal that needs no device comes before the "runs on the MI355X only" error."""
import pytest
import torch

from conftest import load_pkg

KW = dict(D=64, E=64, TE=32, text_in=32, n_levels=4, win=5, n_heads=4, sn=8, sratio=0.3, msf=True, norm=True, max_seq_len=128,
          text_layers=1, text_max_len=24)


def _model(**over):
    pkg = load_pkg()
    return pkg, pkg.modeling.create_model(pkg.config.make_opt(**dict(KW, **over)))


def _held(keep, ptr):
    return any(t is not None and t.data_ptr() == ptr for t in keep)


# ---------------------------------------------------------------------------------------------- _text_table
def test_text_table_passes_ready_tensors_as_themselves_and_holds_the_converted():
    M = load_pkg().modeling
    text = [torch.randn(32, 7), torch.randn(32, 5), torch.randn(9, 32).t(), torch.randn(32, 4, dtype=torch.float64)]
    masks = [torch.ones(1, 7, dtype=torch.bool), torch.ones(5, dtype=torch.bool), torch.ones(1, 9, dtype=torch.bool), torch.ones(1, 4)]
    assert not text[2].is_contiguous()
    tptr, mptr, tlen, keep = M._text_table(text, masks)
    assert len(tptr) == len(mptr) == len(tlen) == 4 and list(tlen) == [7, 5, 9, 4]
    for q in (0, 1):                                              # contiguous fp32 text, bool mask: no copy
        assert tptr[q] == text[q].data_ptr() and mptr[q] == masks[q].data_ptr()
    for q in (2, 3):                                              # non-contiguous / fp64 text: a converted copy, held
        assert tptr[q] != text[q].data_ptr() and _held(keep, tptr[q])
        got = next(t for t in keep if t.data_ptr() == tptr[q])
        assert got.dtype == torch.float32 and got.is_contiguous() and torch.equal(got, text[q].float())
    assert mptr[2] == masks[2].data_ptr()
    assert mptr[3] != masks[3].data_ptr() and _held(keep, mptr[3])            # a float mask becomes bool
    assert all(_held(keep, p) for p in list(tptr) + list(mptr))
    with pytest.raises(AssertionError):
        M._text_table([torch.randn(32, 7)], [torch.ones(1, 6, dtype=torch.bool)])
    with pytest.raises(AssertionError):
        M._text_table([torch.randn(1, 32, 7)], [torch.ones(1, 7, dtype=torch.bool)])


# ---------------------------------------------------------------------------------------------- _video_tables
def _videos(dtype, T=32, nqs=(2, 1)):
    g = torch.Generator().manual_seed(3)
    return [(torch.randn(1, 64, T, generator=g).to(dtype), torch.randn(1, 64, T, generator=g).to(dtype), torch.ones(1, T, dtype=torch.bool),
             tuple(torch.randn(1, 32, 5 + v + i, generator=g) for i in range(n)), torch.randn(n, 64, generator=g),
             tuple(torch.ones(1, 1, 5 + v + i, dtype=torch.bool) for i in range(n))) for v, n in enumerate(nqs)]


@pytest.mark.parametrize('dtype,half', [(torch.float32, False), (torch.float16, True)])
def test_video_tables_pass_ready_tensors_as_themselves(dtype, half):
    pkg, model = _model()
    videos = _videos(dtype)
    tb = model._video_tables(videos, half)
    assert list(tb.nqs) == [2, 1]
    for v, a in enumerate(videos):
        assert tb.vid[v] == a[0].data_ptr() and tb.shallow[v] == a[1].data_ptr()
        assert tb.mask[v] == a[2].data_ptr() and tb.cls[v] == a[4].data_ptr()
    # the flat text order is video-major, every entry the (TE, Lk) view of the caller's tensor
    want = [t for a in videos for t in a[3]]
    assert len(tb.text) == len(tb.text_masks) == 3
    assert all(x.shape == w.shape[1:] and x.data_ptr() == w.data_ptr() for x, w in zip(tb.text, want))
    assert all(x is w for x, w in zip(tb.text_masks, [m for a in videos for m in a[5]]))
    tptr, mptr, tlen, keep = pkg.modeling._text_table(tb.text, tb.text_masks)
    assert list(tptr) == [w.data_ptr() for w in want] and list(tlen) == [5, 6, 6]


def test_video_tables_upcast_float16_without_half_and_read_only_what_is_asked_for():
    pkg, model = _model()
    videos = _videos(torch.float16)
    tb = model._video_tables(videos, False)
    for v, a in enumerate(videos):
        for table, src in ((tb.vid, a[0]), (tb.shallow, a[1])):
            assert table[v] != src.data_ptr() and _held(tb.keep, table[v])
            got = next(t for t in tb.keep if t.data_ptr() == table[v])
            assert got.dtype == torch.float32 and torch.equal(got, src[0].float())
        assert tb.mask[v] == a[2].data_ptr() and tb.cls[v] == a[4].data_ptr()
    # a non-contiguous shallow_vid and an integer mask are converted and held
    sh = torch.randn(1, 32, 64).transpose(1, 2)
    tb = model._video_tables([(None, sh, torch.ones(32, dtype=torch.uint8), None, torch.zeros(3, 64), None)], False, vid=False, text=False)
    assert tb.vid is None and list(tb.nqs) == [3] and tb.text == [] and tb.shallow[0] != sh.data_ptr() and _held(tb.keep, tb.shallow[0])
    assert _held(tb.keep, tb.mask[0]) and next(t for t in tb.keep if t.data_ptr() == tb.mask[0]).dtype == torch.bool
    # without cls the counts are the texts'
    tb = model._video_tables(_videos(torch.float32, nqs=(1, 3)), False, vid=False, cls=False)
    assert tb.vid is None and tb.cls is None and list(tb.nqs) == [1, 3] and len(tb.text) == 4
    with pytest.raises(AssertionError):                          # two lengths in one call
        model._video_tables(_videos(torch.float32, T=32) + _videos(torch.float32, T=64), False)


# ---------------------------------------------------------------------------------------------- _per_query_levels
def test_per_query_levels_are_views_of_the_flat_buffers():
    pkg, model = _model(n_levels=3)
    T, nq, S = 16, 2, 28
    flat = (torch.randn(nq, S), torch.randn(nq, S, 2), torch.rand(nq, S) > 0.5)
    lg, of, mk = model._per_query_levels(flat, T, 0, nq)
    assert len(lg) == len(of) == len(mk) == nq
    for q in range(nq):
        assert [tuple(x.shape) for x in lg[q]] == [tuple(x.shape) for x in mk[q]] == [(1, 16), (1, 8), (1, 4)]
        assert [tuple(x.shape) for x in of[q]] == [(1, 16, 2), (1, 8, 2), (1, 4, 2)]
        for part, buf in ((lg, flat[0]), (of, flat[1]), (mk, flat[2])):
            assert isinstance(part[q], tuple)
            assert all(x.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr() for x in part[q])
            assert torch.equal(torch.cat(part[q], 1)[0], buf[q])
    one = model._per_query_levels(flat, T, 1, 2)
    assert len(one[0]) == 1 and one[0][0][0].data_ptr() == lg[1][0].data_ptr()
    flat[0][1, 0] = 7.0                                           # a view: a write to the buffer shows
    assert float(lg[1][0][0, 0]) == 7.0
    pkg, strided = _model(n_levels=3, vid_stride=2)               # the pyramid starts behind the strided convolutions
    assert [tuple(x.shape) for x in strided._per_query_levels((torch.zeros(1, 14),) * 3, T, 0, 1)[0][0]] == [(1, 8), (1, 4), (1, 2)]


# ---------------------------------------------------------------------------------------------- _alloc_outputs
def test_alloc_outputs_reuse():
    pkg, model = _model()
    dev = torch.device('cpu')
    assert model._out_cache == {}
    a = model._alloc_outputs(3, 30, dev, False)
    assert model._out_cache == {}                                 # reuse=False never touches the cache
    assert [tuple(x.shape) for x in a] == [(3, 30), (3, 30, 2), (3, 30)]
    assert [x.dtype for x in a] == [torch.float32, torch.float32, torch.bool]
    b = model._alloc_outputs(3, 30, dev, True)
    c = model._alloc_outputs(3, 30, dev, True)
    assert all(x is y for x, y in zip(b, c)) and not any(x is y for x, y in zip(a, b))
    d = model._alloc_outputs(3, 30, dev, False)                   # ... not even when an entry of this shape is there
    assert not any(x is y for x, y in zip(d, b)) and all(x is y for x, y in zip(model._alloc_outputs(3, 30, dev, True), b))
    e = model._alloc_outputs(2, 30, dev, True)                    # another shape replaces the one entry
    assert len(model._out_cache) == 1 and all(x is y for x, y in zip(model._out_cache[(2, 30, dev)], e))
    assert not any(x is y for x, y in zip(model._alloc_outputs(3, 30, dev, True), b))


# ---------------------------------------------------------------------------------------------- the refusals come first
def _video(T=128, nq=1, dtype=torch.float32):
    return (torch.zeros(1, 64, T, dtype=dtype), torch.zeros(1, 64, T, dtype=dtype), torch.ones(1, T, dtype=torch.bool),
            tuple(torch.zeros(1, 32, 5) for _ in range(nq)), torch.zeros(nq, 64), tuple(torch.ones(1, 1, 5, dtype=torch.bool) for _ in range(nq)))


def _batch(pkg, counts, nqs, T=128):
    nv = len(counts)
    return pkg.modeling.SelectionBatch(torch.zeros(sum(nqs), T), torch.zeros(nv, T, dtype=torch.int32), torch.zeros(nv, T, dtype=torch.int32),
                                       None, counts, nqs)


def test_refusals_come_before_the_device_check():
    pkg, model = _model()
    a, h = _video(), _video(dtype=torch.float16)
    mixed = (h[0], a[1]) + a[2:]
    gpu = 'runs on the MI355X only'
    # forward (eval and train) and forward_window: the float16 pair
    with pytest.raises(ValueError, match='come as a pair'):
        model(*mixed, eval=True)
    with pytest.raises(ValueError, match='come as a pair'):
        model.forward_window(mixed[0], mixed[1], a[2], a[3], a[5], torch.zeros(1, 128))
    # forward_videos: the pair, then all float16 or none
    with pytest.raises(ValueError, match='come as a pair'):
        model.forward_videos([a, mixed])
    with pytest.raises(ValueError, match='forward_videos: the videos of one call are all float16 or none of them is'):
        model.forward_videos([a, h])
    # select_clips_videos / gather_clip_rows_videos: all float16 or none
    with pytest.raises(ValueError, match='select_clips_videos: the videos of one call are all float16 or none of them is'):
        model.select_clips_videos([a, h])
    batch = _batch(pkg, [4, 3], [1, 1])
    with pytest.raises(ValueError, match='gather_clip_rows_videos: 1 feature tensors for a selection of 2 videos'):
        model.gather_clip_rows_videos([a[0]], batch)
    with pytest.raises(ValueError, match='gather_clip_rows_videos: the videos of one call are all float16 or none of them is'):
        model.gather_clip_rows_videos([a[0], h[0]], batch)
    # forward_videos_selected: the pair of (vid_rows, shallow_vid)
    with pytest.raises(ValueError, match='come as a pair'):
        model.forward_videos_selected(torch.zeros(7, 64, dtype=torch.float16), batch, [a, a])
    # forward_selected: the model's refusals and the pair (what follows its device check stays behind it, as before)
    with pytest.raises(ValueError, match='come as a pair'):
        model.forward_selected(torch.zeros(4, 64, dtype=torch.float16), batch.selection(0), a[1], a[2], a[3], a[5])
    with pytest.raises(NotImplementedError, match='scat'):
        _model(scat=True)[1].forward_selected(torch.zeros(4, 64), batch.selection(0), a[1], a[2], a[3], a[5])
    # with every host check passed, each route ends at the device check -- no engine, no allocation
    calls = [lambda: model(*a, eval=True), lambda: model(*a), lambda:model.forward_window(a[0], a[1], a[2], a[3], a[5], torch.zeros(1, 128)),
             lambda: model.forward_videos([a, a]), lambda: model.select_clips_videos([a, a]),
             lambda: model.gather_clip_rows_videos([a[0], a[0]], batch), lambda: model.forward_videos_selected(torch.zeros(7, 64), batch, [a, a]),
             lambda: model.forward_selected(torch.zeros(4, 64), batch.selection(0), a[1], a[2], a[3], a[5]),
             lambda: model.select_clips(a[1], a[2], a[4])]
    for call in calls:
        with pytest.raises(RuntimeError, match=gpu):
            call()
    assert model._engine is None and model._out_cache == {}
