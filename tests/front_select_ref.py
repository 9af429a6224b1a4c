"""An fp64 restatement in torch of include/decafnet_hip_front_select.h: the forward and the weight gradient of vid_map on the packed
expert rows of the selected clips (``selected_forward`` / ``selected_grads``), and the packing itself (``pack``: the union of a video's
gate rows AND its mask, as tests/select_videos_ref.py restates dcf_op_select_clips_videos).  A helper module of
tests/test_front_select_cpu.py, tests/test_gpu_front_select.py and tests/front_select_abi_cases.py.

    rows[row_first[v] + i]  = vid[v][:, clips[v, i]]
    Y[q,t,:]                = bias + m ( g P1c[row_first[v] + pos[v,t]] + P2[v,t] + c w3 ),   P1c = rows W1^T; no expert half where pos < 0
    R1c[row_first[v] + pos] = sum_{q in v} m g dY[q,t,:]   (pos >= 0),   dW1 = R1c^T rows
"""
import torch

import front_grad_ref as R
import select_videos_ref as V


def pack(vid, gate, vid_masks, text_size):
    """vid (nvid, D, T) or None, gate (B', T), vid_masks (nvid, T) -> (rows (n_rows, D) or None, row_first: list, pos int32 (nvid, T),
    clips int32 (nvid, T), counts: list)"""
    clips, pos, counts, row_first = V.select_clips_videos(gate, vid_masks, list(text_size), fill=0)
    rows = None if vid is None else V.gather_clip_rows_videos(list(vid), clips, counts)
    return rows, row_first, pos, clips, counts


def _row_index(row_first, pos, text_size):
    """per query row: (B', T) long index into the packed rows (clamped to 0 where there is none) and the (B', T) bool "has a row\""""
    v = R._video_of(text_size)
    first = torch.tensor(row_first[:-1])[v][:, None]
    p = pos.long()[v]
    return (first + p).clamp(min=0), p >= 0


def selected_forward(rows, row_first, pos, shallow, gate, mask, correl, text_size, W, bias):
    D, n = rows.size(1), row_first[-1]
    v = R._video_of(text_size)
    idx, has = _row_index(row_first, pos, text_size)
    P1c = rows[:n] @ W[:, :D].t()
    m = mask.to(rows.dtype)[..., None]
    acc = (gate * (has & (gate != 0)).to(rows.dtype))[..., None] * P1c[idx]
    if shallow is not None:
        acc = acc + (R.tm(shallow) @ W[:, D:2 * D].t())[v]
    if correl is not None:
        acc = acc + correl[..., None] * W[:, -1]
    return bias + m * acc


def selected_grads(rows, row_first, pos, shallow, gate, mask, correl, text_size, dY):
    """dW (E, Cin), db (E,)"""
    n, nvid = row_first[-1], pos.size(0)
    v = R._video_of(text_size)
    idx, has = _row_index(row_first, pos, text_size)
    m = mask.to(dY.dtype)[..., None]
    r1 = m * gate[..., None] * dY
    R1c = torch.zeros(n, dY.size(-1), dtype=dY.dtype).index_add_(0, idx[has], r1[has])
    cols = [R1c.t() @ rows[:n]]
    if shallow is not None:
        R2 = torch.zeros(nvid, *dY.shape[1:], dtype=dY.dtype).index_add_(0, v, m * dY)
        cols.append(torch.einsum('bte,bdt->ed', R2, shallow))
    if correl is not None:
        cols.append((m * correl[..., None] * dY).sum((0, 1))[:, None])
    return torch.cat(cols, dim=1), dY.sum((0, 1))


def fixture_pack(f, dtype=torch.float64):
    """the fixture's expert rows at the union of its gate rows AND the video mask -> (rows, row_first, pos, counts)"""
    rows, row_first, pos, _, counts = pack(f.vid.to(dtype), f.gate.float(), f.vid_masks, f.text_size)
    return rows, row_first, pos, counts
