"""The reader of tests/golden/front_grad_<case>.npz (make_golden_front_grad.py: vid_map inside one training step of the reference, in
fp32 and fp64) and an fp64 restatement of include/decafnet_hip_front.h in torch: the forward and the weight gradient of vid_map on
SHARED products (``shared_forward`` / ``shared_grads``) beside the dense formula the reference evaluates (``dense_input``,
``dense_forward`` / ``dense_grads``).  A helper module of tests/test_front_grad_cpu.py and tests/test_gpu_front_grad.py.

Fixture tensors keep the reference's channel-major layout for the features ((nvid, D, T)); Y / dY are turned token-major (B', T, E)."""
import torch

from conftest import Golden

CASES = ('msf+scat', 'msf', 'nomsf+scat', 'nomsf')
TILE = 64


def tm(x):
    return x.transpose(1, 2).contiguous()


class Fixture:
    """case `name`.  Inputs: vid / shallow (nvid, D, T), vid_masks (nvid, T), text_cls (B', D), text_size, W (E, Cin), bias (E,), gate /
    mask (B', T) bool, correl (B', T) or None (correl64: the fp64 run's), dY (B', T, E).  Recorded: y32 / dw32 / db32 (the reference in fp32) and the fp64
    yardstick y64 / dw64 / db64 (rebuilt as x_32 + d in fp64).  e_ref[k] = max |x_32 - x_64|, top[k] = max |x_64|."""

    def __init__(self, name):
        g = Golden(f'front_grad_{name}.npz')
        self.name, self.meta = name, g.js('meta')
        self.msf, self.scat, self.text_size = self.meta['msf'], self.meta['scat'], self.meta['text_size']
        self.vid, self.shallow, self.vid_masks, self.text_cls = g.t('vid'), g.t('shallow'), g.t('vid_masks'), g.t('text_cls')
        self.W, self.bias = g.t('W'), g.t('bias')
        self.gate, self.mask = g.t('gate'), g.t('mask_gated')
        self.correl = g.t('correl') if self.scat else None
        self.correl64 = self.correl.double() + g.t('correl_d').double() if self.scat else None      # the fp64 run's scores
        self.dY = tm(g.t('dY'))
        self.y32, self.dw32, self.db32 = tm(g.t('Y_32')), g.t('dW_32'), g.t('db_32')
        self.y64 = self.y32.double() + tm(g.t('Y_d')).double()
        self.dw64, self.db64 = self.dw32.double() + g.t('dW_d').double(), self.db32.double() + g.t('db_d').double()
        ref = {'Y': (self.y32, self.y64), 'dW': (self.dw32, self.dw64), 'db': (self.db32, self.db64)}
        self.e_ref = {k: float((a.double() - b).abs().max()) for k, (a, b) in ref.items()}
        self.top = {k: float(b.abs().max()) for k, (a, b) in ref.items()}
        self.D, self.T, self.E = self.vid.size(1), self.vid.size(2), self.W.size(0)

    def operands(self, dtype=torch.float64, correl64=False):
        """(vid, shallow or None, gate, mask, correl or None, text_size, W, bias) in `dtype` (gate as 0 / 1 of that type).
        correl64: the scores of the reference's fp64 run, the input channel the yardstick saw, in place of the fp32 run's"""
        c = lambda z: None if z is None else z.to(dtype)
        return (c(self.vid), c(self.shallow) if self.msf else None, self.gate.to(dtype), self.mask,
                c(self.correl64 if correl64 else self.correl), self.text_size, c(self.W), c(self.bias))

    def closed_tiles(self):
        """[(video, t0, t1)]: the 64-clip tiles of a video that no query of it keeps"""
        out, q = [], 0
        for b, k in enumerate(self.text_size):
            for t0 in range(0, self.T, TILE):
                if not bool(self.gate[q:q + k, t0:t0 + TILE].any()):
                    out.append((b, t0, min(t0 + TILE, self.T)))
            q += k
        return out


def rule(e_ref, top):
    """the project's bound on the GPU's error against the fp64 yardstick: max(4 e_ref, 2^-21 max |x_64|)"""
    return max(4.0 * e_ref, 2.0 ** -21 * top)


def _video_of(text_size):
    return torch.tensor([b for b, k in enumerate(text_size) for _ in range(k)])


def dense_input(vid, shallow, gate, correl, text_size):
    """the (B', T, Cin) input of vid_map as model.py:578-612 builds it (token-major): [gate * vid ; shallow ; correl]"""
    v = _video_of(text_size)
    parts = [tm(vid)[v] * gate[..., None]]
    if shallow is not None:
        parts.append(tm(shallow)[v])
    if correl is not None:
        parts.append(correl[..., None])
    return torch.cat(parts, dim=2)


def dense_forward(x, mask, W, bias):
    """MaskedConv1D k = 1 (blocks.py:87-106): conv(x * mask) + bias; the output is not masked"""
    return (x * mask[..., None].to(x.dtype)) @ W.t() + bias


def dense_grads(x, mask, dY):
    """dW (E, Cin) and db (E,) of dense_forward: dY is not assumed masked, db runs over every row"""
    xm = (x * mask[..., None].to(x.dtype)).reshape(-1, x.size(-1))
    g = dY.reshape(-1, dY.size(-1))
    return g.t() @ xm, g.sum(0)


def shared_forward(vid, shallow, gate, mask, correl, text_size, W, bias):
    """Y[q,t,:] = bias + m ( g P1[b,t,:] + P2[b,t,:] + c w3 ), P1[b] = vid[b]^T W1^T and P2[b] = shallow[b]^T W2^T once per video"""
    D = vid.size(1)
    v = _video_of(text_size)
    m = mask.to(vid.dtype)[..., None]
    acc = gate[..., None] * (tm(vid) @ W[:, :D].t())[v]
    if shallow is not None:
        acc = acc + (tm(shallow) @ W[:, D:2 * D].t())[v]
    if correl is not None:
        acc = acc + correl[..., None] * W[:, -1]
    return bias + m * acc


def shared_grads(vid, shallow, gate, mask, correl, text_size, dY):
    """dW (E, Cin), db (E,): R1[b] = sum_{q in b} m g dY[q], R2[b] = sum_{q in b} m dY[q]; dW1 = sum_b R1[b]^T vid[b]^T, dW2 likewise
    from R2 and shallow; dw3 = sum m c dY; db = sum dY"""
    nvid = vid.size(0)
    v = _video_of(text_size)
    m = mask.to(dY.dtype)[..., None]
    R1 = torch.zeros(nvid, *dY.shape[1:], dtype=dY.dtype).index_add_(0, v, m * gate[..., None] * dY)
    R2 = torch.zeros(nvid, *dY.shape[1:], dtype=dY.dtype).index_add_(0, v, m * dY)
    cols = [torch.einsum('bte,bdt->ed', R1, vid)]
    if shallow is not None:
        cols.append(torch.einsum('bte,bdt->ed', R2, shallow))
    if correl is not None:
        cols.append((m * correl[..., None] * dY).sum((0, 1))[:, None])
    return torch.cat(cols, dim=1), dY.sum((0, 1))
