"""fp64 restatement of the level-0 embedding stage of the video backbone (video_net.py:133-151) in the two forms the engine runs:

``stage_unfolded``  as the reference writes it (oracle/decafnet_ref.py:279-294): fusion.ln_out -> embd_fc -> [MaskedConv1D(k3) ->
                    LayerNorm -> ReLU] x 2 -> + pe * mask; MaskedConv1D is conv(x * mask) and does not mask its output.
``stage_folded``    as k_embd_chain computes it (csrc/embd_chain.h): LayerNorm WITHOUT affine -> the first convolution with embd_fc and
                    ln_out's affine folded into its weight, and three bias vectors c_t each gated by its tap's neighbour flag ->
                    LayerNorm -> ReLU -> masked k3 convolution -> LayerNorm -> ReLU -> + pe * mask.

Rows are laid out as the kernels see them: X (B, T, C), mask (B, T) bool.  Everything is float64; no GPU."""
import torch

EPS = 1e-5


def params_of(sd, E):
    """the stage's parameters from a state dict, float64: Wfc (E, E), bfc, g / b of fusion.ln_out, Wc[i] (E, E, 3), lw[i], lb[i]"""
    d = lambda k: sd[k].detach().cpu().double()
    return dict(Wfc=d('vid_net.embd_fc.conv.weight').reshape(E, E), bfc=d('vid_net.embd_fc.conv.bias').reshape(E),
                g=d('fusion.ln_out.weight').reshape(E), b=d('fusion.ln_out.bias').reshape(E),
                Wc=[d(f'vid_net.embd_convs.{i}.conv.weight').reshape(E, E, 3) for i in range(2)],
                lw=[d(f'vid_net.embd_norms.{i}.weight').reshape(E) for i in range(2)],
                lb=[d(f'vid_net.embd_norms.{i}.bias').reshape(E) for i in range(2)])


def ln(x, w=None, b=None):
    """LayerNorm over the channels (last axis): mean, then the mean of squared deviations (blocks.py:125-131)"""
    mu = x.mean(-1, keepdim=True)
    d = x - mu
    y = d / torch.sqrt((d * d).mean(-1, keepdim=True) + EPS)
    return y if w is None else y * w + b


def shifted(x, tap):
    """x[b, t + tap - 1] with zeros beyond the ends of a sequence; x (B, T, ...)"""
    out = torch.zeros_like(x)
    if tap == 0:
        out[:, 1:] = x[:, :-1]
    elif tap == 1:
        out = x.clone()
    else:
        out[:, :-1] = x[:, 1:]
    return out


def masked_conv3(x, mask, W):
    """MaskedConv1D(k3, padding 1, no bias) on rows: W (N, Cin, 3); the output is not masked (blocks.py:98-99)"""
    xm = x * mask.unsqueeze(-1).to(x.dtype)
    return sum(shifted(xm, tap) @ W[:, :, tap].T for tap in range(3))


def fold(p, ln_in):
    """W' (3, N, K) = Wc_t Wfc diag(g), c (3, N) = Wc_t (Wfc b + b_fc); without ln_in the rows come with ln_out's affine applied:
    g = 1, b = 0"""
    E = p['Wfc'].size(0)
    g = p['g'] if ln_in else torch.ones(E, dtype=torch.float64)
    b = p['b'] if ln_in else torch.zeros(E, dtype=torch.float64)
    Wp = torch.stack([p['Wc'][0][:, :, t] @ p['Wfc'] * g for t in range(3)])
    c = torch.stack([p['Wc'][0][:, :, t] @ (p['Wfc'] @ b + p['bfc']) for t in range(3)])
    return Wp, c


def tail(y1, mask, p, pe):
    x = torch.relu(ln(y1, p['lw'][0], p['lb'][0]))
    x = torch.relu(ln(masked_conv3(x, mask, p['Wc'][1]), p['lw'][1], p['lb'][1]))
    if pe is not None:
        x = x + pe[:x.size(1)].double().unsqueeze(0) * mask.unsqueeze(-1).to(x.dtype)
    return x


def stage_unfolded(X, mask, p, ln_in, pe=None):
    X = X.double()
    m = mask.unsqueeze(-1).to(X.dtype)
    xn = ln(X, p['g'], p['b']) if ln_in else X
    x = (xn * m) @ p['Wfc'].T + p['bfc']                     # embd_fc = MaskedConv1D(k1): conv(x * mask) + bias
    return tail(masked_conv3(x, mask, p['Wc'][0]), mask, p, pe)


def stage_folded(X, mask, p, ln_in, pe=None):
    X = X.double()
    m = mask.unsqueeze(-1).to(X.dtype)
    xh = ln(X) if ln_in else X
    Wp, c = fold(p, ln_in)
    y = 0
    for t in range(3):                                       # the tap's row must exist in the sequence AND be valid
        y = y + shifted(m, t) * (shifted(xh, t) @ Wp[t].T + c[t])
    return tail(y, mask, p, pe)
