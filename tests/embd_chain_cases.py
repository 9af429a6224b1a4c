"""Shared pieces of the GPU tests of the embedding-stage extension (include/decafnet_hip_embd.h): a small finalized model at E = 256,
the operator shapes and their masks, and the two exports as Python calls."""
import ctypes

import torch

from conftest import load_pkg

E = 256
# B sequences x T rows.  Seams at wave boundaries (32), at window boundaries (124, 248) and one row past one; sequences back to back;
# a one-row sequence; the kernel's window holds 128 rows of which 124 come out
SHAPES = [(5, 64), (3, 100), (2, 333), (1, 366), (2, 124), (1, 125), (4, 1)]
KW = dict(D=64, E=E, TE=32, text_in=32, n_levels=2, win=5, n_heads=4, sn=8, sratio=0.3, msf=True, norm=True, max_seq_len=512,
          text_layers=1, text_max_len=24, fusion_layers=1)


def make_model(seed=41, mutate=None, **over):
    """(pkg, model, sd, handle): the model on the GPU with its engine bound and finalized; mutate(sd) edits the weights first"""
    pkg = load_pkg()
    opt = pkg.config.make_opt(**dict(KW, **over))
    model = pkg.modeling.create_model(opt)
    sd = pkg.synth.make_state_dict({k: list(v.shape) for k, v in model.state_dict().items()}, seed)
    if mutate is not None:
        mutate(sd)
    model.load_state_dict(sd)
    model = model.cuda().eval().requires_grad_(False)
    model._engine = pkg.modeling._Engine(model._config())
    model._engine.bind(model)
    return pkg, model, sd, model._engine.handle


def masks_of(B, T, seed):
    """sequence 0 full; with three or more sequences the second one fully masked (between two valid ones); the others with a ragged
    tail and, where they are long enough, holes; a single sequence has both"""
    g = torch.Generator().manual_seed(seed)
    mask = torch.zeros(B, T, dtype=torch.bool)
    for b in range(B):
        if b == 0 and B > 1:
            n = T
        elif b == 1 and B >= 3:
            n = 0
        else:
            n = T if T == 1 else int(torch.randint(max(1, T // 2), T, (1,), generator=g))
        mask[b, :n] = True
        if n > 8 and (b > 0 or B == 1):
            mask[b, torch.randint(1, n - 1, (3,), generator=g)] = False
            mask[b, n // 2:n // 2 + 2] = False               # (a hole of two rows as well)
    return mask


def rows_of(B, T, ln_in, seed, params):
    """input rows (B, T, E) fp32: the raw stream for ln_in, else what fusion.ln_out would have written"""
    import embd_chain_ref as ER
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(B, T, E, generator=g) * 2 + 0.3
    return X if ln_in else ER.ln(X.double(), params['g'], params['b']).float()


def call(pkg, handle, name, X, mask, ln_in, pe, Y):
    B, T = mask.shape
    fn = getattr(pkg._lib.lib(), name)
    rc = fn(handle, pkg._lib.ptr(X), X.stride(-2), pkg._lib.ptr(mask), B, T, int(ln_in), pkg._lib.ptr(pe), pkg._lib.ptr(Y), Y.stride(-2),
            pkg._lib.current_stream())
    pkg._lib.check(rc, name)
    return rc


def set_options(pkg, **opts):
    for k, v in opts.items():
        pkg._lib.check(pkg._lib.lib().dcf_debug_set_option(k.encode(), ctypes.c_int32(v)), 'dcf_debug_set_option')
