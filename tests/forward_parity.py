"""The forward's parity rule and its fp64 side (a helper module, shared by tests/test_forward_parity_cpu.py and tests/test_gpu_e2e.py).

The rule is the one of the gradient tests (tests/test_gpu_conv_grad.py), per fixture and output kind:

    e_gpu <= max(4 * e_ref, 2^-21 * max |y64|),   e = max |y - y64|

y64 is the CPU oracle (oracle/decafnet_ref.py) evaluated in fp64: the state dict and every float input cast to torch.float64, masks
unchanged (`oracle64`).  e_ref is the error of the fp32 reference side against it: the reference's own fixture wherever one exists,
the fp32 oracle elsewhere -- never anything the GPU returned.  The maxima are POOLED over all queries and all pyramid levels of one
output kind (`pool`): a top pyramid level has a handful of clips, and its own e_ref can be tiny by luck.

The fp64 results of the fixtures are computed once per process (`e2e_case`, `train_case`, `train_secondary_case`,
`text_identity_cases`, `text_identity_model_case`) and must be left unchanged by their users.
"""
import functools
import sys
import types

import torch

from conftest import Golden, ROOT, load_pkg

if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import decafnet_ref as R  # noqa: E402

FLOOR = 2.0 ** -21
E2E = ['c1', 'pe', 'nomsf', 'scat', 'sfonly', 'affine', 'stride2', 'stride4', 'pool', 'pool_stride2']
SECONDARY = ['late', 'second', 'late_scat', 'early', 'early_single']
TRAIN_SECONDARY = ['late', 'early', 'early_single']


def to64(x):
    """float tensors -> fp64, through lists / tuples / dicts; masks, integers and python values unchanged"""
    if isinstance(x, torch.Tensor):
        return x.double() if x.is_floating_point() else x
    if isinstance(x, dict) and x and all(isinstance(v, torch.Tensor) for v in x.values()):
        return {k: to64(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(to64(v) for v in x)
    return x


def assert_fp64(x, where):
    """every float tensor of an oracle result is fp64: a silent downcast inside the oracle would make the gate fp32 against fp32"""
    if isinstance(x, torch.Tensor):
        assert x.dtype == torch.float64 or not x.is_floating_point(), (where, x.dtype)
    elif isinstance(x, dict):
        for k, v in x.items():
            assert_fp64(v, f'{where}[{k!r}]')
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            assert_fp64(v, f'{where}[{i}]')


def _in_fp64(fn):
    @functools.wraps(fn)
    def run(sd, cfg, *args, **kw):
        with torch.no_grad():
            out = fn(to64(sd), cfg, *(to64(a) for a in args), **{k: to64(v) for k, v in kw.items()})
        assert_fp64(out, fn.__name__)
        return out
    return run


# the oracle's entry points with the state dict and every float input cast to fp64; called exactly as the fp32 forms are
oracle64 = types.SimpleNamespace(**{name: _in_fp64(getattr(R, name)) for name in (
    'encode_text', 'forward_eval', 'forward_eval_late_fusion', 'forward_eval_early_fusion', 'forward_train', 'forward_train_single_head')})


def pool(parts, select=None):
    """one flat fp64 vector of the tensors in `parts` (nested lists: queries x levels); select[i] picks elements of the i-th leaf"""
    flat = []

    def walk(p):
        if isinstance(p, torch.Tensor):
            flat.append(p.detach().cpu())
        else:
            for x in p:
                walk(x)
    walk(parts)
    if select is not None:
        assert len(select) == len(flat)
        flat = [t[s] for t, s in zip(flat, select)]
    return torch.cat([t.double().reshape(-1) for t in flat])


def rule(got, y64, y32):
    """the rule's figures for one pooled output kind, nothing asserted: (max |y64|, e_ref, e_gpu, bound, e_gpu / bound)"""
    got, y64, y32 = got.detach().cpu().double(), y64.detach().double(), y32.detach().double()
    e_ref, e_gpu, top = float((y32 - y64).abs().max()), float((got - y64).abs().max()), float(y64.abs().max())
    bound = max(4 * e_ref, FLOOR * top)
    return top, e_ref, e_gpu, bound, (e_gpu / bound if bound else 0.0)


def check(tag, got, y64, y32):
    """the rule on one pooled output kind; prints the FWERR line, asserts, returns e_gpu / bound"""
    assert got.shape == y64.shape == y32.shape, (tag, got.shape, y64.shape, y32.shape)
    assert bool(torch.isfinite(got).all()), tag
    top, e_ref, e_gpu, bound, ratio = rule(got, y64, y32)
    print(f'FWERR {tag}: max|y64| {top:.3e} e_ref {e_ref:.3e} e_gpu {e_gpu:.3e} bound {bound:.3e} ratio {ratio:.3f}')
    assert e_gpu <= bound, (tag, e_gpu, bound)
    return ratio


class Case(types.SimpleNamespace):
    """g (the fixture), meta, kw, opt, sd, inp, y64 / y32: dicts of output kind -> nested lists of tensors (queries x levels; text,
    vid_map, fused: queries), masks: the fixture's"""


def _eval_oracle(ns, cls, sd, cfg, inp, texts, tmasks):
    args = (sd, cfg, inp['vid'], inp['shallow_vid'], inp['vid_masks'], list(texts), inp['text_cls'], list(tmasks))
    if cls == 'PtTransformer':
        return ns.forward_eval_late_fusion(*args), None
    if cls is not None and cls.startswith('early'):
        return ns.forward_eval_early_fusion(*args, second_fusion=cls == 'early2'), None
    out = ns.forward_eval(*args, return_intermediates=True, second_fusion=cls == 'iter2')
    return out[:3], out[3]


def _eval_case(g, kw, meta, shapes, prefix=''):
    """fp64 oracle of an evaluation fixture (keys `<prefix>q<i>/...`), with its own fp64 text encodings; y32 = the fixture"""
    pkg = load_pkg()
    opt = pkg.config.make_opt(**kw)
    sd = pkg.synth.make_state_dict(shapes, meta['wseed'])
    inp = pkg.synth.make_inputs(meta.get('feat_dim', kw['D']), meta['T'], meta['vid_len'], meta['nq'], kw['text_in'], meta['lq'], meta['iseed'])
    nq, L = meta['nq'], kw['n_levels']
    texts, tmasks = zip(*[oracle64.encode_text(sd, opt.model, t[None], torch.ones(1, 1, t.size(-1), dtype=torch.bool)) for t in inp['tokens']])
    (lg, of, mk), inter = _eval_oracle(oracle64, meta.get('cls'), sd, opt.model, inp, texts, tmasks)
    y64 = dict(text=list(texts), logits=lg, offsets=of)
    y32 = dict(logits=[[g.t(f'{prefix}q{q}/l{l}/logits') for l in range(L)] for q in range(nq)],
               offsets=[[g.t(f'{prefix}q{q}/l{l}/offsets') for l in range(L)] for q in range(nq)])
    if f'{prefix}q0/text' in g:
        y32['text'] = [g.t(f'{prefix}q{q}/text') for q in range(nq)]
    masks = [[g.t(f'{prefix}q{q}/l{l}/mask') for l in range(L)] for q in range(nq)]
    for q in range(nq):                                        # same masks and same shapes as the fixture's
        if f'{prefix}q{q}/text_mask' in g:
            assert torch.equal(tmasks[q], g.t(f'{prefix}q{q}/text_mask'))
        for l in range(L):
            assert torch.equal(mk[q][l], masks[q][l]), (q, l)
            assert lg[q][l].shape == y32['logits'][q][l].shape and of[q][l].shape == y32['offsets'][q][l].shape
    if inter is not None and f'{prefix}q0/vid_map' in g:
        for key in ('vid_map', 'fused'):
            y64[key] = [inter['per_query'][q][key] for q in range(nq)]
            y32[key] = [g.t(f'{prefix}q{q}/{key}') for q in range(nq)]
    return Case(g=g, meta=meta, kw=kw, opt=opt, sd=sd, inp=inp, nq=nq, L=L, y64=y64, y32=y32, masks=masks, tmasks=list(tmasks))


@functools.lru_cache(maxsize=None)
def e2e_case(name):
    """tests/golden/e2e_<name>.npz (the ten compositions of the default class and the five secondary ones)"""
    g = Golden(f'e2e_{name}.npz')
    return _eval_case(g, g.js('opt_kwargs'), g.js('meta'), g.js('shapes'))


@functools.lru_cache(maxsize=None)
def text_identity_model_case():
    """the model of tests/golden/text_identity.npz (text_net.name == 'identity')"""
    g = Golden('text_identity.npz')
    return _eval_case(g, g.js('model/opt_kwargs'), g.js('model/meta'), g.js('model/shapes'), prefix='model/')


@functools.lru_cache(maxsize=None)
def text_identity_cases():
    """the stand-alone TextIdentity cases of tests/golden/text_identity.npz: [(case, y64, fixture output)]"""
    g, pkg = Golden('text_identity.npz'), load_pkg()
    out = []
    for i, c in enumerate(g.js('cases')):
        shapes = g.js(f't{i}/shapes')
        sd = {'text_net.' + k: v for k, v in pkg.synth.make_state_dict(shapes, 700 + i).items()} if shapes else {}
        cfg = dict(name='identity', max_seq_len=c['max_seq_len'], n_heads=c['n_heads'], use_abs_pe=c['use_abs_pe'], use_bkgd_token=c['use_bkgd_token'])
        y, m = oracle64.encode_text(sd, {'text_net': cfg}, g.t(f't{i}/tokens'), g.t(f't{i}/mask'))
        assert torch.equal(m, g.t(f't{i}/out_mask')) and y.shape == g.t(f't{i}/out').shape
        out.append((c, y, g.t(f't{i}/out')))
    return out


def _train(g, kw, shapes, wseed, sizes, prefix, kind):
    pkg = load_pkg()
    opt = pkg.config.make_opt(**kw)
    sd = pkg.synth.make_state_dict(shapes, wseed)
    args = (g.t(f'{prefix}vid'), g.t(f'{prefix}shallow'), g.t(f'{prefix}vid_masks'), g.t(f'{prefix}tokens'), g.t(f'{prefix}token_masks'),
            g.t(f'{prefix}text_cls'), sizes)
    if kind is None:
        names, out = ('logits1', 'logits2', 'offsets', 'masks'), oracle64.forward_train(sd, opt.model, *args)
    else:
        names, out = ('logits', 'offsets', 'masks'), oracle64.forward_train_single_head(sd, opt.model, kind, *args)
    L = kw['n_levels']
    y64, y32 = {}, {}
    for part, name in zip(out, names):
        want = [g.t(f'{prefix}{name}/l{l}') for l in range(L)]
        assert all(part[l].shape == want[l].shape for l in range(L)), name
        if name == 'masks':
            assert all(torch.equal(part[l], want[l]) for l in range(L))
            masks = want
        else:
            y64[name], y32[name] = list(part), want
    return Case(g=g, kw=kw, opt=opt, sd=sd, L=L, y64=y64, y32=y32, masks=masks)


@functools.lru_cache(maxsize=None)
def train_case():
    """tests/golden/train.npz: the training-mode forward of the default class (logits1, logits2, offsets)"""
    g = Golden('train.npz')
    meta = g.js('meta')
    return _train(g, g.js('opt_kwargs'), g.js('shapes'), meta['wseed'], meta['sizes'], '', None)


@functools.lru_cache(maxsize=None)
def train_secondary_case(name):
    """tests/golden/train_secondary.npz: the training-mode forward of the classes with one classification head"""
    g = Golden('train_secondary.npz')
    case, meta = g.js('cases')[name], g.js('meta')
    kind = 'late' if case['cls'] == 'PtTransformer' else case['cls']
    return _train(g, case['opt_kwargs'], g.js(f'{name}/shapes'), case['wseed'], meta['sizes'], f'{name}/', kind)


def valid_columns(case):
    """per query, the valid clips of a (1, E, T) tap: padded clips of vid_map carry its bias, consumers re-mask"""
    return [(slice(None), slice(None), case.inp['vid_masks'][0])] * case.nq
