"""Generate tests/golden/step_grad_attn_drop_<case>*.npz: make_golden_step_grad_drop.py's whole training step of the reference -- forward
in .train(), the Trainer's objective, `total.backward()`, in fp32 and from the same model cast to fp64, every random draw replaced by the
project's stated stream -- with EVERY dropout site the reference's model constructors take switched on (include/decafnet_hip_attn_drop.h):

    attn_pdrop 0.1, proj_pdrop 0.2, path_pdrop 0.3 on vid_net, fusion and text_net alike, cdrop 0.1, the TCN at its hard-wired 0.5.

Run where the reference is importable (not on the GPU machine):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_step_grad_attn_drop.py

Cases, otherwise those of make_golden_step_grad.py:
    s2a   `s2` WITH its second fusion: stride 2, msf, T = 80; the fusion's modules are called again per pyramid level, so the call is
          part of the site: call k >= 1 of decoder layer i draws at (DROP_G_FUSION2, (k - 1) * n_layers + i)
    s1g   `s1` with mha_win_size = 0 and one head (heads of 32 channels: what the global kernels take): global attention over the clips
          in the stem and in every pyramid level
The generator is make_golden_step_grad_drop.main() itself, with its conditions on the reference alone, run on these cases (as
make_golden_global_attn_grad.step_case runs make_golden_step_grad.main): its `Stream` is subclassed here for the sites it does not
know -- the 4-D attention maps (sub 6, element index = flat index), the text encoder's blocks (group 5), the second fusion's calls
(group 6) and channel dropout (group 7, sub 7, one decision per (sample, channel), applied where the reference applies it: on the input
of vid_map) -- and its files are renamed step_grad_attn_drop_<case>*.npz (tests/step_grad_ref.py reads them as `attn_drop_<case>`).

Conditions on the reference alone beyond make_golden_step_grad_drop.py's (no drop-path site drops every row, one drops a row, one keeps
all; e_ref <= 2^-15 max|g_64|; every parameter takes a gradient), asserted here and again on the committed files by
tests/test_attn_drop_cpu.py: every dropout site both drops and keeps, and at least one channel is dropped for one sample and kept for
another.  If a key trips a condition, change the key, not the condition."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402
import make_golden_dropout as MD  # noqa: E402
import make_golden_step_grad as SG  # noqa: E402
import make_golden_step_grad_drop as SD  # noqa: E402
import philox_ref as P  # noqa: E402

ATTN, CDROP = 0.1, 0.1
G_TEXT, G_FUSION2, G_INPUT, SUB_ATTN, SUB_CHANNEL = 5, 6, 7, 6, 7
CASES = {
    's2a': dict(SG.CASES['s2'], key0=0xD1B54A32D192ED03),
    's1g': dict(SG.CASES['s1'], opt=dict(SG.CASES['s1']['opt'], win=0, n_heads=1), key0=0x9E3779B97F4A7C15),
}
SECOND = {'s2a': True, 's1g': False}
N_FUSION = 2                                  # decoder layers of the fusion (config.make_opt's default; asserted on the model)
CURRENT = {}                                  # the stream of the run in progress (the vid_map wrapper of the model reads it)
base_site_of, BaseStream = MD.site_of, MD.Stream


def site_of(name):
    parts = name.split('.')
    if parts[0] == 'text_net' and parts[1] == 'transformer':
        return G_TEXT, int(parts[2]), '.'.join(parts[3:])
    return base_site_of(name)


class Stream(BaseStream):
    """MD.Stream with the attention maps, the second fusion's calls and channel dropout"""

    def __init__(self, seed):
        super().__init__(seed)
        self.calls = {}
        CURRENT['stream'] = self

    def _forward_index(self, mod, per_forward):
        """how many forwards of its block this module has finished before this call"""
        k = self.calls.get(id(mod), 0)
        self.calls[id(mod)] = k + 1
        return k // per_forward

    def _placed(self, mod, per_forward, fn):
        """fn() with the module's site moved to the second fusion where this is a later call of a fusion module"""
        g, i, rest = mod._dcf_site
        k = self._forward_index(mod, per_forward) if g == P.G_FUSION else 0
        if k == 0:
            return fn()
        mod._dcf_site = (G_FUSION2, (k - 1) * N_FUSION + i, rest)
        try:
            return fn()
        finally:
            mod._dcf_site = (g, i, rest)

    def dropout(self, mod, x):
        if not mod.training or mod.p == 0.0:
            return x
        rest = mod._dcf_site[2]
        if rest in ('attn.attn.attn_drop', 'xattn.xattn.attn_drop'):
            return self._placed(mod, 1, lambda: self.attn(mod, x))
        return self._placed(mod, 2 if rest == 'ffn.dropout' else 1, lambda: self._plain(mod, x))

    def _plain(self, mod, x):
        g, i, rest = mod._dcf_site
        if g in (G_TEXT, G_FUSION2):            # MD.Stream names its sites by the groups it knows: the same subs under this group
            base = dict(zip((G_TEXT, G_FUSION2), (P.G_STEM, P.G_FUSION)))[g]
            sub = P.PROJ if rest.endswith('proj_drop') else None
            if rest == 'ffn.dropout':
                k = self.ffn_calls.get((g, i), 0)
                self.ffn_calls[(g, i)] = k + 1
                sub = P.FFN_HID if k % 2 == 0 else P.FFN_OUT
            assert sub is not None and base is not None, mod._dcf_site
            s = P.site(g, i, sub)
            assert x.ndim == 3 and x.is_contiguous() and s not in self.log, (s, x.shape)
            keep = P.dropout_mask(self.seed, s, tuple(x.shape), mod.p)
            self.log[s] = (tuple(x.shape), keep)
            return x * (torch.from_numpy(keep).to(x.dtype) * float(P.scale(mod.p)))
        return super().dropout(mod, x)

    def attn(self, mod, x):
        g, i, _ = mod._dcf_site
        s = P.site(g, i, SUB_ATTN)
        assert x.ndim == 4 and x.is_contiguous() and s not in self.log, (s, x.shape)
        keep = P.keep(self.seed, s, np.arange(x.numel(), dtype=np.uint64).reshape(tuple(x.shape)), mod.p)
        self.log[s] = (tuple(x.shape), keep)
        return x * (torch.from_numpy(keep).to(x.dtype) * float(P.scale(mod.p)))

    def drop_path(self, mod, x):
        return self._placed(mod, 1, lambda: BaseStream.drop_path(self, mod, x))

    def channel(self, x):
        """nn.Dropout1d(CDROP) on the (B', Cin, T) input of vid_map (model.py:614): one decision per (b, c), e = b Cin + c"""
        s = P.site(G_INPUT, 0, SUB_CHANNEL)
        assert x.ndim == 3 and s not in self.log
        keep = P.keep(self.seed, s, np.arange(x.size(0) * x.size(1), dtype=np.uint64).reshape(x.size(0), x.size(1)), CDROP)
        self.log[s] = (tuple(x.shape[:2]), keep)
        return x * (torch.from_numpy(keep).to(x.dtype) * float(P.scale(CDROP)))[:, :, None]


def patched_make_opt(**kw):
    opt = base_make_opt(**kw)
    for part in ('vid_net', 'fusion', 'text_net'):
        opt.model[part]['attn_pdrop'] = ATTN
    opt.model['text_net']['proj_pdrop'], opt.model['text_net']['path_pdrop'] = SD.PROJ, SD.PATH
    return opt


class Bypass(torch.nn.Module):
    """calls a module's forward without its hooks"""

    def __init__(self, module):
        super().__init__()
        object.__setattr__(self, 'inner', module)

    def forward(self, *args, **kw):
        return self.inner.forward(*args, **kw)


def model_factory(real):
    def build(opt, second_fusion=False):
        """the case's own second_fusion (make_golden_step_grad_drop.py builds every case without); channel dropout moves from the
        nn.Dropout1d in front of vid_map into vid_map's forward, so that the generator's hook on vid_map still reads the gate off an
        input without dropped channels -- the arithmetic is the reference's: vid_map(channel_drop(x), mask)"""
        net = real(opt, second_fusion=SECOND[CURRENT['case']])
        assert len(net.fusion.layers) == N_FUSION and net.channel_drop.p == 0.0
        if net.second_fusion:                  # the generator's hook on `fusion` taps the first fusion: the calls per level go past it
            outer = net.fuse_and_predict

            def fuse_and_predict(*args, **kw):
                real_fusion = net._modules['fusion']
                net._modules['fusion'] = Bypass(real_fusion)
                try:
                    return outer(*args, **kw)
                finally:
                    net._modules['fusion'] = real_fusion
            net.fuse_and_predict = fuse_and_predict
        inner = net.vid_map.forward
        net.vid_map.forward = lambda x, m: inner(CURRENT['stream'].channel(x) if net.training else x, m)
        return net
    return build


def save(name, d):
    """step_grad_drop_<case>*.npz -> step_grad_attn_drop_<case>*.npz; the core file's meta says what this generator switched on, and the
    conditions of this generator are asserted on it"""
    if 'meta' in d:
        m = d['meta']
        case = m['case']
        m.update(second_fusion=SECOND[case], attn_pdrop=ATTN, cdrop=CDROP, text_dropout=True)
        by_sub = {}
        for s in m['sites']:
            n = int(np.prod(s['shape']))
            if s['site'] & 15 not in (P.PATH_ATTN, P.PATH_FFN):
                assert 0 < s['kept'] < n, ('a dropout site that does not both drop and keep', s)
            by_sub.setdefault((s['site'] >> 16, s['site'] & 15), []).append(s['site'])
        groups = {g for g, _ in by_sub}
        assert {G_TEXT, G_INPUT, P.G_FUSION, P.G_STEM, P.G_BRANCH, P.G_REFINE} <= groups and (G_FUSION2 in groups) == SECOND[case], groups
        if SECOND[case]:
            assert len(by_sub[(G_FUSION2, SUB_ATTN)]) == m['n_levels'] * N_FUSION
        ch = [s for s in m['sites'] if s['site'] == P.site(G_INPUT, 0, SUB_CHANNEL)][0]
        keep = P.keep(m['seed'], ch['site'], np.arange(int(np.prod(ch['shape'])), dtype=np.uint64).reshape(ch['shape']), CDROP)
        assert (keep.any(0) & ~keep.all(0)).any(), 'no channel is dropped for one sample and kept for another'
        print(f'{case}: {len(m["sites"])} sites in groups {sorted(groups)}, channel keep {int(keep.sum())} of {keep.size}')
    base_save(name.replace('step_grad_drop_', 'step_grad_attn_drop_'), d)


def main():
    global base_make_opt, base_save
    MG.install_stubs()
    import libs.modeling.model as RM
    base_make_opt, base_save = MG.make_opt, SG.save
    MG.make_opt, SG.save, MD.site_of, MD.Stream = patched_make_opt, save, site_of, Stream
    RM.PtTransformerEarlyFusionIterative = model_factory(RM.PtTransformerEarlyFusionIterative)
    for name, c in CASES.items():              # one case per run of the generator's main: the model factory reads which
        CURRENT['case'] = name
        SD.CASES = {name: c}
        SD.main()


if __name__ == '__main__':
    main()
