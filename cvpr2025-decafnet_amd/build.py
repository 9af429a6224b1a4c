"""Build libdecafnet_hip.so (gfx950) in-tree with hipcc.

    python -m build        # from inside the package directory, or
    __graft_entry__.build()

One translation unit per kernel family, compiled in parallel, linked into a single shared
object that exports the C ABI of include/decafnet_hip.h and of its extensions,
include/decafnet_hip_train.h, include/decafnet_hip_dist.h, include/decafnet_hip_attn.h, include/decafnet_hip_front.h, include/decafnet_hip_guard.h, include/decafnet_hip_clock.h, include/decafnet_hip_half.h, include/decafnet_hip_front_half.h, include/decafnet_hip_embd.h, include/decafnet_hip_batch.h, include/decafnet_hip_eval.h, include/decafnet_hip_fit.h, include/decafnet_hip_steplog.h, include/decafnet_hip_attn_drop.h, include/decafnet_hip_select.h, include/decafnet_hip_select_videos.h and include/decafnet_hip_front_select.h.  The .so stays in the source tree
(git-ignored) so that it travels with the working copy to the GPU machine.
"""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
OUT = os.path.join(HERE, 'libdecafnet_hip.so')
SOURCES = ['engine.hip', 'engine_model.hip', 'engine_blocks.hip', 'engine_hybrid.hip', 'ops_api.hip', 'half.hip', 'dropout.hip', 'gemm.hip', 'gemm_bf16s.hip', 'ffn_chain.hip', 'head_chain.hip', 'dec_chain.hip', 'enc_chain.hip', 'rowops.hip', 'attn.hip', 'attn_grad.hip', 'global_attn_grad.hip', 'score.hip', 'heads.hip', 'postproc.hip', 'loss.hip', 'objective.hip', 'conv_grad.hip', 'enc_grad.hip', 'xattn_grad.hip', 'refine_grad.hip', 'drop_grad.hip', 'front_grad.hip', 'front_select.hip', 'optim.hip', 'optim_guard.hip', 'optim_clock.hip', 'grad_bucket.hip', 'batch.hip', 'eval_metric.hip', 'fit.hip', 'steplog.hip', 'attn_drop.hip', 'calib.hip', 'select_videos.hip', 'select.hip']
ARCH = 'gfx950'
FLAGS = ['-O3', '-std=c++17', '-fPIC', f'--offload-arch={ARCH}', '-fno-gpu-rdc', '-Wall', '-Wno-unused-function']


# No SLP vectorisation: it packs adjacent fp32 operations into v_pk_fma_f32 / v_pk_mul_f32 ... op_sel, which (i) produced
# sporadically wrong low halves in lanes 48 - 63 in the row-statistics epilogue of gemm_bf16s.hip (profiles/r03_notes.md section 1;
# the scalar code is exact and deterministic) and (ii) are slower than the scalar pair on this part (MI355X_MICROARCH.md,
# per-instruction constants: the k3 GEMM kernels got 2 - 5 % faster without them, the other files measured the same).  The
# pattern is kept out of every kernel file rather than only the one where a test caught it.
FLAGS.append('-fno-slp-vectorize')
# eval_metric.hip restates torch's CPU arithmetic operation by operation: no contraction of a multiply and an add into an FMA;
# fit.hip restates numpy's, for the validation loss
EXTRA = {'eval_metric.hip': ['-ffp-contract=off'], 'fit.hip': ['-ffp-contract=off']}


def hipcc():
    for c in (os.environ.get('HIPCC'), '/opt/rocm/bin/hipcc', 'hipcc'):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError('hipcc not found')


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _includes(src, seen=None):
    """the project headers a source file includes, transitively (quoted includes, looked up in csrc/ and include/)"""
    seen = set() if seen is None else seen
    inc_dir = os.path.join(os.path.dirname(HERE), 'include')
    with open(src) as f:
        names = re.findall(r'^\s*#\s*include\s+"([^"]+)"', f.read(), re.M)
    for n in names:
        for d in (CSRC, inc_dir):
            h = os.path.normpath(os.path.join(d, n))
            if os.path.exists(h) and h not in seen:
                seen.add(h)
                _includes(h, seen)
    return seen


def build(force=False, verbose=False, variant=None, extra=None, drop=None):
    """variant=None: the product build (cvpr2025-decafnet_amd/libdecafnet_hip.so).  variant='name': a developer build under
    build/variants/name/ with `extra` = {file: [flags]} added and the flags listed in `drop` = {file: [flags]} removed
    ('*' = every file) -- loaded through DCF_LIB_PATH for A/B runs inside one GPU call (tools/); never the product path."""
    objdir = os.path.join(HERE, 'build') if variant is None else os.path.join(HERE, 'build', 'variants', variant)
    out = OUT if variant is None else os.path.join(objdir, 'libdecafnet_hip.so')
    os.makedirs(objdir, exist_ok=True)
    cc = hipcc()
    jobs = []
    extra, drop = extra or {}, drop or {}
    for s in SOURCES:
        src = os.path.join(CSRC, s)
        obj = os.path.join(objdir, s.replace('.hip', '.o'))
        if force or _stale(obj, [src] + sorted(_includes(src))):
            gone = set(drop.get(s, [])) | set(drop.get('*', []))
            flags = [f for f in FLAGS + EXTRA.get(s, []) if f not in gone] + extra.get(s, []) + extra.get('*', [])
            jobs.append([cc] + flags + ['-c', src, '-o', obj])

    def run(cmd):
        if verbose:
            print(' '.join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError('hipcc failed:\n' + ' '.join(cmd) + '\n' + r.stdout + r.stderr)
        return r.stderr

    with ThreadPoolExecutor(max_workers=4) as ex:
        for err in ex.map(run, jobs):
            if verbose and err.strip():
                print(err)
    objs = [os.path.join(objdir, s.replace('.hip', '.o')) for s in SOURCES]
    if force or jobs or _stale(out, objs):
        run([cc, '-shared', '-fPIC', f'--offload-arch={ARCH}', '-o', out] + objs)
    return out


if __name__ == '__main__':
    print(build(force='--force' in sys.argv, verbose=True))
