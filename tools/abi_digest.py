"""Digest of what the C ABI computes: the sha256 of every `out` / `inout` operand of every operator case, for comparing two builds of
the library bit for bit (a refactor that must not change a result).

    python tools/abi_digest.py [--out DIR] [name=path/to/libdecafnet_hip.so ...]      # DIR: default build/digest of the package

Cases: every entry of every case table of tests/borders.TABLE (the base table of tests/abi_cases.py and the train, dist, attn, front,
guard, clock, half and front_half extension tables in the same format), under the key `<export>-<tag>`, run once on plain tensors (tests/arena.plain_operands: `out` operands start from the sentinel, so a part an export leaves alone hashes equal),
and MANY_PARTS below: for each user of the fixed-order blocked sum (blocked_sum, csrc/grad_common.h) the smallest shape whose number
of partials lies in 9 .. 63 and the smallest with more than 64, so that all three levels of the tree carry data.  The part counts
are read off the slicing constants of the kernels and recorded in the JSON.

Each library runs in a child process of its own (DCF_LIB_PATH, read by _lib.py at import; no name=path: the in-tree build as `tree`),
one after the other, each under `timeout`; a child that fails ends the run.  Writes <out>/<name>.json and, for two or more
libraries, compares them entry for entry against the first: exit status 1 on any difference."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_LIMIT = 420        # seconds


def ceil_div(a, b):
    return (a + b - 1) // b


def many_parts():
    """[(export, tag, parts, make)]; parts = the nparts the reduce kernel of that export gets at this shape"""
    import abi_cases as A
    import front_abi_cases as F
    import train_abi_cases as T
    column = lambda rows: ceil_div(rows, 4 * ceil_div(rows, 4 * 512))        # EG_MAX_WG = 512 workgroups of four waves; k_ln_bwd alike
    L = []
    # k_cg_reduce (conv_grad.hip): CG_SMALL_SLICE = 256 rows per slice for N <= 2; at most CG_MAX_SLICES = 64 slices of a multiple of
    # 32 rows on the matrix cores (so never more than 64 there); LayerNorm's dw / db over the workgroups of k_ln_bwd
    for rows in (2049, 16385):
        L.append(('dcf_op_conv_bwd_weight', f'1x{rows}-32-1-k3', ceil_div(rows, 256), A._conv_bwd_weight(1, rows, 32, 1, 3, 0)))
    L.append(('dcf_op_conv_bwd_weight', '1x257-32-32-k3', ceil_div(257, 32 * ceil_div(ceil_div(257, 64), 32)), A._conv_bwd_weight(1, 257, 32, 32, 3, 0)))
    for rows in (33, 257):
        L.append(('dcf_op_layernorm_bwd', f'{rows}x32', column(rows), A._layernorm_bwd(rows, 32, 0, 0)))
    # k_eg_reduce (enc_grad.hip, and drop_grad.hip through launch_eg_reduce): the workgroups of the column reductions
    for rows in (33, 257):
        L.append(('dcf_op_dwconv3_bwd', f'1x{rows}-32-n1-s1', column(rows), A._dwconv3(1, rows, 32, 1, 1, bwd=True)))
        L.append(('dcf_op_layerscale_residual_bwd', f'{rows}x32', column(rows), A._lsres(rows, 32, 1, 1, bwd=True)))
        L.append(('dcf_op_drop_residual_bwd', f'1x{rows}x32', column(rows), T._residual_bwd(1, rows, 32, 0, 0.5, 0.0, 1, 1, 'rhs', 0)))
    # k_xg_reduce (xattn_grad.hip): XG_SLICE_ROWS = 512 query rows per slice
    for t in (4097, 32769):
        L.append(('dcf_op_xattn_bwd', f'1x{t}-k2-16-h1', ceil_div(t, 512), A._xattn(1, t, 2, 16, 1, bwd=True)))
    # k_rg_reduce / k_refine_in_reduce (refine_grad.hip): RG_SLICE_ROWS = 128
    for rows in (1025, 8193):
        L.append(('dcf_op_tcn_layer_bwd', f'1x{rows}-d1', ceil_div(rows, 128), A._tcn_layer(1, rows, 1, 0.0, bwd=True)))
        L.append(('dcf_op_refine_in_bwd', f'1x{rows}-L1', ceil_div(rows, 128), A._refine_in(1, rows, 1, bwd=True)))
    # k_fg_reduce (front_grad.hip, the rolled form): one slice of slice_t = 64 clips per video while T <= 64
    for nvid in (9, 65):
        L.append(('dcf_op_vidmap_shared_bwd', f'T64-E64-{nvid}videos', nvid, F._backward([1] * nvid, 32, 64, 64, False, False, True, 0)))
    return L


def child(out_path):
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
    import torch
    import arena
    import borders
    ctx = borders.Ctx()
    check = ctx.pkg._lib.check
    digest, parts = {}, {}

    def run(key, export, make, options=()):
        made = make()
        specs, call = made[0], made[1]
        views, keep = arena.plain_operands(specs, 'cuda')
        if len(made) > 2 and made[2] is not None:
            made[2](views, lambda name, t: views[name].copy_(t))
        try:
            for name, value in options:
                check(ctx.lib.dcf_debug_set_option(name.encode(), value), 'dcf_debug_set_option')
            check(call(ctx, views), export)
            torch.cuda.synchronize()
        finally:
            for name, _ in options:
                check(ctx.lib.dcf_debug_set_option(name.encode(), -1), 'dcf_debug_set_option')
        assert key not in digest, key
        digest[key] = {name: hashlib.sha256(views[name].contiguous().reshape(-1).view(torch.uint8).cpu().numpy().tobytes()).hexdigest()
                       for name, _, role, *_ in specs if role != 'in'}

    for row in borders.TABLE.values():
        for c in row.cases.CASES:
            run(f'{c.export}-{c.tag}', c.export, c.make, c.options)
    for export, tag, n, make in many_parts():
        run(f'many-parts:{export}-{tag}', export, make)
        parts[f'many-parts:{export}-{tag}'] = n
    ctx.close()
    with open(out_path, 'w') as f:
        json.dump({'library': ctx.pkg._lib.SO_PATH, 'cases': len(digest), 'parts': parts, 'digest': digest}, f, indent=1, sort_keys=True)
    print(f'{len(digest)} cases, {sum(map(len, digest.values()))} operands -> {out_path}', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'cvpr2025-decafnet_amd', 'build', 'digest'))     # (build/ is git-ignored)
    ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
    ap.add_argument('libs', nargs='*', help='name=path of a libdecafnet_hip.so; none: the in-tree build')
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    os.makedirs(args.out, exist_ok=True)
    libs = [a.split('=', 1) for a in args.libs] or [['tree', '']]
    results = []
    for name, path in libs:
        env = dict(os.environ)
        if path:
            assert os.path.exists(path), path
            env['DCF_LIB_PATH'] = os.path.abspath(path)
        else:
            env.pop('DCF_LIB_PATH', None)
        out = os.path.join(args.out, name + '.json')
        cmd = ['timeout', '-k', '10', str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), '--child', out]
        rc = subprocess.run(cmd, env=env).returncode
        if rc != 0:                           # a fault, an abort or the time limit: nothing more is started on the GPU
            sys.exit(rc)
        with open(out) as f:
            results.append((name, json.load(f)))
    bad = 0
    base_name, base = results[0]
    for name, r in results[1:]:
        keys = sorted(set(base['digest']) | set(r['digest']))
        diff = [k for k in keys if base['digest'].get(k) != r['digest'].get(k)]
        print(f'{name} against {base_name}: {len(keys)} cases, ' + ('all equal' if not diff else f'{len(diff)} differ: ' + ', '.join(diff[:20])))
        bad += len(diff)
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
