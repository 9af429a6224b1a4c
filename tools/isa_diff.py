"""Compare the gfx950 ISA of two source trees, kernel by kernel: the evidence that a refactor left the device code alone.

    python tools/isa_diff.py [--diff] <old tree> <new tree> [file.hip ...]      # no GPU needed; ~3 s per file and tree

Every file of each tree's own build.SOURCES (or the files named) is compiled with that tree's build.FLAGS plus
`--cuda-device-only -S`.  The listings are normalised -- comments, `.file` / `.ident` lines and `__hip_cuid_*` symbols dropped, the
numbers of local labels dropped -- and every function symbol (the kernels and what the compiler did not inline) gets one verdict:

    identical    the normalised listings match, kernel descriptor included
    scalar-only  the instructions whose mnemonic does not start with `s_` are the same sequence and the descriptor agrees in
                 everything but its scalar-register counts: only scalar bookkeeping (loop counters, addresses, waits) differs.
                 Vector and memory instructions are compared with the NUMBERS of their scalar-register operands dropped, since
                 different bookkeeping hands them the same values in other registers.
    different    anything else

Exit status 1 if a symbol is `different` or exists in one tree only.  --diff prints the unified diff of every listing that is not
identical.
"""
import difflib
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

PKG = 'cvpr2025-decafnet_amd'


def load_build(tree):
    spec = importlib.util.spec_from_file_location('build_' + re.sub(r'\W', '_', os.path.abspath(tree)), os.path.join(tree, PKG, 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def listing(build, name, tmp):
    out = os.path.join(tmp, name.replace('.hip', '.s'))
    cmd = [build.hipcc()] + build.FLAGS + build.EXTRA.get(name, []) + ['--cuda-device-only', '-S', os.path.join(build.CSRC, name), '-o', out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError('hipcc failed:\n' + ' '.join(cmd) + '\n' + r.stdout + r.stderr)
    with open(out) as f:
        return f.read()


def normalise(text):
    lines = []
    for l in text.split('\n'):
        l = l.split(';', 1)[0].rstrip()
        if not l.strip() or re.match(r'\s*\.(file|ident)\b', l) or '__hip_cuid_' in l:
            continue
        lines.append(re.sub(r'(\.L[A-Za-z_]*?)[0-9_]+\b', r'\1', l))
    return lines


def functions(lines):
    """{symbol: (body lines, descriptor lines)}: the body runs from the symbol's label to its .Lfunc_end label, the descriptor is
    the .amdhsa_kernel block of a kernel (empty for other functions)"""
    syms = [m.group(1) for l in lines for m in [re.match(r'\s*\.type\s+(\S+),@function', l)] if m]
    out = {}
    for s in syms:
        start = lines.index(s + ':')
        end = next(i for i in range(start, len(lines)) if lines[i].startswith('.Lfunc_end'))
        desc = []
        if '\t.amdhsa_kernel ' + s in lines:
            d0 = lines.index('\t.amdhsa_kernel ' + s)
            desc = lines[d0:lines.index('\t.end_amdhsa_kernel', d0)]
        out[s] = (lines[start + 1:end], desc)
    return out


def is_instruction(l):
    s = l.strip()
    return l[:1].isspace() and not s.startswith('.') and not s.endswith(':')


def vector_sequence(body):
    seq = [l.strip() for l in body if is_instruction(l) and not l.strip().startswith('s_')]
    return [re.sub(r'\bs\[\d+:\d+\]', 's[:]', re.sub(r'\bs\d+\b', 's', l)) for l in seq]


def verdict(old, new):
    if old == new:
        return 'identical'
    scalar_desc = lambda d: [l for l in d if 'sgpr' not in l]
    if vector_sequence(old[0]) == vector_sequence(new[0]) and scalar_desc(old[1]) == scalar_desc(new[1]):
        return 'scalar-only'
    return 'different'


def note(old, new):
    """what a `different` pair still has in common, for the reader: it does not change the verdict"""
    if sorted(vector_sequence(old[0])) == sorted(vector_sequence(new[0])):
        return 'the same vector and memory instructions, register for register, in another order'
    return ''


def compare_file(builds, name, tmp):
    fns = []
    for i, b in enumerate(builds):
        d = os.path.join(tmp, str(i))
        os.makedirs(d, exist_ok=True)
        fns.append(functions(normalise(listing(b, name, d))))
    rows = [(s, verdict(fns[0][s], fns[1][s]) if s in fns[0] and s in fns[1] else ('removed' if s in fns[0] else 'added'),
             sum(map(is_instruction, fns[0][s][0])) if s in fns[0] else 0, sum(map(is_instruction, fns[1][s][0])) if s in fns[1] else 0)
            for s in sorted(set(fns[0]) | set(fns[1]))]
    diffs = {s: list(difflib.unified_diff(fns[0][s][0] + fns[0][s][1], fns[1][s][0] + fns[1][s][1], 'old', 'new', lineterm='', n=2))
             for s, v, _, _ in rows if v in ('scalar-only', 'different')}
    notes = {s: note(fns[0][s], fns[1][s]) for s, v, _, _ in rows if v == 'different'}
    return name, rows, diffs, notes


def demangle(sym):
    tool = shutil.which('c++filt') or shutil.which('llvm-cxxfilt')
    r = subprocess.run([tool, sym], capture_output=True, text=True) if tool else None
    return r.stdout.strip() if r and r.returncode == 0 and r.stdout.strip() else sym


def main(argv):
    show = '--diff' in argv
    argv = [a for a in argv if a != '--diff']
    if len(argv) < 2:
        print(__doc__)
        return 2
    builds = [load_build(argv[0]), load_build(argv[1])]
    names = argv[2:] or [s for s in builds[1].SOURCES if s in builds[0].SOURCES]
    for s in set(builds[0].SOURCES) ^ set(builds[1].SOURCES):
        print(f'{s}: in one tree only')
    bad = len(set(builds[0].SOURCES) ^ set(builds[1].SOURCES)) if not argv[2:] else 0
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=int(os.environ.get('MAX_JOBS', '8'))) as ex:
        for name, rows, diffs, notes in ex.map(lambda n: compare_file(builds, n, tmp), names):
            count = {}
            for _, v, _, _ in rows:
                count[v] = count.get(v, 0) + 1
            print(f'{name:24s} ' + (', '.join(f'{n} {v}' for v, n in sorted(count.items())) or 'no device functions'), flush=True)
            for s, v, n0, n1 in rows:
                if v != 'identical':
                    print(f'    {v:11s} {demangle(s)}   ({n0} -> {n1} instructions)' + (': ' + notes[s] if notes.get(s) else ''))
                    bad += v != 'scalar-only'
                    if show:
                        print('\n'.join('        ' + l for l in diffs.get(s, [])))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
