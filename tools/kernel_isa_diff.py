#!/usr/bin/env python3
"""Do two builds of csrc/ hold the same kernels, instruction for instruction?  CPU only: hipcc cross-compiles.

usage: python tools/kernel_isa_diff.py PARENT_CSRC HEAD_CSRC

Every *.hip of both directories is compiled with its own Makefile's CXXFLAGS plus --cuda-device-only -S; each .s is cut at
the kernel symbols (NAME: up to .Lfunc_end), comments go, and the compiler's local label numbers (.LBB<n>_, .LJTI<n>_,
.Ltmp<n>) are normalised, since they count functions and labels of the whole translation unit.  Per kernel, whichever file
holds it, the instruction lines and the .amdhsa_ descriptor lines (LDS, VGPR / SGPR / AGPR counts, scratch) are compared.
Prints `same N`, every `DIFF <kernel>` with its first differing lines, every kernel present on one side only; exit status 1
on any of those.  (PARENT_CSRC must sit in a tree with include/, e.g. `git worktree add` or `git archive | tar -x`.)"""
import difflib, pathlib, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor


def make_var(makefile, name):
    m = re.search(r'^%s\s*\??=\s*((?:.*\\\n)*.*)$' % name, makefile, re.M)
    return m.group(1).replace('\\\n', ' ').strip()


def compile_tree(csrc, out):
    mk = (csrc / 'Makefile').read_text()
    flags = make_var(mk, 'CXXFLAGS').replace('$(ARCH)', make_var(mk, 'ARCH')).split()
    def one(src):
        dst = out / (src.stem + '.s')
        r = subprocess.run([make_var(mk, 'HIPCC'), *flags, '--cuda-device-only', '-S', src.name, '-o', str(dst)], cwd=csrc,
                           stderr=subprocess.PIPE, text=True)
        if r.returncode:
            sys.exit('%s: hipcc failed\n%s' % (src, r.stderr))
        return dst
    with ThreadPoolExecutor(8) as pool:
        return list(pool.map(one, sorted(csrc.glob('*.hip'))))


def kernels_of(asm_files):
    """{kernel name: normalised instruction lines + descriptor lines}"""
    found = {}
    for path in asm_files:
        body, desc, cur, cur_desc, func = {}, {}, None, None, None
        for raw in path.read_text().splitlines():
            line = raw.split(';', 1)[0].strip()
            if not line:
                continue
            m = re.fullmatch(r'\.type\s+(\w+),@function', line)
            if m:
                func = m.group(1)
            elif line.startswith('.amdhsa_kernel '):          # the descriptor sits inside its function, after the code
                cur_desc = line.split()[1]; desc[cur_desc] = []
            elif line == '.end_amdhsa_kernel':
                cur_desc = None
            elif cur_desc is not None:
                desc[cur_desc].append(line)
            elif cur is None and line == '%s:' % func:
                cur = func; body[cur] = []
            elif cur is not None and line.startswith('.Lfunc_end'):
                cur = None
            elif cur is not None:
                body[cur].append(line)
        for name, d in desc.items():
            text = '\n'.join(body[name])
            text = re.sub(r'\.(LBB|LJTI)\d+_', r'.\1_', text)
            tmps = {}
            text = re.sub(r'\.Ltmp\d+', lambda t: tmps.setdefault(t.group(0), '.Ltmp#%d' % len(tmps)), text)
            key = name if name not in found else '%s@%s' % (name, path.stem)
            found[key] = text.split('\n') + d
    return found


def main(parent, head):
    with tempfile.TemporaryDirectory() as tmp:
        sides = []
        for tag, csrc in (('parent', parent), ('head', head)):
            out = pathlib.Path(tmp) / tag
            out.mkdir()
            sides.append(kernels_of(compile_tree(pathlib.Path(csrc).resolve(), out)))
    a, b = sides
    same = [k for k in a if k in b and a[k] == b[k]]
    bad = 0
    for k in sorted(a.keys() & b.keys()):
        if a[k] != b[k]:
            bad += 1
            print('DIFF', k)
            for ln in list(difflib.unified_diff(a[k], b[k], 'parent', 'head', lineterm='', n=1))[:12]:
                print('   ', ln)
    for tag, only in (('parent', a.keys() - b.keys()), ('head', b.keys() - a.keys())):
        for k in sorted(only):
            bad += 1
            print('ONLY in', tag, k)
    print('same', len(same))
    return 1 if bad or not same else 0          # no kernel found at all is no pass either


if __name__ == '__main__':
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
