"""Device code of two trees, compared from the compiler's assembly.

    for u in csrc/*.hip: hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S $u -o DIR/$(basename $u .hip).s
    python tools/asm_compare.py PARENT_DIR THIS_DIR

Per translation unit: `identical file` (but for the name of the __hip_cuid_<hash> marker object, a hash of the source path), or -- host code that instantiates its kernels in another order permutes the file and
renumbers the per-function local labels -- a comparison per kernel symbol: the instruction stream and the .amdhsa_ kernel
descriptor of every symbol with comments stripped and the function number taken out of local labels (.LBB<n>_<m> -> .LBB_<m>).
Exit status 1 if any unit differs in its set of symbols or in a kernel's code."""
import os
import re
import sys


def functions(path):
    """{symbol: normalised text of the function (label to .Lfunc_end, the .amdhsa_kernel block included)}"""
    out, sym, body = {}, None, []
    for ln in open(path):
        m = re.match(r'\s*\.type\s+(\S+),@function', ln)
        if m:
            sym, body = m.group(1), []
            continue
        if sym is None:
            continue
        if re.match(r'\.Lfunc_end\d+:', ln):
            out[sym] = '\n'.join(body)
            sym = None
            continue
        ln = ln.split(';', 1)[0].rstrip()
        ln = re.sub(r'\.L([A-Za-z_]+?)\d+(_\d+)\b', r'.L\1\2', ln)
        if ln.strip() and not re.match(r'\s*\.section\b', ln):
            body.append(ln)
    return out


def main():
    pa, th = sys.argv[1], sys.argv[2]
    units = sorted(f for f in os.listdir(pa) if f.endswith('.s'))
    assert units == sorted(f for f in os.listdir(th) if f.endswith('.s')), 'the two directories hold different units'
    bad = 0
    for u in units:
        a, b = os.path.join(pa, u), os.path.join(th, u)
        whole = lambda p: re.sub(rb'__hip_cuid_[0-9a-f]+', b'__hip_cuid_', open(p, 'rb').read())
        if whole(a) == whole(b):
            print('%-18s identical file (%d bytes)' % (u, os.path.getsize(a)))
            continue
        fa, fb = functions(a), functions(b)
        kernels = sum('.amdhsa_kernel' in t for t in fa.values())
        only = sorted(set(fa) ^ set(fb))
        diff = sorted(s for s in set(fa) & set(fb) if fa[s] != fb[s])
        order = 'same order' if list(fa) == list(fb) else 'other order'
        print('%-18s files differ; per symbol: %d functions (%d kernels) / %d, %s, %d only in one tree, %d with other code'
              % (u, len(fa), kernels, len(fb), order, len(only), len(diff)))
        for s in (only + diff)[:20]:
            print('    %s %s' % ('only in one:' if s in only else 'code differs:', s))
        bad += len(only) + len(diff)
    print('RESULT: %s' % ('device code equal in every unit' if not bad else '%d symbols differ' % bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
