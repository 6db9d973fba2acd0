"""Digest of the launch sequence in a rocprofv3 kernel trace (CSV): one line per dispatch in dispatch order,
(kernel name, grid, workgroup, LDS bytes), sha256 over the lines.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o NAME -- python -m pytest ...
    python tools/launch_digest.py DIR/.../NAME_kernel_trace.csv OUT.json [SEQUENCE.txt]
    python tools/launch_digest.py SEQUENCE.txt OUT.json
    python tools/launch_digest.py --compare A.json B.json [A_SEQUENCE.txt B_SEQUENCE.txt]

Two digests: every dispatch, and the dispatches of this library's kernels alone (everything but the tensor library's own
kernels and the HIP runtime's copy kernels, recognised by their names)."""
import csv
import hashlib
import json
import re
import sys

FOREIGN = re.compile(r'\b(at|c10|rocprim|hipcub|thrust|cub)::|^Cijk_|^__amd_rocclr_')      # (__amd_rocclr_*: the HIP runtime's copy / fill kernels)


def rows(path):
    with open(path, newline='') as f:
        rd = csv.DictReader(f)
        col = {c.lower(): c for c in rd.fieldnames}
        pick = lambda *names: next(col[n] for n in names if n in col)
        name, order = pick('kernel_name'), pick('dispatch_id', 'start_timestamp')
        dims = [pick('grid_size_' + a) for a in 'xyz'] + [pick('workgroup_size_' + a) for a in 'xyz']
        lds = pick('lds_block_size', 'lds_block_size_v', 'group_segment_size')
        out = [(int(r[order]), r[name], tuple(int(r[d]) for d in dims), int(r[lds])) for r in rd]
    out.sort(key=lambda t: t[0])
    return ['%s grid %d,%d,%d wg %d,%d,%d lds %d' % ((n,) + d + (l,)) for _, n, d, l in out]


def digest(lines):
    return hashlib.sha256('\n'.join(lines).encode()).hexdigest()


def main():
    if sys.argv[1] == '--compare':
        a, b = json.load(open(sys.argv[2])), json.load(open(sys.argv[3]))
        for k in ('dispatches', 'digest', 'library_dispatches', 'library_digest', 'library_kernels'):
            print('%-20s %s  %s  %s' % (k, a[k], b[k], 'equal' if a[k] == b[k] else 'DIFFERENT'))
        if len(sys.argv) > 5 and a['digest'] != b['digest']:
            la, lb = open(sys.argv[4]).read().split('\n'), open(sys.argv[5]).read().split('\n')
            i = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
            print('first difference at dispatch %d:\n  %s\n  %s' % (i, la[i] if i < len(la) else '(end)', lb[i] if i < len(lb) else '(end)'))
        return 0 if a['library_digest'] == b['library_digest'] else 1
    seq = open(sys.argv[1]).read().split('\n') if sys.argv[1].endswith('.txt') else rows(sys.argv[1])      # (.txt: a SEQUENCE file written earlier)
    own = [s for s in seq if not FOREIGN.search(s)]
    json.dump({'dispatches': len(seq), 'digest': digest(seq), 'library_dispatches': len(own), 'library_digest': digest(own),
               'library_kernels': len({s.split(' grid ')[0] for s in own})}, open(sys.argv[2], 'w'), indent=1)
    if len(sys.argv) > 3:
        open(sys.argv[3], 'w').write('\n'.join(seq))
    return 0


if __name__ == '__main__':
    sys.exit(main())
