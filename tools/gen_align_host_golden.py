"""Records tests/golden/align_host.json: the tables of tests/test_align_host.py run against a built library.

    python tools/gen_align_host_golden.py --commit <sha of the tree the library was built from> [--lib path/to/libfami_hip.so]

Needs no GPU: every refusal of the table comes before any HIP call (a case that does not stops the recording) and the queries are
host arithmetic."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', required=True)
    ap.add_argument('--lib', default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'align_host.json'))
    a = ap.parse_args()
    from fami_pose_amd import _lib
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    import test_align_host as T
    L = _lib.lib()
    refusals = T.run_refusals(L)
    for cid, (rc, text) in refusals.items():
        assert rc in (-1, -2), 'case %s reached the runtime (%d, %s): take it out of the table' % (cid, rc, text)
    queries, wrong = T.run_queries(L)
    assert not wrong, wrong
    json.dump({'commit': a.commit, 'library': 'libfami_hip.so built from that commit (make -C fami-pose_amd/csrc)',
               'refusals': refusals, 'queries': queries}, open(a.out, 'w'), indent=0, sort_keys=True)
    print('%d refusals, %d queries x %d settings -> %s' % (len(refusals), len(T.query_table()), len(queries), a.out))


if __name__ == '__main__':
    main()
