"""Records tests/golden/conv_refusals.json: the table of tests/test_conv_refusals_host.py run against a built library.

    python tools/gen_conv_refusals_golden.py --commit <sha of the tree the library was built from> [--lib path/to/libfami_hip.so]

Needs no GPU: every case of the table is refused before any HIP call (a case that is not stops the recording)."""
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'conv_refusals.json'))
    a = ap.parse_args()
    from fami_pose_amd import _lib
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    import test_conv_refusals_host as T
    L = _lib.lib()
    L.cdll.fami_tune_reset()
    got = T.run(L)
    for cid, (rc, text) in got.items():
        assert rc in (-1, -2), 'case %s reached the runtime (%d, %s): take it out of the table' % (cid, rc, text)
    json.dump({'commit': a.commit, 'library': 'libfami_hip.so built from that commit (make -C fami-pose_amd/csrc)',
               'cases': got}, open(a.out, 'w'), indent=1, sort_keys=True)
    print('%d cases -> %s' % (len(got), a.out))


if __name__ == '__main__':
    main()
