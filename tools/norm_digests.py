"""sha256 of every output of the BatchNorm / channel-sum entry points of ONE given libfami_hip.so, to compare two builds of
csrc/norm.hip bit for bit (a differing digest = a rounding moved).  One library per process.

usage: python tools/norm_digests.py LIB OUT.json [FULL.json]

OUT.json holds one digest per (case, storage type, operand kind): the sha256 over the sorted "output name: sha256" lines of
that group, with the number of outputs; FULL.json, if given, every output's own digest (to find which one moved).

Cases: the table of tests/_norm_exact.py on its integer operands (every entry point, the fp64-atomics forms included: the
sums are exact there), plus the same shapes on seeded random floats generated on the CPU, for the entry points whose sums
are taken in a fixed order (three-launch forms, one-launch kernels, eval_bwd, apply, the slot apply passes on host-written
rows, channel_sum, running_update*).  Prototypes come from include/fami.h through fami_pose_amd._lib.parse_header."""
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
os.environ.setdefault('HIP_FORCE_DEV_KERNARG', '1')

import torch  # noqa: E402
from fami_pose_amd._lib import parse_header  # noqa: E402
from _norm_exact import CASES, Runner, case_id, make_case  # noqa: E402


class Lib:
    """the given library behind the two members tests/_norm_exact.Runner uses: .cdll and .call"""

    def __init__(self, path):
        self.cdll = ctypes.CDLL(os.path.abspath(path))
        self.protos = parse_header()
        for name, (restype, argtypes) in self.protos.items():
            fn = getattr(self.cdll, name)
            fn.restype, fn.argtypes = restype, argtypes

    def call(self, name, *args):
        rc = getattr(self.cdll, name)(*args)
        if self.protos[name][0] is ctypes.c_int and rc != 0:
            raise RuntimeError('%s failed (%d): %s' % (name, rc, self.cdll.fami_last_error().decode()))
        return rc


def main(lib_path, out_path, full_path=None):
    L, dev = Lib(lib_path), torch.device('cuda:0')
    digests = {}
    for case in CASES:
        P, C, tune = case
        for dt in ('f32', 'bf16', 'f16'):
            for integers in (True, False):
                if tune is not None:
                    L.call('fami_bn_tune_small', tune)
                try:
                    r = Runner(L, dev, dt, make_case(P, C, integers))
                    outs = r.run_deterministic() + (r.run_atomic() if integers else [])
                    torch.cuda.synchronize(dev)
                finally:
                    if tune is not None:
                        L.call('fami_bn_tune_small', -1)
                assert not r.A.touched(), r.A.touched()
                for nm, got, _, _ in outs:
                    key = '%s %s %s %s' % (case_id(case), dt, 'int' if integers else 'float', nm)
                    assert key not in digests, key
                    digests[key] = hashlib.sha256(got.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()
    with open(out_path, 'w') as f:
        json.dump(fold(digests), f, indent=0, sort_keys=True)
    if full_path:
        with open(full_path, 'w') as f:
            json.dump(digests, f, indent=0, sort_keys=True)
    print('%d digests in %d groups -> %s' % (len(digests), len(fold(digests)), out_path))


def fold(digests):
    """{'case dtype kind': 'n outputs, sha256 of their sorted "name: digest" lines'}"""
    groups = {}
    for key in sorted(digests):
        case, dt, kind, name = key.split(' ', 3)
        groups.setdefault('%s %s %s' % (case, dt, kind), []).append('%s: %s\n' % (name, digests[key]))
    return {g: '%d outputs, %s' % (len(v), hashlib.sha256(''.join(v).encode()).hexdigest()) for g, v in groups.items()}


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
