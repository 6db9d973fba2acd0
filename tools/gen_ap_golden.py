"""Writes tests/golden/posetrack_ap.npz: the reference's OWN evaluateAP (poseval/py/evaluateAP.py:37-47, after its
cleanupData and removeIgnoredPoints, eval_helpers.py:305-367) on seeded frames.  Runs only where the reference tree is
present (oracle.ref_harness); nothing of the reference enters the repository, only the numbers it computes.

    python tools/gen_ap_golden.py

The reference's modules are loaded by path as a package of their own.  What they import and this environment lacks
(shapely, termcolor, click, tqdm, motmetrics, and tabulate if absent) is replaced by stand-in modules in sys.modules that
hold nothing: the AP path calls none of them.  shapely being one of them, the frames carry NO ignore regions (the
reference's point filter would need it); the even-odd filter is tested against the restatement only.

Fixture: 200 seeded frames stated as annolists (tests/_ap_ref.make_annolists, seed below; coordinates on a 1/8 pixel
grid and scores on a 2^-24 grid, so that the file stays small; every rect carries a track_id, which assignGTmulti
indexes), stored as the packed arrays of evaluate.pack_posetrack_frames (pr_xys, gt_xy, gt_head as float32, which holds
every value on those grids exactly; pr_has, gt_has, pr_seg, gt_seg, frame_index, n_frames) and the reference's apAll /
preAll / recAll [16] float64.
The tool refuses to write a fixture when
  * the float64 restatement (tests/_ap_ref.evaluate_ap) disagrees with the reference by more than 1e-9 (0-100 scale);
  * the smallest decision margin min |dist - 0.5| / 0.5 is below 1e-9 (one subtraction, one sqrt and one division in fp64
    are a few ulp ~ 1e-15 relative: six orders of room);
  * two predictions of one joint have equal scores (the reference's argsort leaves their order open);
  * the total AP lies outside 20 .. 80;
  * there is no prediction within the threshold of some joint yet left unassigned because another prediction took its
    pose, no frame with predictions and no annotated pose left, or no annotated pose nobody matched."""
import copy
import importlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(ROOT, 'tests', 'golden', 'posetrack_ap.npz')
SEED = 7
FRAMES = 200
STANDINS = ('shapely', 'termcolor', 'click', 'tqdm', 'motmetrics', 'tabulate')


class _Nothing:
    """What an attribute of a stand-in module is: usable as a decorator factory at import time, never called for a value."""

    def __call__(self, *a, **k):
        return self

    def __getattr__(self, name):
        return self


class _StandIn(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith('__'):
            raise AttributeError(name)
        return _Nothing()


def load_reference():
    """-> (eval_helpers, evaluateAP) modules of the reference, imported as the package `_reference_poseval`."""
    from oracle import ref_harness
    if not ref_harness.available():
        raise SystemExit('gen_ap_golden needs the reference tree (oracle.ref_harness.available() is False)')
    for name in STANDINS:
        try:
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = _StandIn(name)
    pkg = types.ModuleType('_reference_poseval')
    pkg.__path__ = [os.path.join(ref_harness.REF, 'datasets', 'zoo', 'posetrack', 'posetrack_utils', 'poseval', 'py')]
    sys.modules['_reference_poseval'] = pkg
    return (importlib.import_module('_reference_poseval.eval_helpers'),
            importlib.import_module('_reference_poseval.evaluateAP'))


def reference_ap(eh, eap, gt, pr):
    """The reference's load_data_dir after the files are read, then evaluateAP, on copies -> ap, pre, rec [16]."""
    import _ap_ref as ar
    g, p = eh.cleanupData(copy.deepcopy(gt), copy.deepcopy(pr))
    g, p = eh.removeIgnoredPoints(g, p)
    ap, pre, rec = eap.evaluateAP(g, p)
    return ap[:, 0].copy(), pre[:, 0].copy(), rec[:, 0].copy()


def main(seed=SEED):
    import _ap_ref as ar
    from fami_pose_amd import evaluate as ev
    eh, eap = load_reference()
    rng = np.random.RandomState(seed)
    gt, pr = ar.make_annolists(rng, FRAMES, max_people=3, grid=2.0 ** -3)
    ap, pre, rec = reference_ap(eh, eap, gt, pr)
    mine = ar.evaluate_ap(gt, pr)
    err = max(float(np.nanmax(np.abs(mine[k] - v))) for k, v in (('ap', ap), ('pre', pre), ('rec', rec)))
    print('seed %d: %d frames kept, %d predicted / %d annotated poses, total AP %.3f, restatement off by %.3e, margin %.3e'
          % (seed, len(mine['frame_index']), len(mine['pr_has']), len(mine['gt_has']), ap[15], err, mine['margin']))
    assert err <= 1e-9 and all(np.array_equal(np.isnan(mine[k]), np.isnan(v)) for k, v in (('ap', ap), ('pre', pre), ('rec', rec)))
    assert mine['margin'] >= 1e-9
    assert all(len(set(s)) == len(s) for s in mine['scores']), 'equal scores within a joint'
    assert 20.0 <= ap[15] <= 80.0
    cases = {k: mine[k] for k in ('outcompeted', 'empty_gt_frames', 'unmatched_gt')}
    print(cases)
    assert min(cases.values()) >= 1, cases
    packed = ev.pack_posetrack_frames(gt, pr)
    assert len(packed['verts']) == 0 and np.array_equal(packed['frame_index'], mine['frame_index'])
    out = {k: packed[k] for k in ('pr_has', 'gt_has', 'pr_seg', 'gt_seg', 'frame_index')}
    for k in ('pr_xys', 'gt_xy', 'gt_head'):                     # on the grids every value is an fp32 number: stored as such
        out[k] = packed[k].astype(np.float32)
        assert np.array_equal(out[k].astype(np.float64), packed[k])
    out.update({'n_frames': np.int64(FRAMES), 'ap': ap, 'pre': pre, 'rec': rec})
    np.savez_compressed(OUT, **out)
    print('wrote %s (%d bytes)' % (OUT, os.path.getsize(OUT)))


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else SEED)
