"""Writes tests/golden/pose_nms.npz: the reference's OWN oks_nms / soft_oks_nms (datasets/process/nms.py:89-192) on
seeded detections.  Runs only where the reference tree is present (oracle.ref_harness); nothing of the reference enters
the repository, only the arrays it computes.

    python tools/gen_nms_golden.py

nms.py is loaded by its file path: the package `datasets.process` imports cv2 in its __init__, the module itself needs
numpy only.  The reference's functions take a per-detection score; that score is the HRNet rescoring rule
(tests/_nms_ref.rescore at IN_VIS_THRE 0.2, Base_PoseTrack17.yaml), which nms.py does not contain, so the file stores
the box scores and the scores that were fed.

Fixture: M = 12 images of 1 ... 40 detections (tests/_nms_ref.make_dets, seed below), N detections in all, every value
fp32-representable: kpts [N,17,3], area [N], box_score [N] float32, seg [M+1] (image m owns rows seg[m] .. seg[m+1]),
in_vis_thre, score [N] float64, cases [8,4] float64 = (soft, vis_thr or NaN for none, thr, max_dets), and per case c
keep_c (positions within the image, concatenated over the images, in the reference's pick order) with kseg_c [M+1].
The tool refuses to write a fixture on which the float64 restatement disagrees with the reference, whose decision margin
is below 1e-4, or which lacks a suppression, a survivor behind a suppressed detection, or an image where vis_thr
changes the result."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(ROOT, 'tests', 'golden', 'pose_nms.npz')
SEED = 10
SIZES = (1, 2, 3, 5, 8, 12, 17, 20, 21, 26, 33, 40)
IN_VIS_THRE = 0.2
CASES = [(soft, vis, thr, 20) for soft in (0, 1) for vis in (None, 0.2) for thr in (0.5, 0.9)]


def main(seed=SEED):
    from oracle import ref_harness
    import _nms_ref as nr
    if not ref_harness.available():
        raise SystemExit('gen_nms_golden needs the reference tree (oracle.ref_harness.available() is False)')
    spec = importlib.util.spec_from_file_location('_reference_nms',
                                                  os.path.join(ref_harness.REF, 'datasets', 'process', 'nms.py'))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    rng = np.random.RandomState(seed)
    parts = [nr.make_dets(rng, n) for n in SIZES]
    kpts = np.concatenate([p[0] for p in parts])
    area = np.concatenate([p[1] for p in parts])
    bs = np.concatenate([p[2] for p in parts])
    seg = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
    score = nr.rescore(kpts, bs, IN_VIS_THRE)
    assert len(np.unique(score)) == len(score)                  # the reference's argsort leaves ties open: there are none
    out = {'kpts': kpts, 'area': area, 'box_score': bs, 'seg': seg, 'in_vis_thre': np.float64(IN_VIS_THRE),
           'score': score, 'cases': np.array([[s, np.nan if v is None else v, t, md] for s, v, t, md in CASES])}
    margin = np.inf
    for c, (soft, vis, thr, md) in enumerate(CASES):
        keeps, kseg = [], [0]
        for m in range(len(SIZES)):
            r = slice(seg[m], seg[m + 1])
            db = [{'score': score[i], 'keypoints': kpts[i].astype(np.float64), 'area': float(area[i])}
                  for i in range(r.start, r.stop)]
            if soft:
                k = ref.soft_oks_nms(db, thr, max_dets=md, vis_thr=vis)
                mine, mg = nr.soft_oks_nms(kpts[r], score[r], area[r], thr, md, None, vis)
            else:
                k = ref.oks_nms(db, thr, vis_thr=vis)
                mine, mg = nr.oks_nms(kpts[r], score[r], area[r], thr, None, vis)
            k = [int(i) for i in k]
            assert k == mine, (c, m, k, mine)
            margin = min(margin, mg)
            keeps.extend(k)
            kseg.append(len(keeps))
        out['keep_%d' % c] = np.asarray(keeps, dtype=np.int32)
        out['kseg_%d' % c] = np.asarray(kseg, dtype=np.int32)
    print('seed %d: %d detections, smallest decision margin %.3e' % (seed, len(kpts), margin))
    assert margin >= 1e-4
    props = nr.fixture_properties(out)
    print(props)
    assert min(props.values()) >= 1, props
    np.savez_compressed(OUT, **out)
    print('wrote %s (%d bytes)' % (OUT, os.path.getsize(OUT)))


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else SEED)
