"""Writes tests/golden/dark_final_preds.npz: the reference's OWN dark_get_final_preds
(datasets/process/heatmaps_process.py:84-143) on seeded maps.  Runs only where the reference tree is present
(oracle.ref_harness); nothing of the reference enters the repository, only the arrays it computes.

    python tools/gen_dark_golden.py

cv2 is absent where this runs: the reference gets `tests/_dark_ref.cv2_gaussian_blur` as `cv2.GaussianBlur` (the
documented kernel of cv2.GaussianBlur(., (11, 11), 0): sigma 2.0, normalised fp64 taps, separable, reflect-101 border),
as g12 gives it `cv2.getAffineTransform`.  So the fixture pins `taylor`, the clamp, the log, the rescale and
`transform_preds` against the reference's real code, and everything but those two third-party calls.

Fixture: hm [2,17,64,48] float32 (construction 1 of tests/_dark_ref.make_maps: sigma-3 peaks of amplitude U(0.2, 1)
centred in U(-2, W+2) x U(-2, H+2) plus 1e-2 N(0, 1) noise; hm[0,0] all negative, hm[0,1] all zero), center / scale
[2,2] float32 (one identity-like box, one realistic), preds [2,17,2] float64, maxvals [2,17,1] float32."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(ROOT, 'tests', 'golden', 'dark_final_preds.npz')


def main():
    from oracle import ref_harness
    import _dark_ref as dr
    if not ref_harness.available():
        raise SystemExit('gen_dark_golden needs the reference tree (oracle.ref_harness.available() is False)')
    ref_harness.load()
    sys.modules['cv2'].GaussianBlur = dr.cv2_gaussian_blur
    hp = sys.modules['datasets.process.heatmaps_process']
    B, J, H, W = 2, 17, 64, 48
    hm = dr.make_maps(np.random.RandomState(20), B, J, H, W)
    hm[0, 0] = -np.abs(hm[0, 0])
    hm[0, 1] = 0.0
    center = np.array([[W / 2, H / 2], [512.0, 300.25]], np.float32)
    scale = np.array([[W / 200, H / 200], [2.5, 3.3333]], np.float32)
    with np.errstate(invalid='ignore', divide='ignore'):     # the all-zero map: 0 / 0 in the reference's rescale
        preds, maxvals = hp.dark_get_final_preds(hm.copy(), center, scale)
    assert preds.shape == (B, J, 2) and maxvals.shape == (B, J, 1) and np.isfinite(preds).all()
    np.savez_compressed(OUT, hm=hm, center=center, scale=scale, preds=preds, maxvals=maxvals)
    print('wrote %s (%d bytes)' % (OUT, os.path.getsize(OUT)))


if __name__ == '__main__':
    main()
