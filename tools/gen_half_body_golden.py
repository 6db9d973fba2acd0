"""Writes tests/golden/g15_half_body.npz: the reference's OWN half_body_transform and fliplr_joints
(datasets/process/pose_process.py:45-81, :12-26) on hand-built joint sets under recorded numpy seeds.  Runs only where
the reference tree is present (oracle.ref_harness); nothing of the reference enters the repository, only the arrays it
computes.  No test runs this file.

    python tools/gen_half_body_golden.py

half_body_transform draws ONE numpy.random.randn() and takes the upper half where it is < 0.5; per case the seed is the
first one from 0 whose first randn() falls on the wanted side, and it is recorded.  Cases (aspect_ratio 288 / 384,
pixel_std 200, upper_body_ids 0..10):
    upper_wide       draw < 0.5, upper joints taken, w > aspect * h
    upper_tall       draw < 0.5, upper joints taken, w < aspect * h
    lower            draw >= 0.5, more than two lower joints: lower joints taken
    lower_fallback   draw >= 0.5, two lower joints: falls back to the upper joints
    upper_too_few    draw < 0.5, two upper joints: lower joints taken
    none             one visible joint in all: (None, None)
Fixture: names [N]; seed [N]; joints, joints_vis [N,17,3] float32; aspect_ratio, pixel_std; upper_body_ids;
is_none [N]; center, scale [N,2] float32 (zeros where is_none); and, for fliplr_joints on case `lower` at width 640 with
the PoseTrack flip pairs: flip_width, flip_pairs, flip_joints, flip_vis."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, 'tests', 'golden', 'g15_half_body.npz')
UPPER = tuple(range(11))
PAIRS = ((3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16))


def _seed(upper):
    """first seed whose first randn() is < 0.5 (upper) / >= 0.5"""
    for s in range(1000):
        if (np.random.RandomState(s).randn() < 0.5) == upper:
            return s
    raise AssertionError


def _case(rng, visible, box):
    """17 joints uniform in box = (x0, y0, x1, y1); the ids in `visible` are visible"""
    joints = np.zeros((17, 3), np.float32)
    joints[:, 0] = rng.uniform(box[0], box[2], 17)
    joints[:, 1] = rng.uniform(box[1], box[3], 17)
    vis = np.zeros((17, 3), np.float32)
    vis[list(visible), :2] = 1
    return joints, vis


def main():
    from oracle import ref_harness
    if not ref_harness.available():
        raise SystemExit('gen_half_body_golden needs the reference tree (oracle.ref_harness.available() is False)')
    ref_harness.load()
    pp = importlib.import_module('datasets.process.pose_process')
    rng = np.random.RandomState(15)
    aspect, pixel_std = 288 * 1.0 / 384, 200
    cases = [
        ('upper_wide', True, _case(rng, range(17), (100, 200, 500, 260))),
        ('upper_tall', True, _case(rng, range(17), (300, 20, 340, 460))),
        ('lower', False, _case(rng, (0, 2, 5, 6, 11, 12, 13, 14, 16), (50, 60, 400, 420))),
        ('lower_fallback', False, _case(rng, (1, 3, 5, 7, 9, 13, 16), (10, 10, 630, 470))),
        ('upper_too_few', True, _case(rng, (4, 10, 11, 12, 15, 16), (200, 100, 320, 400))),
        ('none', True, _case(rng, (6,), (0, 0, 640, 480))),
    ]
    N = len(cases)
    out = {'names': np.array([c[0] for c in cases]), 'seed': np.zeros(N, np.int64),
           'joints': np.zeros((N, 17, 3), np.float32), 'joints_vis': np.zeros((N, 17, 3), np.float32),
           'aspect_ratio': np.float64(aspect), 'pixel_std': np.int64(pixel_std), 'upper_body_ids': np.array(UPPER),
           'is_none': np.zeros(N, bool), 'center': np.zeros((N, 2), np.float32), 'scale': np.zeros((N, 2), np.float32)}
    for k, (name, upper, (joints, vis)) in enumerate(cases):
        seed = _seed(upper)
        np.random.seed(seed)
        c, s = pp.half_body_transform(joints.copy(), vis.copy(), 17, UPPER, aspect, pixel_std)
        out['seed'][k], out['joints'][k], out['joints_vis'][k] = seed, joints, vis
        if c is None:
            assert s is None
            out['is_none'][k] = True
        else:
            assert c.dtype == np.float32 and s.dtype == np.float32 and c.shape == (2,) and s.shape == (2,)
            out['center'][k], out['scale'][k] = c, s
    assert list(out['is_none']) == [False] * 5 + [True]
    w_h = out['scale'][:2] * pixel_std / 1.5                      # the two aspect branches were both taken
    j0, j1 = out['joints'][0, :11], out['joints'][1, :11]
    assert np.ptp(j0[:, 0]) > aspect * np.ptp(j0[:, 1]) and np.ptp(j1[:, 0]) < aspect * np.ptp(j1[:, 1]), w_h
    fj, fv = pp.fliplr_joints(out['joints'][2].copy(), out['joints_vis'][2].copy(), 640, PAIRS)
    out.update(flip_width=np.int64(640), flip_pairs=np.array(PAIRS), flip_joints=fj, flip_vis=fv)
    np.savez_compressed(OUT, **out)
    print('wrote %s (%d bytes)' % (OUT, os.path.getsize(OUT)))


if __name__ == '__main__':
    main()
