"""Writes tests/golden/g16_joint_weights.npz: the reference's OWN generate_heatmaps
(datasets/process/heatmaps_process.py:146-203) with use_different_joints_weight=True and the PoseTrack vector
(datasets/zoo/posetrack/PoseTrack_Alignment.py:41-43) on hand-built 17-joint sets.  Runs only where the reference tree
is present (oracle.ref_harness); nothing of the reference enters the repository, only the arrays it computes.  No test
runs this file.

    python tools/gen_target_golden.py

Sets on the 24x18 map (image 72 x 96, stride 4, sigma 3), each [17, 3] joints with visibility:
    centre     every joint on an integer heatmap position within two pixels of the centre
    borders    joints on, just beyond and far beyond each border; the rounded centres mx = -11, W + 9 and my = -11, H + 9
               put the 19x19 patch wholly outside (weight 0), mx = -10 and W + 8 keep the weight and draw nothing
    vis0       visibility 0 on a 1.5-weighted wrist (joint 9), a 1.2-weighted elbow (7) and a 1.0 joint (0)
    half       x / stride at exactly a half (the rounded centre is the upper pixel), y / stride at a quarter
    random     seeded positions from two strides outside the map to two strides outside
and one seeded set on the 96x72 map (image 288 x 384).
Fixture: names [N]; joints, joints_vis [N,17,3] float32; target [N,17,24,18], weight [N,17,1] float32 (the multiplied
weights); joints_big, joints_vis_big [1,17,3]; target_big [1,17,96,72]; weight_big [1,17,1]; joints_weight [17]
float32; sigma; image_size, heatmap_size, image_size_big, heatmap_size_big (w, h)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, 'tests', 'golden', 'g16_joint_weights.npz')
JOINTS_WEIGHT = (1., 1., 1., 1., 1., 1., 1., 1.2, 1.2, 1.5, 1.5, 1., 1., 1.2, 1.2, 1.5, 1.5)
SIGMA = 3


def _set(xy, vis=None):
    joints = np.zeros((17, 3), np.float32)
    joints[:, :2] = np.asarray(xy, np.float64)
    v = np.ones((17, 3), np.float32)
    v[:, 2] = 0
    if vis is not None:
        v[:, 0] = v[:, 1] = vis
    return joints, v


def main():
    from oracle import ref_harness
    if not ref_harness.available():
        raise SystemExit('gen_target_golden needs the reference tree (oracle.ref_harness.available() is False)')
    ref = ref_harness.load()
    jw = np.array(JOINTS_WEIGHT, np.float32).reshape(17, 1)
    image, hm = np.array([72, 96]), np.array([18, 24])
    image_big, hm_big = np.array([288, 384]), np.array([72, 96])
    W, H = hm
    rng = np.random.RandomState(16)
    s = 4.0
    centre = [((W // 2 + (j % 5) - 2) * s, (H // 2 + (j // 5) - 2) * s) for j in range(17)]
    # heatmap positions (x, y) before the stride; -11.5 rounds (toward zero) to -11, -10.5 to -10
    borders = [(0, 12), (W - 1, 12), (9, 0), (9, H - 1), (-1, 5), (W, 5), (5, -1), (5, H), (-10.5, 12), (-11.5, 12),
               (W + 8, 12), (W + 9, 12), (9, -10.5), (9, -11.5), (9, H + 8), (9, H + 9), (-30, -30)]
    borders = [(x * s, y * s) for x, y in borders]
    vis0 = np.ones(17, np.float32)
    vis0[[0, 7, 9]] = 0
    vis0_xy = np.stack([rng.uniform(2, W - 2, 17), rng.uniform(2, H - 2, 17)], -1) * s
    half = [((2 + (j % 6) * 2 + 0.5) * s, (3 + j + 0.25) * s) for j in range(17)]
    rnd_xy = np.stack([rng.uniform(-2, W + 2, 17), rng.uniform(-2, H + 2, 17)], -1) * s
    rnd_vis = (rng.uniform(size=17) < 0.8).astype(np.float32)
    sets = [('centre', _set(centre)), ('borders', _set(borders)), ('vis0', _set(vis0_xy, vis0)), ('half', _set(half)),
            ('random', _set(rnd_xy, rnd_vis))]
    N = len(sets)
    out = {'names': np.array([n for n, _ in sets]), 'joints': np.zeros((N, 17, 3), np.float32),
           'joints_vis': np.zeros((N, 17, 3), np.float32), 'target': np.zeros((N, 17, H, W), np.float32),
           'weight': np.zeros((N, 17, 1), np.float32), 'joints_weight': jw.reshape(17), 'sigma': np.int64(SIGMA),
           'image_size': image, 'heatmap_size': hm, 'image_size_big': image_big, 'heatmap_size_big': hm_big}
    for k, (name, (joints, vis)) in enumerate(sets):
        t, w = ref.generate_heatmaps(joints.copy(), vis.copy(), SIGMA, image, hm, 17, use_different_joints_weight=True,
                                     joints_weight=jw)
        assert t.dtype == np.float32 and t.shape == (17, H, W) and w.dtype == np.float32 and w.shape == (17, 1)
        out['joints'][k], out['joints_vis'][k], out['target'][k], out['weight'][k] = joints, vis, t, w
    w = out['weight'][..., 0]
    names = list(out['names'])
    assert np.array_equal(w[names.index('centre')], jw.reshape(17))
    wb = w[names.index('borders')]
    assert [j for j in range(17) if wb[j] == 0] == [9, 11, 13, 15, 16], wb      # wholly outside: weight 0
    tb = out['target'][names.index('borders')].reshape(17, -1).max(1)
    assert tb[8] == 0 and tb[10] > 0 and wb[8] == jw[8, 0] and wb[10] == jw[10, 0], (tb, wb)
    wv = w[names.index('vis0')]
    assert wv[0] == 0 and wv[7] == 0 and wv[9] == 0 and wv[10] == np.float32(1.5) and wv[8] == np.float32(1.2)
    assert sorted(set(w.reshape(-1).tolist())) == sorted({0.0, 1.0, float(np.float32(1.2)), 1.5})
    big_xy = np.stack([rng.uniform(-8, 72 + 8, 17), rng.uniform(-8, 96 + 8, 17)], -1) * s
    joints, vis = _set(big_xy, (rng.uniform(size=17) < 0.85).astype(np.float32))
    t, w = ref.generate_heatmaps(joints.copy(), vis.copy(), SIGMA, image_big, hm_big, 17, use_different_joints_weight=True,
                                 joints_weight=jw)
    assert t.shape == (17, 96, 72) and w.shape == (17, 1) and t.dtype == np.float32 and w.dtype == np.float32
    out.update(joints_big=joints[None], joints_vis_big=vis[None], target_big=t[None], weight_big=w[None])
    np.savez_compressed(OUT, **out)
    print('wrote %s (%d bytes)' % (OUT, os.path.getsize(OUT)))


if __name__ == '__main__':
    main()
