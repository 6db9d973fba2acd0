"""Host side of pose rescoring and OKS-NMS (evaluate.pose_nms / pose_nms_options / EvalAccumulator.pose_nms,
csrc/nms.hip): the numpy yardstick tests/_nms_ref.py against the fixture tests/golden/pose_nms.npz, the cfg switches,
and the argument validation that happens before any device work.

The fixture holds what the reference's OWN oks_nms and soft_oks_nms (datasets/process/nms.py:89-192) keep on seeded
detections (tools/gen_nms_golden.py): 12 images of 1 ... 40 detections, hard and soft mode, vis_thr none / 0.2,
thresholds 0.5 and 0.9.  The reference stores its OKS values as float32 (and squares them in float32 in soft mode); the
restatement is float64 throughout, so the keep arrays must agree exactly only where no decision is closer than that
rounding (~1e-7 relative): the restatement's smallest decision margin on the fixture is asserted to be >= 1e-4."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _nms_ref as nr  # noqa: E402

import fami_pose_amd as fp  # noqa: E402
from fami_pose_amd import evaluate as ev  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pose_nms.npz')


def test_restatement_reproduces_the_reference_fixture():
    g = np.load(GOLD)
    seg, kpts, area = g['seg'], g['kpts'], g['area']
    assert kpts.dtype == np.float32 and kpts.shape[1:] == (17, 3) and 100 <= len(kpts) <= 1000
    score = nr.rescore(kpts, g['box_score'], float(g['in_vis_thre']))
    assert np.array_equal(score, g['score'])                      # the scores the reference was fed are the rule's
    cases = nr.fixture_cases(g)
    assert all(c[2] in (None, 0.2) for c in cases)
    assert {(c[1], c[2] is None, c[3]) for c in cases} == {(s, v, t) for s in (False, True) for v in (False, True)
                                                            for t in (0.5, 0.9)}
    margin = np.inf
    for c, soft, vis, thr, md, keeps in cases:
        for m, want in enumerate(keeps):
            r = slice(seg[m], seg[m + 1])
            if soft:
                got, mg = nr.soft_oks_nms(kpts[r], score[r], area[r], thr, md, None, vis)
            else:
                got, mg = nr.oks_nms(kpts[r], score[r], area[r], thr, None, vis)
            assert got == want, (c, m)
            margin = min(margin, mg)
    print('fixture: smallest decision margin %.3e' % margin)
    assert margin >= 1e-4


def test_fixture_cannot_pass_vacuously():
    props = nr.fixture_properties(np.load(GOLD))
    print(props)
    assert props['suppressed'] >= 1              # something is suppressed
    assert props['survivors_behind'] >= 1        # ... and something lower-scored than a suppressed detection survives
    assert props['vis_changes'] >= 1             # vis_thr changes the keep list of an image
    assert props['soft_capped'] >= 1             # soft mode stops at max_dets somewhere


def _two(score_a, score_b):
    """A and B agree on joints 0..7 and lie far apart on joints 8..16; A is confident on 8..16 only, B on 0..7 only."""
    rng = np.random.RandomState(1)
    k = np.zeros((2, 17, 3))
    k[0, :, :2] = rng.uniform(100, 400, (17, 2))
    k[1, :, :2] = k[0, :, :2]
    k[1, 8:, :2] += 500.0
    k[0, :8, 2], k[0, 8:, 2] = 0.1, 0.9
    k[1, :8, 2], k[1, 8:, 2] = 0.9, 0.1
    return k, np.array([score_a, score_b]), np.array([2e4, 2e4])


def test_the_mask_reads_the_compared_detection_only():
    """`list(vg > t) and list(vd > t)` is the second list.  A picked, B compared: B's visible joints (0..7) coincide with
    A's -> OKS 1, B is suppressed; the picked pose's visibility (8..16: far apart) or the intersection (empty) would both
    keep B.  B picked, A compared: A's visible joints are the far ones -> OKS 0, both are kept."""
    k, sc, a = _two(0.9, 0.8)
    assert nr.oks_iou(k[0], k[1:], a[0], a[1:], None, 0.2)[0] == 1.0
    assert nr.oks_nms(k, sc, a, 0.5, None, 0.2)[0] == [0]
    k, sc, a = _two(0.8, 0.9)
    assert nr.oks_iou(k[1], k[:1], a[1], a[:1], None, 0.2)[0] < 1e-12
    assert nr.oks_nms(k, sc, a, 0.5, None, 0.2)[0] == [1, 0]
    # without a vis_thr all 17 joints count either way: 8 coincide, 9 are far -> OKS 8/17 < 0.5
    assert abs(nr.oks_iou(k[0], k[1:], a[0], a[1:])[0] - 8 / 17) < 1e-12
    # an empty mask is OKS 0, not a division by zero
    assert nr.oks_iou(k[0], k[1:], a[0], a[1:], None, 0.95)[0] == 0.0


def test_restatement_rules():
    rng = np.random.RandomState(2)
    k, a, b = nr.make_dets(rng, 6)
    # rescoring: the mean over the joints above the threshold, 0 when none passes, one rounding to fp32
    s = nr.rescore(k, b, 0.2)
    for i in range(6):
        c = k[i, :, 2].astype(np.float64)
        c = c[c > 0.2]
        assert abs(s[i] - float(b[i]) * c.mean()) <= 1e-7 * s[i] and s[i] == np.float32(s[i])
    assert (nr.rescore(k, b, 2.0) == 0).all()
    # equal scores: the one listed first is picked first
    far = k.copy()
    far[:, :, 0] += 3000.0 * np.arange(6)[:, None]
    assert nr.oks_nms(far, np.full(6, 0.5), a, 0.5)[0] == [0, 1, 2, 3, 4, 5]
    assert nr.soft_oks_nms(far, np.array([.5, .7, .5, .7, .1, .5]), a, 0.5, max_dets=4)[0] == [1, 3, 0, 2]
    # identical poses: OKS 1, the second is suppressed (hard) / decayed by exp(-1 / thr) (soft)
    twin = np.stack([k[0], k[0]])
    assert nr.oks_nms(twin, np.array([.6, .7]), a[[0, 0]], 0.9)[0] == [1]
    assert np.allclose(nr.rescore_overlap(np.array([1.0]), np.array([0.6]), 0.5), 0.6 * np.exp(-2.0))
    assert np.allclose(nr.rescore_overlap(np.array([0.6, 0.4]), np.array([0.5, 0.5]), 0.5, 'linear'), [0.2, 0.5])


def test_coco_sigmas_and_exports():
    assert np.array_equal(ev.COCO_SIGMAS, nr.COCO_SIGMAS) and ev.COCO_SIGMAS.shape == (17,)
    assert ev.COCO_SIGMAS[0] == .26 / 10.0 and ev.COCO_SIGMAS[11] == 1.07 / 10.0
    assert fp.pose_nms is ev.pose_nms and fp.pose_nms_options is ev.pose_nms_options and fp.COCO_SIGMAS is ev.COCO_SIGMAS
    for name in ('COCO_SIGMAS', 'pose_nms', 'pose_nms_options'):
        assert name in fp.__all__


def test_pose_nms_options_defaults():
    cfg = fp.default_cfg()
    for node in ('VAL', 'TEST'):
        assert cfg[node]['IN_VIS_THRE'] == 0.0 and cfg[node]['OKS_THRE'] == 0.5 and cfg[node]['SOFT_NMS'] is False
    want = {'in_vis_thre': 0.0, 'oks_thre': 0.5, 'soft': False}
    for phase in (fp.VAL_PHASE, fp.TEST_PHASE):
        assert ev.pose_nms_options(cfg, phase) == want
        assert ev.pose_nms_options(fp.CfgNode(), phase) == want          # absent node
        assert ev.pose_nms_options({'VAL': {}, 'TEST': {}}, phase) == want   # absent keys
    assert ev.flip_test_options(cfg, fp.VAL_PHASE) == {'flip': False, 'shift_heatmap': False}


def test_pose_nms_options_per_phase():
    cfg = fp.default_cfg()
    cfg.VAL.IN_VIS_THRE, cfg.VAL.OKS_THRE, cfg.VAL.SOFT_NMS = 0.2, 0.9, True          # Base_PoseTrack17.yaml's values
    assert ev.pose_nms_options(cfg, fp.VAL_PHASE) == {'in_vis_thre': 0.2, 'oks_thre': 0.9, 'soft': True}
    assert ev.pose_nms_options(cfg, fp.TEST_PHASE) == {'in_vis_thre': 0.0, 'oks_thre': 0.5, 'soft': False}
    cfg.TEST.OKS_THRE = 0.7
    assert ev.pose_nms_options(cfg, fp.TEST_PHASE) == {'in_vis_thre': 0.0, 'oks_thre': 0.7, 'soft': False}
    assert ev.pose_nms_options(cfg, fp.VAL_PHASE)['oks_thre'] == 0.9                   # each phase reads its own node
    with pytest.raises(ValueError):
        ev.pose_nms_options(cfg, fp.TRAIN_PHASE)
    with pytest.raises(ValueError):
        ev.pose_nms_options(cfg, 'anything')


def _valid(n=6, J=17, seed=3):
    k, a, b = nr.make_dets(np.random.RandomState(seed), n, J)
    boxes = np.zeros((n, 6))
    boxes[:, 4], boxes[:, 5] = a, b
    return k.astype(np.float64), boxes, {'a': [0, 2, 4], 'b': [1, 3, 5][:max(0, n - 3)]}


def _nan(x, idx):
    x = x.copy()
    x[idx] = np.nan
    return x


BAD = {
    'J != 17 without sigmas': lambda p, b, f: dict(preds=p[:, :15]),
    'J > 32': lambda p, b, f: dict(preds=np.concatenate([p, p], 1), sigmas=np.ones(34)),
    'sigmas of another length': lambda p, b, f: dict(sigmas=np.ones(15)),
    'a sigma of 0': lambda p, b, f: dict(sigmas=np.where(np.arange(17) == 3, 0.0, ev.COCO_SIGMAS)),
    'NaN keypoint': lambda p, b, f: dict(preds=_nan(p, (1, 2, 0))),
    'inf confidence': lambda p, b, f: dict(preds=np.where(np.arange(3) == 2, np.inf, p)),
    'NaN area': lambda p, b, f: dict(boxes=_nan(b, (0, 4))),
    'NaN box score': lambda p, b, f: dict(boxes=_nan(b, (5, 5))),
    'finite in fp64, inf in fp32': lambda p, b, f: dict(boxes=np.where(np.arange(6) == 4, 1e39, b)),
    'NaN sigma': lambda p, b, f: dict(sigmas=_nan(ev.COCO_SIGMAS, 0)),
    'NaN threshold': lambda p, b, f: dict(oks_thre=float('nan')),
    'inf vis_thre': lambda p, b, f: dict(vis_thre=float('inf')),
    'index == N': lambda p, b, f: dict(filenames_map={'a': [0, 6]}),
    'negative index': lambda p, b, f: dict(filenames_map={'a': [0, -1]}),
    'index used twice in one image': lambda p, b, f: dict(filenames_map={'a': [0, 1, 0]}),
    'index used twice across images': lambda p, b, f: dict(filenames_map={'a': [0, 1], 'b': [2, 1]}),
    'a float index': lambda p, b, f: dict(filenames_map={'a': [0, 1.0]}),
    'max_dets = 0': lambda p, b, f: dict(max_dets=0),
    'max_dets = 0 in soft mode': lambda p, b, f: dict(max_dets=0, soft=True),
    'max_dets = 2.5': lambda p, b, f: dict(max_dets=2.5),
    'soft with oks_thre = 0': lambda p, b, f: dict(soft=True, oks_thre=0.0),
    'preds of another rank': lambda p, b, f: dict(preds=p[0]),
    'boxes of another length': lambda p, b, f: dict(boxes=b[:5]),
}


@pytest.mark.parametrize('what', sorted(BAD))
def test_bad_arguments_raise_before_any_device_work(what):
    from fami_pose_amd._lib import lib
    p, b, f = _valid()
    kw = {'preds': p, 'boxes': b, 'filenames_map': f}
    kw.update(BAD[what](p, b, f))
    n0 = lib().ncalls
    with pytest.raises(ValueError):
        ev.pose_nms(**kw)
    assert lib().ncalls == n0                    # no entry point was called (and without a GPU any device work raises
                                                 # something that is no ValueError)


def test_more_than_256_detections_in_an_image_is_refused():
    from fami_pose_amd._lib import lib
    p, b, _ = _valid(300)
    n0 = lib().ncalls
    with pytest.raises(ValueError, match='256'):
        ev.pose_nms(p, b, {'a': list(range(257)), 'b': list(range(257, 300))})
    acc = ev.EvalAccumulator(300)
    acc.all_preds[:], acc.all_boxes[:], acc.idx = p, b, 300
    acc.add_images(['x'] * 257 + ['y'] * 43)
    with pytest.raises(ValueError, match='256'):
        acc.pose_nms()
    assert lib().ncalls == n0


def test_device_only():
    p, b, f = _valid()
    with pytest.raises(RuntimeError):
        ev.pose_nms(p, b, f, device='cpu')                                # device only, like loss.py


def test_entry_point_refuses_bad_arguments():
    """The argument checks are host code of the library: callable without a GPU.  None of these launches."""
    from fami_pose_amd._lib import lib
    c = lib().cdll
    ok = [4096] * 6 + [8, 17, 2, 0.0, 0.5, 0, 20, 0.0, 0] + [4096] * 3 + [None]          # fake, aligned addresses

    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return c.fami_pose_nms_f32(*a)

    assert c.fami_pose_nms_f32(*([None] * 6 + ok[6:15] + [None] * 4)) == -1
    assert b'fami_pose_nms_f32' in c.fami_last_error()
    for i in (0, 1, 2, 3, 4, 5, 15, 16, 17):
        assert call(**{'a%d' % i: None}) == -1, i                          # each null pointer
        assert call(**{'a%d' % i: 4098}) == -1, i                          # each misaligned pointer
    for N in (0, -1, (2 ** 31 - 1) // 51 + 1):
        assert call(a6=N) == -1, N
    for J in (0, -3, 33):
        assert call(a7=J) == -1, J
    for M in (0, -1, 2 ** 31 - 1):
        assert call(a8=M) == -1, M
    assert call(a9=float('nan')) == -1 and call(a10=float('nan')) == -1
    assert call(a13=float('nan'), a14=1) == -1
    for thr in (0.0, -0.5):
        assert call(a10=thr, a11=1) == -1, thr                             # soft mode divides by oks_thre
    assert call(a11=1, a12=0) == -1                                        # soft mode with max_dets < 1
    assert b'soft' in c.fami_last_error()
