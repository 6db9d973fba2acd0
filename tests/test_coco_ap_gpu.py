"""COCO keypoint AP / AR on the MI355X (csrc/coco_ap.hip: fami_coco_kpt_match_f64, fami_coco_kpt_curve_f64;
evaluate.coco_keypoint_ap / evaluate_coco_keypoints) against the float64 restatement tests/_coco_ref.py, which
tests/test_coco_ap_host.py holds to hand-derived numbers.

Bounds.  The kept rows, their order, the matched / ignored byte of every kept detection for all 30 (range, threshold) pairs
and the per-(image, range) counts must be EQUAL: the kernel and the restatement evaluate the same fp64 expressions, and
what can differ (the last bit of an exp) is ~1e-16, so equality is demanded of inputs on which nothing is decided that
closely: every set is asserted on the CPU, before anything is launched, to keep every OKS >= 1e-9 away from every threshold
and any two competing OKS values of a detection >= 1e-9 apart unless bit-identical by construction.
precision and recall must be equal BIT FOR BIT, from the curve kernel alone and end to end: every value is int -> double,
one add, one add of 2^-52 and one divide, or a maximum of such values; there is no sum whose order could differ.  stats are
numpy means over those arrays on both sides: equal too.  Two runs must agree bit for bit, the guard words around every
output must be intact, and the input arrays unchanged.

Shapes (the smallest at which the kernels can go wrong): the hand-made images of the host test (crowd, twins, the stop rule,
out-of-range areas, areas on a bound, an annotation without a labelled joint, nothing that counts), one per image in one
launch, at max_dets 20 and 21; 200 seeded images, among them images with no detection, with no annotation and with neither,
at max_dets 20 and 1; an image exactly at the caps (256 detections, 128 annotations, max_dets 64) between two small ones,
also with 32 joints (the largest LDS footprint a launch can have);
an image over each cap, and one whose segment leaves its array, between intact neighbours; equal scores straddling the cut.
Curve lengths 1, 63 / 64 / 65 (the ballot word), 16385 (one past a 64-bit word per thread), 70001 and the cap 229376."""
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _coco_ref as cr  # noqa: E402

from fami_pose_amd import evaluate as ev  # noqa: E402
from fami_pose_amd._lib import FamiError, lib  # noqa: E402

pytestmark = pytest.mark.gpu

MARGIN = 1e-9
GUARD = 256
SENT = 0x5a5a5a5a
T, R, A = 10, 101, 3
VAR = (cr.SIG * 2) ** 2


# ---------------------------------------------------------------------------------------- inputs
def _hand_set():
    """Every hand-made case of the host test as one image of one set (image id = its position)."""
    gt, dt = [], []
    for i, (name, (g, d, _)) in enumerate(cr.cases().items()):
        gt += [dict(copy.deepcopy(a), image_id=i) for a in g]
        dt += [dict(copy.deepcopy(a), image_id=i) for a in d]
    return gt, dt, list(range(len(cr.cases())))


_SETS = {'hand': _hand_set, 'seeded': cr.seeded_set, 'caps': cr.caps_set, 'ties': cr.ties_set}
_FAMILIES = {}


def _family(name, max_det, sigmas=cr.SIG, joints=17):
    """-> (gt, dt, ids, restatement, packed); the margins are asserted here, before any launch."""
    key = (name, max_det, joints)
    if key not in _FAMILIES:
        gt, dt, ids = _SETS[name]()
        if joints != 17:                                             # fewer joints: the first ones; more: the list repeated
            gt = [dict(a, keypoints=(a['keypoints'] * 2)[:3 * joints]) for a in gt]
            dt = [dict(a, keypoints=(a['keypoints'] * 2)[:3 * joints]) for a in dt]
        ref = cr.evaluate(gt, dt, max_det=max_det, sigmas=sigmas, img_ids=ids)
        print('%s @ %d: %d images, %d annotations, %d detections, margin %.3e, tie margin %.3e'
              % (name, max_det, len(ids), len(gt), len(dt), ref['margin'], ref['tie_margin']))
        assert ref['margin'] >= MARGIN and ref['tie_margin'] >= MARGIN
        _FAMILIES[key] = (gt, dt, ids, ref, ev.pack_coco_keypoints(gt, dt, img_ids=ids))
    return _FAMILIES[key]


# ---------------------------------------------------------------------------------------- raw launches, guarded outputs
def _guarded(dev, words):
    return torch.full((GUARD + words + GUARD,), SENT, dtype=torch.int32, device=dev)


def _unguard(t, words):
    a = t.cpu().numpy()
    return a[GUARD:GUARD + words].copy(), bool((a[:GUARD] == SENT).all() and (a[GUARD + words:] == SENT).all())


def _raw_match(dev, k, max_det, var=VAR, iou=cr.IOU, rng=cr.ARNG):
    """The entry point itself on packed arrays -> (score [M,K], row [M,K], flags [M,K,A*T], npig [M,A]), guards intact,
    inputs unchanged?"""
    G, D, M, J = len(k['gt_flags']), len(k['dt_score']), len(k['gt_seg']) - 1, k['num_joints']
    K, AT = max_det, len(rng) * len(iou)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt).reshape(-1)).to(dev)  # noqa: E731
    names = ('gt_kpts', 'gt_area', 'gt_bbox', 'gt_flags', 'dt_kpts', 'dt_score', 'dt_area', 'gt_seg', 'dt_seg')
    keep = [up(k[n], np.int32 if n in ('gt_flags', 'gt_seg', 'dt_seg') else np.float64) for n in names]
    before = [t.clone() for t in keep]
    sizes = (2 * M * K, M * K, (M * K * AT + 3) // 4, M * A)
    outs = [_guarded(dev, n) for n in sizes]
    var, iou, rng = (np.ascontiguousarray(a, dtype=np.float64) for a in (var, iou, rng))
    lib().call('fami_coco_kpt_match_f64', *[t.data_ptr() for t in keep], var.ctypes.data, iou.ctypes.data, rng.ctypes.data,
               G, D, M, J, len(iou), len(rng), K, *[t[GUARD:].data_ptr() for t in outs], torch.cuda.current_stream(dev).cuda_stream)
    res = [_unguard(t, n) for t, n in zip(outs, sizes)]
    same = all(torch.equal(a, b) for a, b in zip(keep, before))
    flags = res[2][0].view(np.uint8)[:M * K * AT].reshape(M, K, AT)
    return (res[0][0].view(np.float64).reshape(M, K), res[1][0].reshape(M, K), flags, res[3][0].reshape(M, A)), \
        all(r[1] for r in res) and same


def _raw_curve(dev, flags, npig_img, rec=cr.REC, t=T, a=A):
    """flags [A*T,N] uint8, npig_img [M,A] -> (precision [T,R,A], recall [T,A]), guards intact?"""
    N, M, nr = flags.shape[1], len(npig_img), len(rec)
    d_fl = torch.from_numpy(np.ascontiguousarray(flags, dtype=np.uint8)).to(dev)
    d_n = torch.from_numpy(np.ascontiguousarray(npig_img, dtype=np.int32)).to(dev)
    rec = np.ascontiguousarray(rec, dtype=np.float64)
    pr, rc = _guarded(dev, 2 * t * nr * a), _guarded(dev, 2 * t * a)       # GUARD words = 1 KiB: the doubles stay aligned
    lib().call('fami_coco_kpt_curve_f64', d_fl.data_ptr() if N else None, d_n.data_ptr(), rec.ctypes.data, N, M, t, a, nr,
               pr[GUARD:].data_ptr(), rc[GUARD:].data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    (p, ok1), (r, ok2) = _unguard(pr, 2 * t * nr * a), _unguard(rc, 2 * t * a)
    return p.view(np.float64).reshape(t, nr, a), r.view(np.float64).reshape(t, a), ok1 and ok2


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _check_images(got, ref, packed, ids, K, only=None):
    """The match launch's outputs against the restatement, image by image (`only`: positions in ids to look at)."""
    score, row, flags, npig = got
    by_id = dict(zip(ref['image_ids'], ref['images']))
    for m, i in enumerate(ids):
        if only is not None and m not in only:
            continue
        r = by_id.get(i)
        n = len(r['kept']) if r else 0
        assert (row[m, n:] == -1).all() and (score[m, n:] == 0).all() and not flags[m, n:].any(), i
        assert npig[m].tolist() == (r['npig'].tolist() if r else [0] * A), i
        if n:
            assert packed['dt_index'][row[m, :n]].tolist() == r['rows'], i
            assert np.array_equal(_bits(score[m, :n]), _bits(r['scores'])), i
            assert np.array_equal(flags[m, :n], r['flags']), (i, np.argwhere(flags[m, :n] != r['flags'])[:4].tolist())


# ---------------------------------------------------------------------------------------- 1. the match kernel
@pytest.mark.parametrize('name,max_det', [('hand', 20), ('hand', 21), ('seeded', 20), ('seeded', 1), ('caps', 64), ('ties', 18),
                                          ('ties', 22)])
def test_match_against_the_restatement(dev, name, max_det):
    gt, dt, ids, ref, packed = _family(name, max_det)
    runs = [_raw_match(dev, packed, max_det) for _ in range(2)]
    got, intact = runs[0]
    assert intact
    _check_images(got, ref, packed, ids, max_det)
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, runs[1][0]))
    if name == 'seeded':
        n_gt, n_dt = np.diff(packed['gt_seg']), np.diff(packed['dt_seg'])
        assert ((n_gt == 0) & (n_dt == 0)).any() and ((n_gt > 0) & (n_dt == 0)).any() and ((n_gt == 0) & (n_dt > 0)).any()
        assert (got[2] == 3).any() and (got[2] == 2).any() and (got[2] == 1).any()
    if name == 'caps':
        assert np.diff(packed['gt_seg']).tolist() == [2, 128, 3] and np.diff(packed['dt_seg']).tolist() == [4, 256, 6]
        assert (got[1][1] >= 0).all() and (got[1][0, 4:] == -1).all()
    if name == 'ties':
        kept = got[1][0].tolist()
        sc = packed['dt_score']
        assert set(sc[kept]) & set(sc[[i for i in range(24) if i not in kept]])     # an equal score on either side of the cut


def test_images_over_a_cap_are_marked_and_their_neighbours_intact(dev):
    """Through the raw entry point (the Python layer refuses these): the middle image of the caps set is given a 257th
    detection, then a 129th annotation -- taken from the image behind it -- and then the last image a segment that leaves
    the array.  The marked image gets npig = -1 and nothing else written; the others come out as the restatement has them."""
    gt, dt, ids, _, packed = _family('caps', 64)
    sent64 = np.array([SENT, SENT], np.int32).view(np.float64)[0]
    for key, anns, pos in (('dt_seg', dt, 260), ('gt_seg', gt, 130)):
        k = {n: (v.copy() if isinstance(v, np.ndarray) else v) for n, v in packed.items()}
        k[key][2] += 1
        moved = copy.deepcopy(anns)
        moved[pos]['image_id'] = 1                                   # the restatement's view of the same move
        ref = cr.evaluate(gt if key == 'dt_seg' else moved, moved if key == 'dt_seg' else dt, max_det=64, img_ids=ids)
        assert ref['margin'] >= MARGIN and ref['tie_margin'] >= MARGIN
        got, intact = _raw_match(dev, k, 64)
        assert intact and (got[3][1] == -1).all()
        assert (got[1][1] == SENT).all() and (_bits(got[0][1]) == _bits(sent64)).all() and (got[2][1] == 0x5a).all()
        _check_images(got, ref, packed, ids, 64, only=(0, 2))
        with pytest.raises(ValueError, match='the limits are'):
            ev.coco_keypoint_ap(k, max_dets=64, device=dev)
    k = {n: (v.copy() if isinstance(v, np.ndarray) else v) for n, v in packed.items()}
    k['dt_seg'][3] += 7
    got, intact = _raw_match(dev, k, 64)
    assert intact and (got[3][2] == -1).all() and (got[1][2] == SENT).all()
    _check_images(got, _family('caps', 64)[3], packed, ids, 64, only=(0, 1))
    with pytest.raises(ValueError, match='must ascend'):
        ev.coco_keypoint_ap(k, max_dets=64, device=dev)


def test_entry_points_refuse_before_any_launch(dev):
    gt, dt, ids, _, packed = _family('ties', 18)
    nan = np.array(cr.IOU)
    nan[3] = np.nan
    for kw in ({'var': np.r_[VAR[:16], np.nan]}, {'iou': nan}, {'rng': [[0, np.nan]]}, {'iou': np.linspace(.5, .95, 33)},
               {'rng': np.zeros((9, 2))}):
        with pytest.raises(FamiError, match='fami_coco_kpt_match_f64'):
            _raw_match(dev, packed, 18, **kw)
    for max_det in (0, 65):
        with pytest.raises(FamiError, match='max_dets'):
            _raw_match(dev, packed, max_det)
    with pytest.raises(FamiError, match='J must be'):
        _raw_match(dev, dict(packed, num_joints=33), 18)
    npig = np.ones((2, A), np.int32)
    for kw in ({'rec': np.r_[cr.REC[:5], np.nan]}, {'rec': np.linspace(0, 1, 257)}, {'t': 33}):
        with pytest.raises(FamiError, match='fami_coco_kpt_curve_f64'):
            _raw_curve(dev, np.zeros((kw.get('t', T) * A, 8), np.uint8), npig, **kw)
    s = torch.cuda.current_stream(dev).cuda_stream
    buf = torch.zeros(4096, dtype=torch.float64, device=dev)
    rec = np.ascontiguousarray(cr.REC)
    for args in ((buf.data_ptr(), buf.data_ptr(), rec.ctypes.data, ev.COCO_MAX_SET + 1, 2, T, A, R, buf.data_ptr(), buf.data_ptr(), s),
                 (buf.data_ptr(), buf.data_ptr(), rec.ctypes.data, -1, 2, T, A, R, buf.data_ptr(), buf.data_ptr(), s),
                 (buf.data_ptr(), buf.data_ptr(), rec.ctypes.data, 8, 0, T, A, R, buf.data_ptr(), buf.data_ptr(), s),
                 (None, buf.data_ptr(), rec.ctypes.data, 8, 2, T, A, R, buf.data_ptr(), buf.data_ptr(), s),
                 (buf.data_ptr(), buf.data_ptr(), rec.ctypes.data, 8, 2, T, A, R, buf.data_ptr() + 4, buf.data_ptr(), s),
                 (buf.data_ptr(), buf.data_ptr() + 2, rec.ctypes.data, 8, 2, T, A, R, buf.data_ptr(), buf.data_ptr(), s)):
        with pytest.raises(FamiError, match='fami_coco_kpt_curve_f64'):
            lib().call('fami_coco_kpt_curve_f64', *args)
    assert not buf.any()


# ---------------------------------------------------------------------------------------- 2. the curve kernel alone
@pytest.mark.parametrize('N', [1, 63, 64, 65, 16385, 70001, ev.COCO_MAX_SET])
def test_curve_lengths(dev, N):
    """Seeded random bytes for the 30 (range, threshold) rows; range 2 has no counting annotation (-1 everywhere); the
    counts of the other two are spread over three images.  precision and recall bit for bit."""
    rng = np.random.RandomState(N % 9973)
    flags = rng.choice(np.array([0, 1, 2, 3], np.uint8), size=(A * T, N), p=[0.35, 0.45, 0.1, 0.1])
    flags[T + 3] = 0                                                   # a row without a true positive
    flags[T + 4] = 1                                                   # ... and one of nothing else
    tp = (flags == 1).sum(1).reshape(A, T).max(1)
    npig = np.array([tp[0] + 7, tp[1], 0])
    npig_img = np.stack([npig // 3, npig // 3, npig - 2 * (npig // 3)]).astype(np.int32)
    want_p, want_r = -np.ones((T, R, A)), -np.ones((T, A))
    for a in range(A):
        for t in range(T):
            want_p[t, :, a], want_r[t, a] = cr.curve(flags[a * T + t], int(npig[a]))
    runs = [_raw_curve(dev, flags, npig_img) for _ in range(2)]
    p, r, intact = runs[0]
    assert intact
    print('N = %d: precision differs in %d, recall in %d entries' % (N, (_bits(p) != _bits(want_p)).sum(), (_bits(r) != _bits(want_r)).sum()))
    assert np.array_equal(_bits(r), _bits(want_r)) and np.array_equal(_bits(p), _bits(want_p))
    assert (p[:, :, 2] == -1).all() and (p[3, 1:, 1] == 0).all() and want_r[4, 1] == 1.0 and (p[:, :, :2] >= 0).all()
    assert np.array_equal(_bits(p), _bits(runs[1][0])) and np.array_equal(_bits(r), _bits(runs[1][1]))


def test_curve_without_detections_and_other_thresholds(dev):
    p, r, intact = _raw_curve(dev, np.zeros((A * T, 0), np.uint8), np.array([[2, 0, 1]], np.int32))
    assert intact and (p[:, :, [0, 2]] == 0).all() and (r[:, [0, 2]] == 0).all() and (p[:, :, 1] == -1).all() and (r[:, 1] == -1).all()
    rng = np.random.RandomState(8)
    flags = rng.choice(np.array([0, 1, 2, 3], np.uint8), size=(2 * 3, 1000))
    rec = np.array([1.0, 0.0, 0.25, 0.25, 0.9999, 2.0, -1.0])          # unsorted, repeated, out of range: searchsorted takes any
    p, r, intact = _raw_curve(dev, flags, np.array([[300, 260]], np.int32), rec=rec, t=3, a=2)
    assert intact
    for a in range(2):
        for t in range(3):
            wp, wr = cr.curve(flags[a * 3 + t], (300, 260)[a], rec)
            assert np.array_equal(_bits(p[t, :, a]), _bits(wp)) and _bits(r[t, a]) == _bits(wr)


# ---------------------------------------------------------------------------------------- 3. end to end
def _same_result(res, ref):
    assert res['precision'].dtype == np.float64 and res['names'] == cr.NAMES
    assert np.array_equal(_bits(res['precision']), _bits(ref['precision'])) and np.array_equal(_bits(res['recall']), _bits(ref['recall']))
    assert np.array_equal(_bits(res['stats']), _bits(ref['stats']))


def test_end_to_end(dev, tmp_path):
    gt, dt, ids, ref, packed = _family('seeded', 20)
    guard = {n: v.copy() for n, v in packed.items() if isinstance(v, np.ndarray)}
    runs = [ev.coco_keypoint_ap(packed, device=dev) for _ in range(2)]
    print('stats', ' '.join('%.4f' % v for v in runs[0]['stats']))
    _same_result(runs[0], ref)
    _same_result(runs[1], runs[0])
    assert runs[0]['num_kept'] == ref['sorted_flags'].shape[1] and (ref['stats'] > -1).all()
    assert all(np.array_equal(packed[n], v) and packed[n].dtype == v.dtype for n, v in guard.items())
    # the raw curve launch on the restatement's own sorted bytes: the same numbers
    npig_img = np.array([r['npig'] for r in ref['images']], np.int32)
    p, r, intact = _raw_curve(dev, ref['sorted_flags'], npig_img)
    assert intact and np.array_equal(_bits(p), _bits(ref['precision'])) and np.array_equal(_bits(r), _bits(ref['recall']))
    # from two files
    (tmp_path / 'gt.json').write_text(json.dumps({'images': [{'id': i} for i in ids], 'annotations': gt}))
    (tmp_path / 'dt.json').write_text(json.dumps(dt))
    stats = ev.evaluate_coco_keypoints(str(tmp_path / 'gt.json'), str(tmp_path / 'dt.json'), device=dev)
    assert np.array_equal(_bits(stats), _bits(ref['stats']))
    # the hand-made images and the image at the caps, through the front door
    for name, max_det in (('hand', 20), ('caps', 64), ('ties', 18), ('seeded', 1)):
        _, _, _, ref2, packed2 = _family(name, max_det)
        _same_result(ev.coco_keypoint_ap(packed2, max_dets=max_det, device=dev), ref2)


def test_other_joints_and_thresholds(dev):
    sig = cr.SIG[:15] * 1.1
    gt, dt, ids, ref, packed = _family('seeded', 20, sigmas=sig, joints=15)
    assert packed['num_joints'] == 15
    with pytest.raises(ValueError, match='pass sigmas'):
        ev.coco_keypoint_ap(packed, device=dev)
    _same_result(ev.coco_keypoint_ap(packed, sigmas=sig, device=dev), ref)
    # the largest launch there is: 32 joints, max_dets 64, the image at the caps (136 KiB of LDS)
    sig = np.r_[cr.SIG, cr.SIG][:32]
    gt, dt, ids, ref, packed = _family('caps', 64, sigmas=sig, joints=32)
    assert packed['num_joints'] == 32 and packed['dt_kpts'].shape == (266, 32, 3)
    _same_result(ev.coco_keypoint_ap(packed, max_dets=64, sigmas=sig, device=dev), ref)
    got, intact = _raw_match(dev, packed, 64, var=(sig * 2) ** 2)
    assert intact
    _check_images(got, ref, packed, ids, 64)
    gt, dt, ids, _, packed = _family('seeded', 20)
    iou, rec, arng = np.array([0.3, 0.75, 1.0]), np.linspace(0, 1, 11), np.array([[0, 1e10], [50 ** 2, 150 ** 2]])
    ref = cr.evaluate(gt, dt, max_det=5, iou=iou, rec=rec, arng=arng, img_ids=ids)
    assert ref['margin'] >= MARGIN and ref['tie_margin'] >= MARGIN
    res = ev.coco_keypoint_ap(packed, max_dets=5, iou_thrs=iou, rec_thrs=rec, area_rngs=arng, device=dev)
    _same_result(res, ref)
    assert res['precision'].shape == (3, 11, 2) and res['stats'][1] == -1 and res['stats'][2] > -1 and res['stats'][4] == -1


def test_pose_nms_to_coco_ap_without_a_file(dev):
    """pose_nms -> EvalAccumulator.coco_results -> pack_coco_keypoints -> coco_keypoint_ap, against the same dicts made by
    hand and against the restatement on them."""
    gt, dt, ids, _, _ = _family('seeded', 20)
    acc = ev.EvalAccumulator(len(dt) + 3)
    preds = np.array([d['keypoints'] for d in dt]).reshape(-1, 17, 3)
    rng = np.random.RandomState(1)
    preds[:, :, 2] = rng.uniform(0.2, 1.0, preds.shape[:2])
    n = len(dt)
    acc.all_preds[:n], acc.idx = preds, n
    acc.all_boxes[:n, 4] = [(k[:, 0].max() - k[:, 0].min()) * (k[:, 1].max() - k[:, 1].min()) for k in preds]
    acc.all_boxes[:n, 5] = [d['score'] for d in dt]
    image_ids = [d['image_id'] for d in dt]
    for i, im in enumerate(image_ids):
        acc.filenames_map.setdefault('img/%06d.jpg' % im, []).append(i)
    boxes2, keep = acc.pose_nms(oks_thre=0.5, device=dev)
    rows = [i for v in keep.values() for i in v]
    assert 0 < len(rows) < n
    res = acc.coco_results(image_ids, keep=keep, boxes=boxes2)
    hand = [{'image_id': image_ids[i], 'category_id': 1, 'keypoints': preds[i].reshape(-1).tolist(), 'score': float(boxes2[i, 5])}
            for i in rows]
    assert res == hand
    ref = cr.evaluate(gt, hand, img_ids=ids)
    assert ref['margin'] >= MARGIN and ref['tie_margin'] >= MARGIN
    _same_result(ev.coco_keypoint_ap(ev.pack_coco_keypoints(gt, res, img_ids=ids), device=dev), ref)
