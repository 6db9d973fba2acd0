"""COCO keypoint AP / AR without a GPU: the float64 restatement (tests/_coco_ref.py) against numbers derived by hand from
the definition in include/fami.h, and the host layer of evaluate.py (pack_coco_keypoints, the threshold arrays, the result
dicts, the exports, the prototypes).  tests/test_coco_ap_gpu.py holds the kernels to the restatement.

How the hand numbers come about.  With npig annotations that count and the detections in score order, pr_k = tp_k /
(fp_k + tp_k + 2^-52), so a precision of "1" is 1 / (1 + 2^-52): hence 1e-12 where a quotient is expected, and equality
where the value is a count, a flag or -1.  One true positive in front, recall 0.5: the 51 recall thresholds 0, .01 .. .5
read pr_0 and the other 50 read 0, AP = 51 / 101.

Every set is first asserted to decide nothing within 1e-9 (`margin`: every OKS against every threshold; `tie_margin`: two
OKS values that compete in one walk, unless bit-identical by construction), because the device's exp may differ from
numpy's by an ulp and the GPU tests demand equal decisions on these very sets."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _coco_ref as cr  # noqa: E402

import fami_pose_amd  # noqa: E402
from fami_pose_amd import evaluate as ev  # noqa: E402
from fami_pose_amd._lib import parse_header  # noqa: E402

MARGIN = 1e-9
TOL = 1e-12
T, A = 10, 3
ALL, MED, LARGE = 0, 1, 2

_CASES = {}


def _case(name):
    if name not in _CASES:
        gt, dt, max_det = cr.cases()[name]
        ref = cr.evaluate(gt, dt, max_det=max_det)
        print('%s: margin %.3e, tie margin %.3e' % (name, ref['margin'], ref['tie_margin']))
        assert ref['margin'] >= MARGIN and ref['tie_margin'] >= MARGIN
        _CASES[name] = (gt, dt, ref)
    return _CASES[name]


def _flags(ref, k, a, image=0):
    """The bytes of kept slot k of an image over the ten thresholds of range a."""
    return ref['images'][image]['flags'][k, a * T:(a + 1) * T].tolist()


# ---------------------------------------------------------------------------------------- the restatement, by hand
def test_one_of_two_and_perfect():
    s = _case('one_of_two')[2]['stats']
    assert np.allclose(s[[0, 1, 2, 3]], 51 / 101, rtol=0, atol=TOL) and s[4] == -1 and s[9] == -1
    assert (s[[5, 6, 7, 8]] == 0.5).all()
    ref = _case('perfect')[2]
    s = ref['stats']
    assert np.allclose(s[[0, 1, 2, 3]], 1.0, rtol=0, atol=TOL) and (s[[5, 6, 7, 8]] == 1.0).all() and s[4] == -1 and s[9] == -1
    # pr_1 = 2 / (2 + 2^-52) is exactly 1 (the sum rounds to 2) and the suffix maximum carries it to the front
    assert (ref['precision'][:, :, LARGE] == -1).all() and (ref['precision'][:, :, ALL] == 1.0).all()
    one = _case('one_of_two')[2]['precision'][:, :, ALL]
    assert (one[:, :51] == 1 / (1 + 2.0 ** -52)).all() and (one[:, 51:] == 0).all()


def test_the_21st_detection_is_cut():
    gt, dt, ref = _case('cut')
    img = ref['images'][0]
    assert len(img['kept']) == 20 and img['rows'][0] == 20 and 0 not in img['rows']       # the detection of g2 (list position 0) is cut
    assert (ref['recall'][:, ALL] == 0.5).all() and abs(ref['stats'][0] - 51 / 101) <= TOL
    ref = _case('cut_21')[2]
    assert ref['images'][0]['rows'][-1] == 0 and (ref['recall'][:, ALL] == 1.0).all()
    assert abs(ref['stats'][0] - (51 + 50 * 2 / 21) / 101) <= TOL                          # the second true positive is 21st: 2 / 21


def test_a_crowd_annotation_takes_two_detections():
    ref = _case('crowd')[2]
    for a in range(A):                                                # crowd: ignored in every range, and never used up
        assert _flags(ref, 0, a) == [3] * T and _flags(ref, 1, a) == [3] * T
    assert _flags(ref, 2, ALL) == [1] * T
    assert abs(ref['stats'][0] - 1.0) <= TOL and ref['stats'][5] == 1.0    # neither is a false positive in front of the match


def test_of_two_identical_annotations_the_later_is_taken():
    ref = _case('twins')[2]
    img = ref['images'][0]
    assert np.array_equal(img['oks'][:, 0].view(np.int64), img['oks'][:, 1].view(np.int64))
    assert img['oks'][0, 0] >= 0.5 + MARGIN
    assert img['taken'][0, 0] == 1 and img['taken'][1, 0] == 0 and img['flags'][:, 0].tolist() == [1, 1]


def test_an_ignored_annotation_behind_a_match_is_not_reached():
    ref = _case('stop')[2]
    img = ref['images'][0]
    assert img['oks'][0, 0] == 1.0 and 0.5 < img['oks'][0, 1] < 0.95   # the crowd copy (listed first) fits better
    assert img['taken'][0, 0] == 1 and img['flags'][0, 0] == 1          # ... and the plain one is taken where it passes,
    assert img['taken'][0, T - 1] == 0 and img['flags'][0, T - 1] == 3  # the crowd one only where it does not (t = .95)
    assert ref['precision'][0, 0, ALL] > 0.99


def test_out_of_range_annotations_and_detections_are_ignored():
    ref = _case('out_of_range_match')[2]
    assert _flags(ref, 0, ALL) == [1] * T and _flags(ref, 0, MED) == [3] * T and _flags(ref, 1, LARGE) == [3] * T
    s = ref['stats']
    assert abs(s[3] - 1.0) <= TOL and abs(s[4] - 1.0) <= TOL and abs(s[0] - 1.0) <= TOL
    gt, dt, ref = _case('out_of_range_det')
    assert cr.prepare(gt, dt)[2][1][0]['area'] > 96 ** 2
    assert _flags(ref, 0, ALL) == [0] * T and _flags(ref, 0, MED) == [2] * T and _flags(ref, 0, LARGE) == [0] * T
    s = ref['stats']
    assert abs(s[0] - 0.5) <= TOL and abs(s[3] - 1.0) <= TOL and s[4] == -1     # a false positive in front in `all` only


def test_an_area_on_a_bound_lies_in_both_ranges():
    ref = _case('edge_areas')[2]
    assert ref['images'][0]['npig'].tolist() == [2, 2, 1]
    s = ref['stats']
    assert abs(s[3] - 1.0) <= TOL and abs(s[4] - 1.0) <= TOL and s[8] == 1.0 and s[9] == 1.0


def test_an_annotation_without_a_labelled_joint():
    ref = _case('no_labelled_joint')[2]
    img = ref['images'][0]
    assert img['oks'][0, 0] == 1.0 and img['oks'][1, 0] < 0.5          # inside the doubled box: distance 0; outside: far
    assert img['npig'].tolist() == [1, 1, 0]                           # ... and it is ignored
    for a in range(A):
        assert _flags(ref, 0, a) == [3] * T
    assert _flags(ref, 1, ALL) == [0] * T


def test_without_a_counting_annotation_everything_is_minus_one():
    ref = _case('only_crowd')[2]
    assert (ref['stats'] == -1).all() and (ref['precision'] == -1).all() and (ref['recall'] == -1).all()
    assert ev.coco_keypoint_ap(ev.pack_coco_keypoints([], []))['stats'].tolist() == [-1.0] * 10      # no launch: no device needed
    empty = ev.coco_keypoint_ap(ev.pack_coco_keypoints([], [], img_ids=[3, 4]))
    assert (empty['precision'] == -1).all() and empty['precision'].shape == (10, 101, 3) and empty['names'] == cr.NAMES


def test_the_seeded_sets_decide_nothing_closely():
    for name, (gt, dt, ids), max_det in (('seeded', cr.seeded_set(), 20), ('caps', cr.caps_set(), 64), ('ties', cr.ties_set(), 18)):
        ref = cr.evaluate(gt, dt, max_det=max_det, img_ids=ids)
        print('%s: %d images, %d annotations, %d detections, margin %.3e, tie margin %.3e, AP %.4f'
              % (name, len(ids), len(gt), len(dt), ref['margin'], ref['tie_margin'], ref['stats'][0]))
        assert ref['margin'] >= MARGIN and ref['tie_margin'] >= MARGIN
        if name == 'seeded':
            n_gt, n_dt = np.bincount([g['image_id'] for g in gt], minlength=200), np.bincount([d['image_id'] for d in dt], minlength=200)
            assert ((n_gt == 0) & (n_dt == 0)).any() and ((n_gt > 0) & (n_dt == 0)).any() and ((n_gt == 0) & (n_dt > 0)).any()
            assert 0.05 < ref['stats'][0] < 0.95 and (ref['stats'] > -1).all() and len(ref['image_ids']) < 200
        if name == 'caps':
            assert [len(r['kept']) for r in ref['images']] == [4, 64, 6] and ref['images'][1]['oks'].shape == (64, 128)
        if name == 'ties':
            sc = sorted((d['score'] for d in dt), reverse=True)
            assert sc[17] == sc[18] and ref['images'][0]['rows'] == sorted(ref['images'][0]['rows'], key=lambda i: (-dt[i]['score'], i))


# ---------------------------------------------------------------------------------------- the host layer
def test_threshold_arrays_are_the_linspace_expressions():
    assert np.array_equal(ev.COCO_IOU_THRS.view(np.int64), np.linspace(.5, .95, 10).view(np.int64))
    assert np.array_equal(ev.COCO_REC_THRS.view(np.int64), np.linspace(0, 1, 101).view(np.int64))
    assert ev.COCO_IOU_THRS[8] == 0.8999999999999999 and ev.COCO_IOU_THRS.dtype == np.float64
    assert ev.COCO_AREA_RNGS.tolist() == [[0, 1e10], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]] and ev.COCO_MAX_DETS == 20
    assert np.array_equal(cr.IOU.view(np.int64), ev.COCO_IOU_THRS.view(np.int64)) and np.array_equal(cr.REC, ev.COCO_REC_THRS)
    assert np.array_equal(cr.SIG.view(np.int64), ev.COCO_SIGMAS.view(np.int64)) and ev.COCO_MAX_SET >= 131072


def test_pack_agrees_with_the_restatement_and_leaves_its_inputs():
    gt, dt, ids = cr.seeded_set()
    gt[3].pop('num_keypoints')
    gt[5].pop('iscrowd')
    gt0, dt0 = copy.deepcopy(gt), copy.deepcopy(dt)
    k = ev.pack_coco_keypoints(gt, dt, img_ids=ids)
    assert gt == gt0 and dt == dt0
    assert k['image_ids'] == ids and k['num_joints'] == 17 and k['gt_seg'].dtype == np.int32 and k['gt_flags'].dtype == np.int32
    _, G, D = cr.prepare(gt, dt, ids)
    g_all, d_all = [g for i in ids for g in G[i]], [d for i in ids for d in D[i]]
    assert k['gt_index'].tolist() == [g['pos'] for g in g_all] and k['dt_index'].tolist() == [d['pos'] for d in d_all]
    assert k['gt_seg'].tolist() == np.concatenate([[0], np.cumsum([len(G[i]) for i in ids])]).tolist()
    assert k['dt_seg'].tolist() == np.concatenate([[0], np.cumsum([len(D[i]) for i in ids])]).tolist()
    assert k['gt_flags'].tolist() == [g['ignore'] | (g['crowd'] << 1) for g in g_all] and (k['gt_flags'] == 3).any()
    assert np.array_equal(k['dt_area'], [d['area'] for d in d_all]) and np.array_equal(k['gt_area'], [g['area'] for g in g_all])
    assert np.array_equal(k['dt_kpts'], [d['kp'] for d in d_all]) and np.array_equal(k['gt_bbox'], [g['bbox'] for g in g_all])
    # ascending image id whatever the list order, list order within an image; other images left out
    sub = ev.pack_coco_keypoints(gt[::-1], dt[::-1], img_ids=[7, 2, 5])
    assert sub['image_ids'] == [2, 5, 7] and [gt[::-1][i]['image_id'] for i in sub['gt_index']] == sorted(g['image_id'] for g in gt if g['image_id'] in (2, 5, 7))
    assert (np.diff(sub['gt_index'][sub['gt_seg'][0]:sub['gt_seg'][1]]) > 0).all()


def test_pack_refuses():
    gt, dt, _ = cr.ties_set()

    def bad(g_edit=None, d_edit=None, match=None):
        g, d = copy.deepcopy(gt), copy.deepcopy(dt)
        if g_edit:
            g_edit(g)
        if d_edit:
            d_edit(d)
        with pytest.raises(ValueError, match=match):
            ev.pack_coco_keypoints(g, d)

    bad(lambda g: g[1]['keypoints'].__setitem__(4, float('nan')), match='non-finite')
    bad(d_edit=lambda d: d[2]['keypoints'].__setitem__(0, float('inf')), match='non-finite')
    bad(d_edit=lambda d: d[2].__setitem__('score', float('nan')), match='score')
    bad(lambda g: g[0].__setitem__('area', float('inf')), match='area')
    bad(lambda g: g[1]['keypoints'].pop(), match='keypoint values')
    bad(d_edit=lambda d: d[5]['keypoints'].extend([1.0, 2.0, 1.0]), match='not 3 x 17')
    bad(d_edit=lambda d: d[3].__setitem__('category_id', 2), match='one category')
    bad(lambda g: g[2].pop('area'), match="no 'area'")
    bad(lambda g: g[2].pop('bbox'), match="no 'bbox'")
    bad(d_edit=lambda d: d[0].pop('score'), match="no 'score'")
    bad(d_edit=lambda d: d[0].pop('image_id'), match='image_id')
    bad(lambda g: g.extend(copy.deepcopy(g[0]) for _ in range(123)), match='129 annotations')
    bad(d_edit=lambda d: d.extend(copy.deepcopy(d[0]) for _ in range(233)), match='257 detections')
    ok = ev.pack_coco_keypoints(gt + [copy.deepcopy(gt[0]) for _ in range(122)], dt + [copy.deepcopy(dt[0]) for _ in range(232)])
    assert ok['gt_seg'].tolist() == [0, 128] and ok['dt_seg'].tolist() == [0, 256]
    for kw, match in (({'max_dets': 0}, 'max_dets'), ({'max_dets': 65}, 'max_dets'), ({'max_dets': 2.0}, 'max_dets'),
                      ({'sigmas': np.ones(15)}, 'sigmas'), ({'iou_thrs': [0.5, float('nan')]}, 'finite'),
                      ({'rec_thrs': np.linspace(0, 1, 257)}, 'rec_thrs'), ({'area_rngs': [0, 1e10]}, 'area_rngs')):
        with pytest.raises(ValueError, match=match):
            ev.coco_keypoint_ap(ok, **kw)
    with pytest.raises(RuntimeError, match='HIP path only'):
        ev.coco_keypoint_ap(ok, device='cpu')


def test_result_dicts():
    rng = np.random.RandomState(0)
    preds, boxes = rng.uniform(0, 100, (5, 17, 3)), rng.uniform(0, 1, (5, 6))
    p0, b0 = preds.copy(), boxes.copy()
    res = ev.coco_keypoint_results(preds, boxes, np.array([9, 9, 4, 4, 4]), keep={'a': [1], 'b': [4, 2]})
    assert [r['image_id'] for r in res] == [9, 4, 4] and all(type(r['image_id']) is int and r['category_id'] == 1 for r in res)
    assert res[1]['keypoints'] == preds[4].reshape(-1).tolist() and res[1]['score'] == boxes[4, 5] and len(res[0]['keypoints']) == 51
    assert np.array_equal(preds, p0) and np.array_equal(boxes, b0)
    assert len(ev.coco_keypoint_results(preds, boxes, [1] * 5)) == 5
    assert [r['score'] for r in ev.coco_keypoint_results(preds, boxes, [1] * 5, keep=[3, 0])] == [boxes[3, 5], boxes[0, 5]]
    acc = ev.EvalAccumulator(8)
    acc.all_preds[:5], acc.all_boxes[:5], acc.idx = preds, boxes, 5
    assert acc.coco_results([9, 9, 4, 4, 4], keep=[1, 4, 2]) == res
    assert acc.coco_results([9, 9, 4, 4, 4], keep=[1], boxes=boxes * 2)[0]['score'] == 2 * boxes[1, 5]
    with pytest.raises(ValueError, match='image_ids'):
        ev.coco_keypoint_results(preds, boxes, [1, 2])
    with pytest.raises(ValueError, match='outside'):
        ev.coco_keypoint_results(preds, boxes, [1] * 5, keep=[5])
    import json
    json.dumps(res)                                                    # plain Python values: what a results file holds


def test_loader(tmp_path):
    import json
    gt, dt, ids = cr.ties_set()
    (tmp_path / 'gt.json').write_text(json.dumps({'images': [{'id': 7}, {'id': 8}], 'annotations': gt}))
    (tmp_path / 'dt.json').write_text(json.dumps(dt))
    g, d, i = ev.load_coco_keypoints(str(tmp_path / 'gt.json'), str(tmp_path / 'dt.json'))
    assert g == gt and d == dt and i == [7, 8]
    (tmp_path / 'other.json').write_text(json.dumps([dict(dt[0], image_id=99)]))
    with pytest.raises(ValueError, match='does not list'):
        ev.load_coco_keypoints(str(tmp_path / 'gt.json'), str(tmp_path / 'other.json'))
    with pytest.raises(ValueError, match='not a list'):
        ev.load_coco_keypoints(str(tmp_path / 'gt.json'), str(tmp_path / 'gt.json'))


def test_exports_and_prototypes():
    for name in ('pack_coco_keypoints', 'coco_keypoint_ap', 'load_coco_keypoints', 'evaluate_coco_keypoints', 'coco_keypoint_results'):
        assert name in fami_pose_amd.__all__ and getattr(fami_pose_amd, name) is getattr(ev, name)
    assert hasattr(ev.EvalAccumulator, 'coco_results')
    protos = parse_header()
    assert len(protos['fami_coco_kpt_match_f64'][1]) == 24 and len(protos['fami_coco_kpt_curve_f64'][1]) == 11
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert 'coco_ap.hip' in open(os.path.join(root, 'fami-pose_amd', 'csrc', 'Makefile')).read()
