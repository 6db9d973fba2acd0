"""Host side of the PoseTrack AP (evaluate.pack_posetrack_frames / load_posetrack_dirs / posetrack_ap,
csrc/posetrack_ap.hip): the numpy yardstick tests/_ap_ref.py against the fixture tests/golden/posetrack_ap.npz, the rules
of the restatement on hand-made cases, and everything the pack and the loader refuse before any device work.

The fixture holds what the reference's OWN evaluateAP returns on 200 seeded frames (tools/gen_ap_golden.py).  They carry
no ignore regions: the reference filters those with shapely, which is absent where the fixture was made; the even-odd
filter is held against hand-made polygons here instead.  The reference and the restatement make the same fp64 decisions
wherever none is closer to the threshold than a few ulp; the smallest decision margin on the fixture is asserted."""
import copy
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ap_ref as ar  # noqa: E402

import fami_pose_amd as fp  # noqa: E402
from fami_pose_amd import evaluate as ev  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'posetrack_ap.npz')
ALL = np.ones(ar.J, bool)
HEAD = np.array([0.0, 0.0, 30.0, 40.0])                          # head size 0.6 * 50 = 30: the threshold is 15 pixels


def _grid_pose(x0, y0):
    """15 joints on a line, 100 pixels apart."""
    return np.stack([x0 + 100.0 * np.arange(ar.J), np.full(ar.J, float(y0))], 1)


def _frame(g_rects, p_rects, regions=None):
    g = {'annorect': g_rects}
    if regions is not None:
        g['ignore_regions'] = regions
    return g, {'annorect': p_rects}


def _region(pts):
    return {'point': [{'x': [float(x)], 'y': [float(y)]} for x, y in pts]}


def _lists(*frames):
    return [f[0] for f in frames], [f[1] for f in frames]


@pytest.fixture(scope='module')
def fixture_ref():
    packed, want = ar.load_fixture(GOLD)
    gt, pr = ar.unpack(packed)
    return packed, want, gt, pr, ar.evaluate_ap(gt, pr)


# ---------------------------------------------------------------------------------------- the fixture
def test_restatement_reproduces_the_reference_fixture(fixture_ref):
    packed, (ap, pre, rec), gt, pr, mine = fixture_ref
    assert 100 <= len(packed['pr_has']) <= 1000 and len(packed['frame_index']) < 200     # some frames were dropped
    for k, want in (('ap', ap), ('pre', pre), ('rec', rec)):
        assert want.shape == (16,) and np.array_equal(np.isnan(mine[k]), np.isnan(want))
        assert np.nanmax(np.abs(mine[k] - want)) <= 1e-9
    assert 20.0 <= ap[15] <= 80.0
    print('margin %.3e, total AP %.4f' % (mine['margin'], ap[15]))


def test_fixture_is_not_vacuous(fixture_ref):
    packed, want, gt, pr, mine = fixture_ref
    assert mine['margin'] >= 1e-9
    assert all(len(set(s)) == len(s) for s in mine['scores'])    # no equal scores: the reference's order is determined
    assert mine['outcompeted'] >= 1                                # within the threshold, yet another prediction took the pose
    assert mine['empty_gt_frames'] >= 1                            # predictions and no annotated pose left
    assert mine['unmatched_gt'] >= 1                               # an annotated pose nobody matched
    assert len(set(np.round(want[0][:15], 6))) > 5                 # the curves are not flat


def test_pack_of_the_unpacked_fixture_is_the_fixture(fixture_ref):
    packed, want, gt, pr, mine = fixture_ref
    again = ev.pack_posetrack_frames(gt, pr)
    for k in ('pr_xys', 'pr_has', 'gt_xy', 'gt_has', 'gt_head', 'pr_seg', 'gt_seg', 'poly_seg', 'vert_seg', 'verts'):
        assert again[k].dtype == packed[k].dtype and np.array_equal(again[k], packed[k]), k
    assert np.array_equal(mine['pr_has'], packed['pr_has']) and np.array_equal(mine['gt_has'], packed['gt_has'])


# ---------------------------------------------------------------------------------------- tie rules
def test_one_prediction_equally_good_for_two_poses_takes_the_first():
    a = _grid_pose(0, 0)
    g = [ar.gt_rect(a, ALL, HEAD, 0), ar.gt_rect(a, ALL, HEAD, 1)]                 # the same pose twice
    p = [ar.pr_rect(a + 1.0, ALL, np.linspace(0.5, 0.9, ar.J))]
    r = ar.evaluate_ap(*_lists(_frame(g, p)))
    assert list(r['assigned']) == [0] and r['label'][0] == 0x7fff and r['unmatched_gt'] == 1
    assert np.allclose(r['rec'][:15], 50.0) and np.allclose(r['pre'][:15], 100.0)


def test_two_predictions_equally_good_for_one_pose_the_first_takes_it():
    a = _grid_pose(0, 0)
    g = [ar.gt_rect(a, ALL, HEAD, 0)]
    p = [ar.pr_rect(a + 1.0, ALL, np.full(ar.J, 0.3)), ar.pr_rect(a - 1.0, ALL, np.full(ar.J, 0.9))]
    r = ar.evaluate_ap(*_lists(_frame(g, p)))
    assert list(r['assigned']) == [0, -1] and list(r['label']) == [0x7fff, 0] and r['outcompeted'] == 1
    # the second one scores higher and is a false positive: it leads every curve
    assert np.allclose(r['ap'][:15], 50.0) and np.allclose(r['pre'][:15], 50.0) and np.allclose(r['rec'][:15], 100.0)


def test_equal_scores_keep_frame_then_pose_order():
    a, far = _grid_pose(0, 0), _grid_pose(0, 5000)
    one = np.full(ar.J, 0.5)
    # frame 0: a miss, then a hit; frame 1: a hit -- all with the same score.  Order: miss, hit, hit
    f0 = _frame([ar.gt_rect(a, ALL, HEAD)], [ar.pr_rect(far, ALL, one), ar.pr_rect(a, ALL, one)])
    f1 = _frame([ar.gt_rect(a, ALL, HEAD)], [ar.pr_rect(a, ALL, one)])
    r = ar.evaluate_ap(*_lists(f0, f1))
    # precision = 0, 1/2, 2/3: the envelope is 2/3 at all three; AP = (1/2) * 2/3 + (1/2) * 2/3
    assert np.allclose(r['ap'][:15], (2.0 / 3.0) * 100.0, atol=1e-12)
    # the other order of the frames: hit, miss, hit -> precision 1, 1/2, 2/3
    r2 = ar.evaluate_ap(*_lists(f1, f0))
    assert np.allclose(r2['ap'][:15], (0.5 * 1.0 + 0.5 * (2.0 / 3.0)) * 100.0, atol=1e-12)


# ---------------------------------------------------------------------------------------- the two quirks of the curve
def test_curve_quirks():
    a = _grid_pose(0, 0)
    g_has = ALL.copy()
    g_has[3] = False                                              # joint 3: predicted, never annotated -> NaN
    p_has = ALL.copy()
    p_has[7] = False                                              # joint 7: annotated, never predicted -> 0, counted
    r = ar.evaluate_ap(*_lists(_frame([ar.gt_rect(a, g_has, HEAD)], [ar.pr_rect(a, p_has, np.linspace(0.1, 0.9, ar.J))])))
    assert np.isnan(r['ap'][3]) and np.isnan(r['rec'][3]) and r['pre'][3] == 0.0
    assert r['ap'][7] == 0.0 and r['pre'][7] == 0.0 and r['rec'][7] == 0.0
    others = [j for j in range(15) if j not in (3, 7)]
    assert np.allclose(r['ap'][others], 100.0)
    assert np.isclose(r['ap'][15], 100.0 * 13 / 14) and np.isclose(r['rec'][15], 100.0 * 13 / 14)
    assert np.isclose(r['pre'][15], 100.0 * 13 / 15)             # pre has no NaN: 15 joints in its mean
    assert ar.curve([], [], 5)[:3] == (0.0, 0.0, 0.0)
    ap, pre, rec, _ = ar.curve([0.9, 0.8], [0, 0], 0)
    assert np.isnan(ap) and pre == 0.0 and np.isnan(rec)
    assert ev._get_cum(r['ap'])[7] == r['ap'][15] and np.allclose(ev._get_cum(r['ap']), ar.get_cum(r['ap']), equal_nan=True)


# ---------------------------------------------------------------------------------------- the even-odd filter
CONCAVE = [(0, 0), (100, 0), (100, 100), (50, 20), (0, 100)]      # a square with a notch cut in from the top edge


def test_even_odd_on_a_concave_polygon():
    poly = np.array(CONCAVE, dtype=np.float64)
    for (x, y), want in (((10, 10), True), ((90, 50), True), ((3, 90), True), ((50, 60), False), ((50, 10), True),
                         ((150, 50), False), ((-5, 5), False), ((50, 150), False), ((30, 70), False), ((10, 70), True)):
        assert ar.point_in_polygon(float(x), float(y), poly) == want, (x, y)


def test_ignore_regions_in_the_selection_and_the_pack():
    a = _grid_pose(10, 10)                                        # joint 0 at (10, 10): inside; joint 1 at (110, 10): outside
    lone = np.zeros(ar.J, bool)
    lone[0] = True
    reg = [_region(CONCAVE)]
    # frame 0: two annotated poses, the second has only joint 0 (emptied by the filter); one prediction
    f0 = _frame([ar.gt_rect(a, ALL, HEAD, 0), ar.gt_rect(a, lone, HEAD, 1)], [ar.pr_rect(a + 1.0, ALL, np.linspace(0.2, 0.8, ar.J))], reg)
    # frame 1: the same points, no region of its own: frame 0's polygon does not apply
    f1 = _frame([ar.gt_rect(a, ALL, HEAD, 0)], [ar.pr_rect(a + 1.0, ALL, np.linspace(0.2, 0.8, ar.J))])
    # frame 2: the only annotated pose is emptied: its prediction (joint 1 survives) is a false positive
    f2 = _frame([ar.gt_rect(a, lone, HEAD, 0)], [ar.pr_rect(a + 1.0, ALL, np.linspace(0.2, 0.8, ar.J))], reg)
    gt, pr = _lists(f0, f1, f2)
    frames = ar.select_frames(gt, pr)
    assert [len(f['gt']) for f in frames] == [1, 1, 0] and [f['n_gt_packed'] for f in frames] == [2, 1, 1]
    r = ar.evaluate_ap(gt, pr)
    assert list(r['gt_has']) == [0x7ffe, 0, 0x7fff, 0] and list(r['pr_has']) == [0x7ffe, 0x7fff, 0x7ffe]
    assert list(r['assigned']) == [0, 0, -1] and list(r['label']) == [0x7ffe, 0x7fff, 0] and r['empty_gt_frames'] == 1
    assert list(r['ngt']) == [1] + [2] * 14
    packed = ev.pack_posetrack_frames(gt, pr)
    assert list(packed['poly_seg']) == [0, 1, 1, 2] and list(packed['vert_seg']) == [0, 5, 10]
    assert np.array_equal(packed['verts'], np.array(CONCAVE + CONCAVE, dtype=np.float64))
    assert list(packed['gt_seg']) == [0, 2, 3, 4] and list(packed['gt_has']) == [0x7fff, 1, 0x7fff, 1]   # the filter is the device's


# ---------------------------------------------------------------------------------------- the pack
def test_pack_selection_scores_and_first_id():
    a = _grid_pose(0, 0)
    bare = ar.gt_rect(a, ALL, HEAD)
    bare['annopoints'] = []
    p = ar.pr_rect(a, ALL, np.linspace(0.1, 0.9, ar.J))
    pts = p['annopoints'][0]['point']
    del pts[2]['score']                                            # joint 2: MIN_SCORE
    pts.append({'id': [4], 'x': [1.0], 'y': [2.0], 'score': [0.99]})     # joint 4 again: the first counts
    pts.append({'id': None, 'x': [1.0], 'y': [2.0]})
    nopoint = {'score': [0.1], 'annopoints': [{}]}
    f0 = _frame([], [p])                                           # no annotated rect: dropped with its prediction
    f1 = _frame([ar.gt_rect(a, ALL, HEAD), bare], [p, nopoint])
    f2 = _frame([bare], [p])                                       # stays, with no annotated pose
    gt, pr = _lists(f0, f1, f2)
    before = copy.deepcopy((gt, pr))
    k = ev.pack_posetrack_frames(gt, pr)
    assert (gt, pr) == before                                      # neither input is modified
    assert list(k['frame_index']) == [1, 2] and list(k['pr_seg']) == [0, 1, 2] and list(k['gt_seg']) == [0, 1, 1]
    assert k['pr_xys'].dtype == np.float64 and k['pr_xys'].shape == (2, 15, 3) and k['gt_head'].shape == (1, 4)
    assert k['pr_xys'][0, 2, 2] == -9999 and k['pr_xys'][0, 4, 2] == p['annopoints'][0]['point'][4]['score'][0]
    assert np.array_equal(k['pr_xys'][0, :, :2], a) and list(k['pr_has']) == [0x7fff, 0x7fff]
    r = ar.evaluate_ap(gt, pr)
    assert np.array_equal(r['frame_index'], k['frame_index']) and r['empty_gt_frames'] == 1
    assert fp.pack_posetrack_frames is ev.pack_posetrack_frames and fp.posetrack_ap is ev.posetrack_ap
    for name in ('pack_posetrack_frames', 'load_posetrack_dirs', 'posetrack_ap', 'evaluate_posetrack_ap'):
        assert name in fp.__all__


def test_pack_refusals():
    a = _grid_pose(0, 0)
    g, p = ar.gt_rect(a, ALL, HEAD), ar.pr_rect(a, ALL, np.full(ar.J, 0.5))
    with pytest.raises(ValueError, match='2 ground-truth frames, 1 prediction'):
        ev.pack_posetrack_frames([{'annorect': [g]}] * 2, [{'annorect': [p]}])
    for bad_id in (15, -1):
        q = copy.deepcopy(p)
        q['annopoints'][0]['point'][3]['id'] = [bad_id]
        with pytest.raises(ValueError, match='outside 0 .. 14'):
            ev.pack_posetrack_frames([{'annorect': [g]}], [{'annorect': [q]}])
    for key, val in (('x', float('nan')), ('y', float('inf')), ('score', float('-inf'))):
        q = copy.deepcopy(p)
        q['annopoints'][0]['point'][3][key] = [val]
        with pytest.raises(ValueError, match='not finite'):
            ev.pack_posetrack_frames([{'annorect': [g]}], [{'annorect': [q]}])
    q = copy.deepcopy(g)
    q['annopoints'][0]['point'][0]['x'] = [float('nan')]
    with pytest.raises(ValueError, match='not finite'):
        ev.pack_posetrack_frames([{'annorect': [q]}], [{'annorect': [p]}])
    ok = _frame([g], [p])
    with pytest.raises(ValueError, match='frame 1 has 257 predicted'):
        ev.pack_posetrack_frames(*_lists(ok, _frame([g], [p] * 257)))
    with pytest.raises(ValueError, match='frame 1 has 1 predicted and 65 annotated'):
        ev.pack_posetrack_frames(*_lists(ok, _frame([g] * 65, [p])))
    ev.pack_posetrack_frames(*_lists(_frame([g] * 64, [p] * 256)))            # at the caps: accepted
    q = copy.deepcopy(g)
    del q['x2']
    with pytest.raises(ValueError, match='head rectangle'):
        ev.pack_posetrack_frames([{'annorect': [q]}], [{'annorect': [p]}])
    with pytest.raises(ValueError, match='polygon needs 3'):
        ev.pack_posetrack_frames(*_lists(_frame([g], [p], [_region([(0, 0), (1, 1)])])))
    q = copy.deepcopy(p)
    q['annopoints'][0]['point'].append({'id': [0], 'x': [1.0], 'y': [1.0], 'score': [0.1]})
    ev.pack_posetrack_frames([{'annorect': [g]}], [{'annorect': [q]}])        # fine without regions
    with pytest.raises(ValueError, match='listed twice'):
        ev.pack_posetrack_frames(*_lists(_frame([g], [q], [_region(CONCAVE)])))


def test_empty_set_needs_no_device():
    r = ev.posetrack_ap(ev.pack_posetrack_frames([], []))
    for k in ('ap', 'pre', 'rec'):
        assert r[k].shape == (16,) and r[k].dtype == np.float64 and not r[k].any()
    assert r['cum'] == [0.0] * 8 and r['names'][:15] == ar.NAMES and r['names'][15] == 'total'
    a = _grid_pose(0, 0)
    dropped = ev.pack_posetrack_frames(*_lists(_frame([], [ar.pr_rect(a, ALL, np.full(ar.J, 0.5))])))
    assert len(dropped['frame_index']) == 0 and ev.posetrack_ap(dropped)['cum'][7] == 0.0
    ref = ar.evaluate_ap([], [])
    assert not ref['ap'].any() and ref['cum'] == [0.0] * 8


# ---------------------------------------------------------------------------------------- the loader
def test_load_posetrack_dirs(tmp_path):
    rng = np.random.RandomState(3)
    gt_a, pr_a = ar.make_annolists(rng, 4)
    gt_b, pr_b = ar.make_annolists(rng, 3)
    gd, pd = tmp_path / 'gt', tmp_path / 'pred'
    gd.mkdir()
    pd.mkdir()
    for name, g, p in (('b_seq.json', gt_b, pr_b), ('a_seq.json', gt_a, pr_a)):
        (gd / name).write_text(json.dumps({'annolist': g}))
        (pd / name).write_text(json.dumps({'annolist': p}))
    (gd / 'notes.txt').write_text('not an annotation file')
    g, p = ev.load_posetrack_dirs(str(gd), str(pd))
    assert g == gt_a + gt_b and p == pr_a + pr_b                   # sorted by base name; JSON keeps every double
    k = ev.pack_posetrack_frames(g, p)
    r = ar.evaluate_ap(gt_a + gt_b, pr_a + pr_b)
    assert np.array_equal(k['frame_index'], r['frame_index']) and len(k['pr_has']) == len(r['pr_has'])
    (pd / 'b_seq.json').write_text(json.dumps({'annolist': pr_b[:2]}))
    with pytest.raises(ValueError, match='# prediction frames 2 != # GT frames 3'):
        ev.load_posetrack_dirs(str(gd), str(pd))
    (pd / 'b_seq.json').unlink()
    with pytest.raises(IOError, match='does not exist'):
        ev.load_posetrack_dirs(str(gd), str(pd))
    (pd / 'b_seq.json').write_text(json.dumps({'images': [], 'annotations': []}))
    with pytest.raises(ValueError, match='out of scope'):
        ev.load_posetrack_dirs(str(gd), str(pd))
    (pd / 'b_seq.json').write_text(json.dumps({'annolist': pr_b}))
    (gd / 'b_seq.json').write_text(json.dumps({'images': [], 'annotations': []}))
    with pytest.raises(ValueError, match='out of scope'):
        ev.load_posetrack_dirs(str(gd), str(pd))
