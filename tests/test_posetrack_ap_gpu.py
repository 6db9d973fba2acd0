"""PoseTrack AP on the MI355X (csrc/posetrack_ap.hip: fami_posetrack_assign_f64, fami_posetrack_curve_f64;
evaluate.posetrack_ap / evaluate_posetrack_ap) against the float64 restatement tests/_ap_ref.py and the reference-made
fixture tests/golden/posetrack_ap.npz (tests/test_posetrack_ap_host.py says what that fixture pins; it carries no ignore
regions, because the reference filters those with shapely, which was absent where it was made).

Bounds.  `label`, `assigned`, `ngt` and the masks left by the ignore filter must be EQUAL: the kernel and the restatement
evaluate the same fp64 expressions, and what can differ (a contracted multiply-add in numpy's build, the last bit of a
square root) is a few ulp ~ 1e-15 relative, so equality is demanded of inputs on which no distance is that close to the
threshold: every family is seeded, and its smallest decision margin min |dist - thresh| / thresh is asserted to be >= 1e-9
before anything is launched.  No polygon test point lies within 1e-6 of an edge (asserted too).
ap / pre / rec must agree within 1e-9 on the 0-100 scale, NaN positions equal: the quotients are the reference's
expressions, only the order of the AP sum differs; at most n <= 10^4 fp64 additions of terms that sum to <= 1 are off by
at most n * 2^-53 * 100 ~ 1e-10 (the number of terms is asserted; the restatement's own sum is math.fsum, exact to one
rounding).  Two runs must agree bit for bit, and the guard words behind every output must be intact.

Shapes (the smallest at which the kernels can go wrong): frames of annotated poses and 0 predictions, 1 x 1, 63 / 64 / 65
predictions (the wave boundary) and 256 (the cap) against 1, 2 and 64 annotated poses (the cap); a pose with no annotated
joint, a prediction with no joint, a head rectangle of size 0, a prediction without a score; one prediction equally good
for two poses, two predictions equally good for one pose, equal scores; a joint absent from every prediction and one
absent from every annotation; concave ignore polygons with points inside and outside, a rect and a frame emptied by them,
a frame whose neighbour's polygon must not apply; per-joint list lengths around a 64-label word (63 / 64 / 65 / 193) and
around the 256-word round after which a thread owns a second word (16383 / 16384 / 16385, three rounds + 1 = 49153)."""
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ap_ref as ar  # noqa: E402

from fami_pose_amd import evaluate as ev  # noqa: E402
from fami_pose_amd._lib import lib  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'posetrack_ap.npz')
MARGIN = 1e-9
TOL = 1e-9
MAX_TERMS = 10 ** 4
GUARD = 256
SENT = 0x5a5a5a5a
J = ar.J
MISS_PR, MISS_GT = 7, 3                                           # never predicted / never annotated in the shapes family
CONCAVE = np.array([(0, 0), (100, 0), (100, 100), (50, 20), (0, 100)], dtype=np.float64)


# ---------------------------------------------------------------------------------------- inputs
def _people(rng, n_g, n_p, p_joint_gt=0.85):
    """One frame: n_g annotated people and n_p predictions dealt round-robin over them (several per person: competition);
    without an annotated person the predictions are of people nobody annotated."""
    people = [ar.make_person(rng, p_joint_gt) for _ in range(max(n_g, 1))]
    g_rects, p_rects = [], []
    for i in range(n_g):
        xy, present, head, size = people[i]
        present = present.copy()
        present[MISS_GT] = False
        g_rects.append(ar.gt_rect(xy, present, head, i))
    for i in range(n_p):
        xy, _, _, size = people[i % len(people)]
        pxy, present, score = ar.make_prediction(rng, xy, size, rng.uniform(0.05, 0.9))
        present[MISS_PR] = False
        p_rects.append(ar.pr_rect(pxy, present, score, i))
    return {'annorect': g_rects}, {'annorect': p_rects}


def _shapes_family():
    rng = np.random.RandomState(11)
    frames = [_people(rng, n_g, n_p) for n_g, n_p in ((3, 0), (1, 1), (1, 63), (2, 64), (64, 65), (64, 256), (2, 5))]
    no_pr, no_gt = np.ones(J, bool), np.ones(J, bool)
    no_pr[MISS_PR], no_gt[MISS_GT] = False, False
    xy, _, head, size = ar.make_person(rng)
    # a pose with no annotated joint (first in its frame: every all-zero pck row points at it), a prediction with no joint
    f = _people(rng, 2, 3)
    f[0]['annorect'].insert(0, ar.gt_rect(xy, np.zeros(J, bool), head, 9))
    f[1]['annorect'].insert(1, ar.pr_rect(xy, np.zeros(J, bool), np.zeros(J), 9))
    frames.append(f)
    # a head rectangle of size 0: dist = inf or NaN (0 / 0 for the joints predicted exactly), nothing matches
    flat = head.copy()
    flat[2:] = flat[:2]
    frames.append(({'annorect': [ar.gt_rect(xy, no_gt, flat, 0)]},
                   {'annorect': [ar.pr_rect(xy, no_pr, np.linspace(0.31, 0.39, J), 0),
                                 ar.pr_rect(xy + 3.0, no_pr, np.linspace(0.41, 0.49, J), 1)]}))
    # one prediction equally good for two poses (the same pose twice): it takes the first
    frames.append(({'annorect': [ar.gt_rect(xy, no_gt, head, 0), ar.gt_rect(xy, no_gt, head, 1)]},
                   {'annorect': [ar.pr_rect(xy + 1.0, no_pr, np.linspace(0.51, 0.59, J), 0)]}))
    # two predictions equally good for one pose, equal scores among them and with the frame behind: the first takes it
    tie = np.full(J, 0.625)
    frames.append(({'annorect': [ar.gt_rect(xy, no_gt, head, 0)]},
                   {'annorect': [ar.pr_rect(xy + 1.0, no_pr, tie, 0), ar.pr_rect(xy - 1.0, no_pr, tie, 1)]}))
    frames.append(({'annorect': [ar.gt_rect(xy, no_gt, head, 0)]},
                   {'annorect': [ar.pr_rect(xy + 500.0, no_pr, tie, 0), ar.pr_rect(xy + 1.0, no_pr, tie, 1)]}))
    # predicted points without a score: MIN_SCORE, last in their curves
    f = _people(rng, 1, 2)
    for pt in f[1]['annorect'][0]['annopoints'][0]['point'][:5]:
        del pt['score']
    frames.append(f)
    # a frame left without an annotated pose (its only rect has no point list) and a dropped frame
    bare = ar.gt_rect(xy, no_gt, head, 0)
    bare['annopoints'] = []
    frames.append(({'annorect': [bare]}, _people(rng, 0, 2)[1]))
    frames.append(({'annorect': []}, _people(rng, 0, 2)[1]))
    return [f[0] for f in frames], [f[1] for f in frames]


def _region(poly):
    return {'point': [{'x': [float(x)], 'y': [float(y)]} for x, y in poly]}


def _edge_distance(x, y, poly):
    a, b = poly, np.roll(poly, -1, axis=0)
    ab, ap = b - a, np.array([x, y]) - a
    t = np.clip((ap * ab).sum(1) / (ab * ab).sum(1), 0.0, 1.0)
    return float(np.sqrt(((ap - t[:, None] * ab) ** 2).sum(1)).min())


def _polygon_family():
    rng = np.random.RandomState(5)
    gt, pr = [], []
    polys_of = []
    for f in range(6):
        polys = [CONCAVE * rng.uniform(2.0, 4.0) + rng.uniform(200, 600, 2) for _ in range(rng.randint(1, 3))]
        g_rects, p_rects = [], []
        for i in range(3):
            xy, present, head, size = ar.make_person(rng)
            xy = xy - xy.mean(0) + polys[0].mean(0) + rng.normal(0, 60, 2)      # people straddle the first polygon
            g_rects.append(ar.gt_rect(xy, present, head, i))
            for _ in range(2):
                p_rects.append(ar.pr_rect(*ar.make_prediction(rng, xy, size, rng.uniform(0.05, 0.6)), track_id=len(p_rects)))
        gt.append({'annorect': g_rects, 'ignore_regions': [_region(q) for q in polys]})
        pr.append({'annorect': p_rects})
        polys_of.append(polys)
    # frame 6 holds the points of frame 0 and no region of its own: frame 0's polygons must not apply to it
    gt.append({'annorect': copy.deepcopy(gt[0]['annorect'])})
    pr.append(copy.deepcopy(pr[0]))
    polys_of.append([])
    # frame 7: a rect emptied by the filter (its one joint is inside) next to one that stays; frame 8: emptied of ground truth
    q = CONCAVE * 3.0 + 300.0
    inside, outside = q[0] + np.array([20.0, 20.0]), q[0] - np.array([50.0, 50.0])
    lone = np.zeros(J, bool)
    lone[2] = True
    xy_in, xy_out = np.tile(inside, (J, 1)), np.tile(outside, (J, 1)) + 40.0 * np.arange(J)[:, None] * np.array([-1.0, 0.0])
    head = np.array([0.0, 0.0, 30.0, 40.0])
    gt.append({'annorect': [ar.gt_rect(xy_in, lone, head, 0), ar.gt_rect(xy_out, np.ones(J, bool), head, 1)],
               'ignore_regions': [_region(q)]})
    pr.append({'annorect': [ar.pr_rect(xy_out + 2.0, np.ones(J, bool), np.linspace(0.2, 0.7, J), 0),
                            ar.pr_rect(xy_in + 1.0, lone, np.linspace(0.3, 0.8, J), 1)]})
    polys_of.append([q])
    gt.append({'annorect': [ar.gt_rect(xy_in, lone, head, 0)], 'ignore_regions': [_region(q)]})
    pr.append({'annorect': [ar.pr_rect(xy_out + 2.0, np.ones(J, bool), np.linspace(0.25, 0.75, J), 0)]})
    polys_of.append([q])
    near = min(_edge_distance(pt['x'][0], pt['y'][0], q) for src, polys in zip(zip(gt, pr), polys_of) for fr in src
               for r in fr['annorect'] for pt in r['annopoints'][0]['point'] for q in polys)
    return gt, pr, near


_FAMILIES = {}


def _family(name):
    """-> (gt, pr, restatement, packed); everything that is asserted of the inputs is asserted here, before any launch."""
    if name not in _FAMILIES:
        if name == 'fixture':
            packed, want = ar.load_fixture(GOLD)
            gt, pr = ar.unpack(packed)
        elif name == 'shapes':
            gt, pr = _shapes_family()
        else:
            gt, pr, near = _polygon_family()
            assert near >= 1e-6, near
        ref = ar.evaluate_ap(gt, pr)
        packed = ev.pack_posetrack_frames(gt, pr)
        print('%s: %d frames, %d predicted / %d annotated poses, margin %.3e, longest AP sum %d terms'
              % (name, len(packed['frame_index']), len(packed['pr_has']), len(packed['gt_has']), ref['margin'], ref['terms']))
        assert ref['margin'] >= MARGIN and ref['terms'] <= MAX_TERMS
        assert np.array_equal(ref['frame_index'], packed['frame_index'])
        if name == 'shapes':
            n_p, n_g = np.diff(packed['pr_seg']), np.diff(packed['gt_seg'])
            assert list(zip(n_g[:6], n_p[:6])) == [(3, 0), (1, 1), (1, 63), (2, 64), (64, 65), (64, 256)]
            assert len(packed['frame_index']) == len(gt) - 1 and n_g[-1] == 0 and n_p[-1] == 2
            assert ref['ngt'][MISS_GT] == 0 and len(ref['scores'][MISS_GT]) > 0 and np.isnan(ref['ap'][MISS_GT])
            assert ref['ngt'][MISS_PR] > 0 and len(ref['scores'][MISS_PR]) == 0 and ref['ap'][MISS_PR] == 0.0
            assert ref['outcompeted'] >= 100 and ref['unmatched_gt'] >= 1 and ref['empty_gt_frames'] == 1
            assert any(len(set(s)) < len(s) for s in ref['scores'])                 # equal scores occur
            assert min(min(s) for s in ref['scores'] if s) == ar.MIN_SCORE
            seg = packed['pr_seg']
            tie = [int(seg[f]) for f in range(len(seg) - 1) if n_g[f] == 2 and n_p[f] == 1][0]
            assert ref['assigned'][tie] == 0 and ref['label'][tie] == 0x7fff & ~(1 << MISS_PR) & ~(1 << MISS_GT)
            flat = [f for f in range(len(n_g)) if n_g[f] == 1 and n_p[f] == 2][0]   # the head of size 0: nobody matches
            assert (ref['assigned'][seg[flat]:seg[flat + 1]] == -1).all()
        if name == 'polygons':
            assert len(packed['verts']) > 0 and (ref['pr_has'] != packed['pr_has']).any() and (ref['gt_has'] != packed['gt_has']).any()
            assert ((ref['pr_has'] != 0) & (ref['pr_has'] == packed['pr_has'])).any()     # points outside too
            s0, s6 = packed['pr_seg'][0], packed['pr_seg'][6]
            n0 = packed['pr_seg'][1] - s0
            assert (ref['pr_has'][s0:s0 + n0] != packed['pr_has'][s0:s0 + n0]).any()       # frame 0 is filtered,
            assert np.array_equal(ref['pr_has'][s6:s6 + n0], packed['pr_has'][s6:s6 + n0])  # its copy without a region is not
            g7 = packed['gt_seg'][7]
            assert list(ref['gt_has'][g7:g7 + 3]) == [0, 0x7fff, 0] and ref['empty_gt_frames'] == 1
            assert list(ref['assigned'][-3:]) == [1, -1, -1]       # packed index 1: the emptied rect keeps its place
        _FAMILIES[name] = (gt, pr, ref, packed)
    return _FAMILIES[name]


# ---------------------------------------------------------------------------------------- raw launches, guarded outputs
def _guarded(dev, words):
    return torch.full((GUARD + words + GUARD,), SENT, dtype=torch.int32, device=dev)


def _unguard(t, words):
    a = t.cpu().numpy()
    return a[GUARD:GUARD + words].copy(), bool((a[:GUARD] == SENT).all() and (a[GUARD + words:] == SENT).all())


def _raw_assign(dev, k, thresh=0.5):
    """The entry point itself on packed arrays -> (pr_has_out, gt_has_out, label, assigned, ngt_frame [F,15]), guards intact?"""
    P, G, F = len(k['pr_has']), len(k['gt_has']), len(k['pr_seg']) - 1
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt).reshape(-1)).to(dev)  # noqa: E731
    keep = [up(k[n], np.float64) for n in ('pr_xys', 'gt_xy', 'gt_head', 'verts')] + \
           [up(k[n], np.int32) for n in ('pr_has', 'gt_has', 'pr_seg', 'gt_seg', 'poly_seg', 'vert_seg')]
    pr_xys, gt_xy, gt_head, verts, pr_has, gt_has, pr_seg, gt_seg, poly_seg, vert_seg = (t.data_ptr() for t in keep)
    sizes = (P, G, P, P, F * J)
    outs = [_guarded(dev, n) for n in sizes]
    lib().call('fami_posetrack_assign_f64', pr_xys, pr_has, gt_xy, gt_has, gt_head, pr_seg, gt_seg, poly_seg, vert_seg, verts,
               P, G, F, len(k['vert_seg']) - 1, len(k['verts']), float(thresh), *[t[GUARD:].data_ptr() for t in outs],
               torch.cuda.current_stream(dev).cuda_stream)
    res = [_unguard(t, n) for t, n in zip(outs, sizes)]
    return [r[0] for r in res[:4]] + [res[4][0].reshape(F, J)], all(r[1] for r in res)


def _raw_curve(dev, lab, n_valid, ngt_frame):
    """lab [15,P] uint8, n_valid [15], ngt_frame [F,15] -> (out [3,16] float64, ngt [15]), guards intact?"""
    P, F = lab.shape[1], len(ngt_frame)
    d_lab = torch.from_numpy(np.ascontiguousarray(lab, dtype=np.uint8)).to(dev)
    d_n = torch.from_numpy(np.ascontiguousarray(n_valid, dtype=np.int32)).to(dev)
    d_f = torch.from_numpy(np.ascontiguousarray(ngt_frame, dtype=np.int32)).to(dev)
    out, ngt = _guarded(dev, 96), _guarded(dev, J)                 # GUARD words = 1 KiB: the doubles stay 8-byte aligned
    lib().call('fami_posetrack_curve_f64', d_lab.data_ptr(), d_n.data_ptr(), d_f.data_ptr(), P, F, out[GUARD:].data_ptr(),
               ngt[GUARD:].data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    (o, ok1), (n, ok2) = _unguard(out, 96), _unguard(ngt, J)
    return o.view(np.float64).reshape(3, 16), n, ok1 and ok2


def _close(got, want):
    return np.array_equal(np.isnan(got), np.isnan(want)) and (np.isnan(want).all() or np.nanmax(np.abs(got - want)) <= TOL)


def _sorted_labels(ref, P):
    """The curve kernel's input from the restatement: lab [15,P], n_valid [15] (stable descending order)."""
    lab, n_valid = np.zeros((J, max(P, 1)), np.uint8), np.zeros(J, np.int32)
    for j in range(J):
        s, l = np.asarray(ref['scores'][j], dtype=np.float64), np.asarray(ref['labels'][j], dtype=np.uint8)
        n_valid[j] = len(s)
        lab[j, :len(s)] = l[np.argsort(-s, kind='stable')]
    return lab, n_valid


# ---------------------------------------------------------------------------------------- 1. against float64
@pytest.mark.parametrize('name', ['fixture', 'shapes', 'polygons'])
def test_against_the_restatement(dev, name):
    gt, pr, ref, packed = _family(name)
    runs = [_raw_assign(dev, packed) for _ in range(2)]
    (pr_has, gt_has, label, assigned, ngt_frame), intact = runs[0]
    assert intact
    assert np.array_equal(pr_has, ref['pr_has']) and np.array_equal(gt_has, ref['gt_has'])
    assert np.array_equal(label, ref['label']) and np.array_equal(assigned, ref['assigned'])
    assert np.array_equal(ngt_frame, ref['ngt_frame'])
    assert all(np.array_equal(a, b) for a, b in zip(runs[0][0], runs[1][0]))
    lab, n_valid = _sorted_labels(ref, len(label))
    curves = [_raw_curve(dev, lab, n_valid, ngt_frame) for _ in range(2)]
    out, ngt, intact = curves[0]
    assert intact and np.array_equal(ngt, ref['ngt'])
    for r, key in enumerate(('ap', 'pre', 'rec')):
        print(key, ' '.join('%.6f' % v for v in out[r]), '| off by %.3e' % np.nanmax(np.abs(out[r] - ref[key])))
        assert _close(out[r], ref[key]), key
    assert np.array_equal(out.view(np.int64), curves[1][0].view(np.int64))
    # the front door: the same numbers bit for bit, through one buffer and torch's stable sort
    res = ev.posetrack_ap(packed, device=dev)
    for key in ('pr_has', 'gt_has', 'label', 'assigned', 'ngt'):
        assert res[key].dtype == np.int32 and np.array_equal(res[key], ref[key]), key
    for r, key in enumerate(('ap', 'pre', 'rec')):
        assert res[key].dtype == np.float64 and np.array_equal(res[key].view(np.int64), out[r].view(np.int64)), key
    assert res['names'] == ar.NAMES + ['total'] and np.allclose(res['cum'], ref['cum'], rtol=0, atol=TOL, equal_nan=True)
    if name == 'fixture':                                          # ... and against the reference's own numbers
        want = ar.load_fixture(GOLD)[1]
        for key, w in zip(('ap', 'pre', 'rec'), want):
            assert _close(res[key], w), key


def test_another_threshold(dev):
    gt, pr, _, packed = _family('fixture')
    ref = ar.evaluate_ap(gt, pr, thresh=0.2)
    assert ref['margin'] >= MARGIN and not np.array_equal(ref['label'], _family('fixture')[2]['label'])
    res = ev.posetrack_ap(packed, dist_thresh=0.2, device=dev)
    assert np.array_equal(res['label'], ref['label']) and np.array_equal(res['assigned'], ref['assigned'])
    assert all(_close(res[k], ref[k]) for k in ('ap', 'pre', 'rec'))


# ---------------------------------------------------------------------------------------- 2. the curve kernel's lengths
LENGTHS = (0, 1, 63, 64, 65, 193, 255, 257, 16383, 16384, 16385, 49153, 49153, 49152, 256)


def test_curve_lengths(dev):
    """One launch, 15 joints with lists of LENGTHS labels in rows of 49153: around the 64-label word, around the 256 words
    after which a thread owns a second one, three such rounds + 1.  Joint 12 has the full length and no annotation (NaN)."""
    rng = np.random.RandomState(2)
    P = max(LENGTHS)
    lab = (rng.uniform(0, 1, (J, P)) < 0.15).astype(np.uint8)      # garbage behind n_valid[j] too: it must not be read as labels
    lab[12] = 0
    n_valid = np.array(LENGTHS, np.int32)
    pos = np.array([int(lab[j, :n].sum()) for j, n in enumerate(LENGTHS)])
    ngt = pos + np.array([5, 0, 3, 0, 7, 1, 0, 2, 9, 0, 4, 6, 0, 8, 1])
    ngt[0] = 4
    ngt_frame = np.stack([ngt // 3, ngt // 3, ngt - 2 * (ngt // 3)]).astype(np.int32)
    assert ngt[12] == 0 and pos.max() <= MAX_TERMS and (pos[[8, 9, 10, 11, 13]] > 2000).all()
    want = np.zeros((3, 16))
    for j, n in enumerate(LENGTHS):
        want[:, j] = ar.curve(-np.arange(n, dtype=np.float64), lab[j, :n], ngt[j])[:3]
    for r in range(3):
        want[r, 15] = np.nanmean(want[r, :15])
    runs = [_raw_curve(dev, lab, n_valid, ngt_frame) for _ in range(2)]
    out, got_ngt, intact = runs[0]
    assert intact and np.array_equal(got_ngt, ngt)
    for r, key in enumerate(('ap', 'pre', 'rec')):
        print(key, ' '.join('%.6f' % v for v in out[r]), '| off by %.3e' % np.nanmax(np.abs(out[r] - want[r])))
        assert _close(out[r], want[r]), key
    assert np.isnan(out[0, 12]) and np.isnan(out[2, 12]) and out[1, 12] == 0.0 and not out[:, 0].any()
    assert np.array_equal(out.view(np.int64), runs[1][0].view(np.int64))


# ---------------------------------------------------------------------------------------- 3. what the Python layer refuses
def test_unchecked_segments_never_write_outside_the_outputs(dev):
    """Through the raw entry point: a frame over the prediction cap and a frame whose segment is no sub-range of the
    arrays are marked ngt_frame = -1 and nothing else of theirs is written; their neighbours come out as if alone."""
    gt, pr, ref, packed = _family('fixture')
    k = {n: v.copy() for n, v in packed.items()}
    F = len(k['pr_seg']) - 1
    k['gt_seg'][F] = len(k['gt_has']) + 7                          # the last frame reaches past the annotated poses
    (pr_has, gt_has, label, assigned, ngt_frame), intact = _raw_assign(dev, k)
    assert intact and (ngt_frame[F - 1] == -1).all() and np.array_equal(ngt_frame[:F - 1], ref['ngt_frame'][:F - 1])
    s = packed['pr_seg'][F - 1]
    assert np.array_equal(label[:s], ref['label'][:s]) and (label[s:] == SENT).all() and (assigned[s:] == SENT).all()
    with pytest.raises(RuntimeError, match='refused'):
        ev.posetrack_ap(k, device=dev)
    big = ev.pack_posetrack_frames(*_family('shapes')[:2])
    big['pr_seg'] = np.array([0, 300, len(big['pr_has'])], np.int32)     # two frames, the first over the cap
    big['gt_seg'] = np.array([0, 3, len(big['gt_has'])], np.int32)
    big['poly_seg'] = np.zeros(3, np.int32)
    with pytest.raises(ValueError, match='300 predicted'):
        ev.posetrack_ap(big, device=dev)
    (pr_has, gt_has, label, assigned, ngt_frame), intact = _raw_assign(dev, big)
    assert intact and (ngt_frame[0] == -1).all() and (label[:300] == SENT).all() and (pr_has[:300] == SENT).all()
    assert (ngt_frame[1] == -1).all()                              # ... and so is the second: more than 64 annotated poses


# ---------------------------------------------------------------------------------------- 4. the front door
COCO = ev.COCO_JOINT


def test_round_trip_through_the_writer(dev, tmp_path):
    """Two videos of three frames: predictions go through the unchanged write_posetrack_results, and
    evaluate_posetrack_ap reads that directory against annolist ground truth -- the restatement on the same files agrees."""
    rng = np.random.RandomState(4)
    annot, names, rows = tmp_path / 'annot', [], []
    annot.mkdir()
    direct = [(k, COCO.index(n)) for k, n in enumerate(ev.POSETRACK_JOINT) if n in COCO]
    for vid in ('000001_bonn', '000002_bonn'):
        frames = []
        for fnum in (1, 2, 3):
            name = 'images/bonn/%s/%08d.jpg' % (vid, fnum)
            rects = []
            for i in range(2 if fnum != 2 else 0):                # frame 2 is not annotated: dropped by the selection
                xy, present, head, size = ar.make_person(rng)
                rects.append(ar.gt_rect(xy, present, head, i))
                coco = np.zeros((17, 3))
                coco[:, :2] = xy.mean(0) + rng.normal(0, 40, (17, 2))
                for k, c in direct:
                    coco[c, :2] = xy[k] + rng.normal(0, 0.3 * size, 2)
                coco[:, 2] = rng.uniform(0.3, 1.0, 17)
                if fnum == 1 or i == 0:                            # one person of frame 3 is missed
                    names.append('/data/' + name)
                    rows.append(coco)
            frames.append({'image': [{'name': name}], 'imgnum': [fnum], 'annorect': rects})
        (annot / (vid + '.json')).write_text(json.dumps({'annolist': frames}))
    preds = np.array(rows)
    boxes = np.zeros((len(rows), 6))
    boxes[:, 5] = rng.uniform(0.5, 1.0, len(rows))
    fmap = {}
    for i, nm in enumerate(names):
        fmap.setdefault(nm, []).append(i)
    written = ev.write_posetrack_results(preds, boxes, fmap, str(annot), str(tmp_path / 'out'))
    pred_dir = os.path.dirname(next(iter(written)))
    assert len(written) == 2
    g, p = ev.load_posetrack_dirs(str(annot), pred_dir)
    ref = ar.evaluate_ap(g, p)
    assert ref['margin'] >= MARGIN and len(ref['frame_index']) == 4 and 0.0 < ref['cum'][7] < 100.0
    cum = ev.evaluate_posetrack_ap(str(annot), pred_dir, device=dev)
    assert len(cum) == 8 and np.allclose(cum, ref['cum'], rtol=0, atol=TOL)
