"""The input families of tests/test_posetrack_mota_gpu.py, stated once so that tests/test_posetrack_mota_host.py can hold
the margin condition against every one of them on the CPU: family(name) -> (gt, pr, seq_ids, restatement), computed once
per process and not modified by anybody.

  fixture   tests/golden/posetrack_mota.npz (what the reference computed; tools/gen_mota_golden.py)
  seeded    six seeded sequences of 1 .. 30 frames (tests/_mota_ref.make_sequences)
  cases     one hand-made sequence per decision of the update rule, every joint alike (CASES says what each must count);
            no annotated pose has joint MISS_GT and no predicted pose joint MISS_PR
  quirks    the dummy lists (a frame without predictions, a frame whose annotated rects have no pose), the dropped last
            frame, a sequence of one frame, a sequence of none
  polygons  ignore regions: filtered points leave the lists, an emptied rect is no rect
  caps      one frame of 64 annotated x 256 predicted poses with all 15 joints, 65 / 64 / 63 predictions beside it, 256
            annotated tracks in the sequence, and a frame in which 64 objects remember a hypothesis

Geometry of the hand-made ones: a pose is a row of joints 40 px apart, joint j at centre + (40 j, 0); a prediction is
the same row elsewhere, so every joint sees the same distances.  The head rectangle is 30 x 40: head size 30, and
dist <= 0.5 is 15 px."""
import os
import sys

import numpy as np
from scipy.optimize import linear_sum_assignment

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ap_ref as ar  # noqa: E402
import _mota_ref as mr  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'posetrack_mota.npz')
J = ar.J
MISS_PR, MISS_GT = 7, 3
HEAD = np.array([0.0, 0.0, 30.0, 40.0])
ROW = np.stack([40.0 * np.arange(J), np.zeros(J)], axis=1)
ALL = np.ones(J, bool)
SEED_5X5 = 0                                                      # the first seed of five_by_five with the property
CONCAVE = np.array([(0, 0), (100, 0), (100, 100), (50, 20), (0, 100)], dtype=np.float64)


def _gt(track, x, y=0.0, present=ALL):
    return ar.gt_rect(ROW + np.array([x, y], dtype=np.float64), present, HEAD, track)


def _pr(track, x, y=0.0, present=ALL):
    return ar.pr_rect(ROW + np.array([x, y], dtype=np.float64), present, np.full(J, 0.5), track)


def _sequence(frames, present_gt=ALL, present_pr=ALL):
    """frames: [([(track, x[, y])], [(track, x[, y])])] -> (gt annolist, pr annolist)."""
    gt = [{'annorect': [_gt(t[0], *t[1:], present=present_gt) for t in g]} for g, _ in frames]
    pr = [{'annorect': [_pr(t[0], *t[1:], present=present_pr) for t in p]} for _, p in frames]
    return gt, pr


LAST = ([(7, 0.0)], [(1, 2.0), (2, 300.0)])                       # every sequence ends with a frame that must not count

# name -> (frames, what every joint that both sides have must count: misses, switches, fps, detections, objects)
CASES = {
    # the remembered hypothesis is still valid (10 px) and wins over a nearer one (1 px): MATCH, the nearer one is an FP
    'carry_forward': ([([(7, 0.0)], [(1, 3.0)]), ([(7, 0.0)], [(2, 1.0), (1, 10.0)]), LAST], (0, 0, 1, 2, 2)),
    # remembered but invalid (20 px): SWITCH; remembered but absent: SWITCH; nobody valid: MISS + FP; back after the gap
    # to the one remembered last: MATCH
    'switch': ([([(7, 0.0)], [(1, 3.0)]), ([(7, 0.0)], [(1, 20.0), (2, 2.0)]), ([(7, 0.0)], [(3, 4.0)]),
                ([(7, 0.0)], [(9, 100.0)]), ([(7, 0.0)], [(3, 5.0)]), LAST], (1, 2, 2, 4, 5)),
    # two objects remember hypothesis 1: the first in the list keeps it, the second switches to hypothesis 2
    'shared_memory': ([([(7, 0.0)], [(1, 3.0)]), ([(8, 8.0)], [(1, 6.0)]), ([(7, 0.0), (8, 8.0)], [(2, 9.0), (1, 4.0)]),
                       LAST], (0, 1, 0, 4, 4)),
    # nearest first would pair 7 with hypothesis 1 (5 px) and leave 8 alone; the minimum is 7-2 (9 px) and 8-1 (7 px)
    'not_greedy_2x2': ([([(7, 0.0), (8, 12.0)], [(1, 5.0), (2, -9.0)]), LAST], (0, 0, 0, 2, 2)),
    # rows 7 and 8 take hypotheses 2 and 3 first; row 9 can only have 3: the augmenting path moves both of them
    'augment_3x3': ([([(7, 0.0), (8, 10.0), (9, 20.0)], [(1, -12.0), (2, 4.0), (3, 14.0)]), LAST], (0, 0, 0, 3, 3)),
}


def five_by_five(seed):
    """A 5 x 5 frame on a line, seeded: object 4, then four (object, hypothesis) pairs a pixel apart, then hypothesis 4,
    about 13.5 px from one to the next.  Shifting every object to its right-hand neighbour pairs all five (about 0.45
    each); the four cheap pairs and one INV cost less.  -> (objects, hypotheses) as _sequence takes them."""
    rng = np.random.RandomState(seed)
    step = 13.5 + rng.uniform(-1.0, 1.0, 6)
    x = np.concatenate([[0.0], np.cumsum(step)])
    objs = [(10 + i, float(x[i + 1]), float(rng.uniform(-1, 1))) for i in range(4)] + [(14, float(x[0]), 0.0)]
    hyps = [(20 + i, float(x[i + 1] + rng.uniform(0.3, 1.0)), float(rng.uniform(-1, 1))) for i in range(4)] + \
           [(24, float(x[5]), 0.0)]
    return objs, hyps


def fewer_pairs_than_matching(objs, hyps, thresh=0.5):
    """-> (valid pairs of the minimum-cost solution, size of the largest matching of valid pairs) by the restatement."""
    gt, pr = _sequence([(objs, hyps)])
    fr = ar.select_frames(gt, pr)[0]
    oids, hids, dist = mr.frame_lists(fr, gt[0], pr[0], thresh)[0][0]
    valid = np.isfinite(dist)
    r, c = linear_sum_assignment(-valid.astype(np.float64))
    n_match, n_switch = mr.update({}, oids, hids, dist)[:2]
    return n_match + n_switch, int(valid[r, c].sum())


def _cases_family():
    no_gt, no_pr = ALL.copy(), ALL.copy()
    no_gt[MISS_GT], no_pr[MISS_PR] = False, False
    gt, pr, seq = [], [], []
    scenes = [v[0] for v in CASES.values()] + [[five_by_five(SEED_5X5), LAST]]
    for s, frames in enumerate(scenes):
        g, p = _sequence(frames, no_gt, no_pr)
        gt, pr, seq = gt + g, pr + p, seq + ['case%d' % s] * len(g)
    return gt, pr, seq


def _quirks_family():
    bare = _gt(5, 0.0)
    bare['annopoints'] = []
    seqs = [
        # two annotated poses and no prediction: ONE miss, one FP, one object; then a real frame; then the dropped one
        [{'annorect': [_gt(7, 0.0), _gt(8, 100.0)]}, {'annorect': [_gt(7, 0.0)]}, {'annorect': [_gt(7, 0.0)]}],
        # no annotated pose left (a rect without a point list) and two predictions: the same dummy lists
        [{'annorect': [bare]}, {'annorect': [_gt(7, 0.0)]}, {'annorect': [_gt(7, 0.0)]}],
        [{'annorect': [_gt(7, 0.0)]}],                            # one frame: nothing
        [{'annorect': []}, {'annorect': []}],                     # no kept frame: nothing
        [{'annorect': [_gt(7, 0.0)]}, {'annorect': []}, {'annorect': [_gt(7, 0.0)]}],   # the unannotated frame is no frame
    ]
    preds = [
        [{'annorect': []}, {'annorect': [_pr(1, 2.0)]}, {'annorect': [_pr(1, 2.0), _pr(2, 9.0)]}],
        [{'annorect': [_pr(1, 2.0), _pr(2, 50.0)]}, {'annorect': [_pr(1, 2.0)]}, {'annorect': [_pr(3, 2.0)]}],
        [{'annorect': [_pr(1, 2.0)]}],
        [{'annorect': [_pr(1, 2.0)]}, {'annorect': []}],
        [{'annorect': [_pr(1, 2.0)]}, {'annorect': [_pr(2, 2.0)]}, {'annorect': [_pr(2, 2.0)]}],
    ]
    gt = [f for s in seqs for f in s]
    pr = [f for s in preds for f in s]
    seq = [i for i, s in enumerate(seqs) for _ in s]
    return gt, pr, seq


def _region(poly):
    return {'point': [{'x': [float(x)], 'y': [float(y)]} for x, y in poly]}


def _polygon_family():
    """The polygon covers x in 300 .. 600 at y = 320: joints 2 .. 8 of a row that starts at (250, 320) are inside (30 px
    or more from an edge), joints 0, 1 and 9 .. 14 outside (10 px or more)."""
    q = CONCAVE * 3.0 + 300.0
    reg = [_region(q)]
    lone = np.zeros(J, bool)
    lone[2] = True
    gt = [
        {'annorect': [_gt(7, 250.0, 320.0), _gt(8, 250.0, 700.0)], 'ignore_regions': reg},
        # the lone joint of pose 9 is inside: the rect is emptied, and it is no object of any joint
        {'annorect': [_gt(7, 250.0, 320.0), _gt(9, 256.0, 326.0, lone)], 'ignore_regions': reg},
        # the same points without a region of this frame: nothing is filtered (pose 9 stands 6 px off pose 7, so that
        # the assignment of joint 2 -- two objects, two hypotheses -- has one optimum)
        {'annorect': [_gt(7, 250.0, 320.0), _gt(9, 256.0, 326.0, lone)]},
        # the only annotated rect is emptied: no annotated rect, the dummy lists
        {'annorect': [_gt(9, 256.0, 326.0, lone)], 'ignore_regions': reg},
        # the only predicted rect is emptied: no predicted rect, the dummy lists
        {'annorect': [_gt(7, 250.0, 700.0)], 'ignore_regions': reg},
        {'annorect': [_gt(7, 250.0, 320.0)]},
    ]
    pr = [
        {'annorect': [_pr(1, 252.0, 321.0), _pr(2, 251.0, 702.0)]},
        {'annorect': [_pr(1, 252.0, 321.0), _pr(3, 253.0, 322.0, lone)]},
        {'annorect': [_pr(1, 252.0, 321.0), _pr(3, 253.0, 322.0, lone)]},
        {'annorect': [_pr(1, 252.0, 321.0)]},
        {'annorect': [_pr(3, 253.0, 322.0, lone)]},
        {'annorect': [_pr(1, 252.0, 321.0)]},
    ]
    return gt, pr, [0] * len(gt)


def _caps_family():
    rng = np.random.RandomState(21)
    gt, pr = [], []
    crowds = [[ar.make_person(rng, 1.0) for _ in range(64)] for _ in range(4)]

    def frame(crowd, first_id, n_pred, pred_id):
        g = [ar.gt_rect(xy, ALL, head, first_id + i) for i, (xy, _, head, _) in enumerate(crowd)]
        p = []
        for k in range(n_pred):
            xy, _, _, size = crowd[k % 64]
            noisy, _, score = ar.make_prediction(rng, xy, size, rng.uniform(0.05, 0.45), 1.0)
            p.append(ar.pr_rect(noisy, ALL, score, pred_id(k)))
        return {'annorect': g}, {'annorect': [p[i] for i in rng.permutation(n_pred)]}

    for c, n_pred in enumerate((256, 65, 64, 63)):
        g, p = frame(crowds[c], 64 * c, n_pred, lambda k, c=c: 1000 * c + k)
        gt.append(g)
        pr.append(p)
    # the first crowd again: predictions 0 .. 63 keep the ids of frame 0 except that neighbours 2 i, 2 i + 1 with i < 8
    # have exchanged them; 64 more carry new ids
    swap = lambda k: (k ^ 1 if k < 16 else k) if k < 64 else 5000 + k  # noqa: E731
    g, p = frame(crowds[0], 0, 128, swap)
    gt.append(g)
    pr.append(p)
    g, p = frame(crowds[1], 64, 3, lambda k: k)                   # the dropped last frame
    gt.append(g)
    pr.append(p)
    return gt, pr, [0] * len(gt)


_FAMILIES = {}
NAMES = ('fixture', 'seeded', 'cases', 'quirks', 'polygons', 'caps')


def family(name):
    if name not in _FAMILIES:
        if name == 'fixture':
            gt, pr, seq = mr.unpack(mr.load_fixture(GOLD)[0])
        elif name == 'seeded':
            gt, pr, seq = mr.make_sequences(np.random.RandomState(12), 6, (30, 17, 1, 9, 2, 24))
        else:
            gt, pr, seq = {'cases': _cases_family, 'quirks': _quirks_family, 'polygons': _polygon_family,
                           'caps': _caps_family}[name]()
        _FAMILIES[name] = (gt, pr, seq, mr.evaluate_mota(gt, pr, seq))
    return _FAMILIES[name]
