"""Float64 numpy restatement of the PoseTrack AP the reference vendors (poseval/py/eval_helpers.py: cleanupData :305-319,
removeIgnoredPoints :322-367, assignGTmulti :453-668, computeRPC / VOCap :192-228; evaluateAP.py:8-47 computeMetrics): the
yardstick of tests/test_posetrack_ap_host.py and tests/test_posetrack_ap_gpu.py, and what tools/gen_ap_golden.py holds
against the reference's own evaluateAP before it writes tests/golden/posetrack_ap.npz.  It does not import the package.

One function per stage:
  select_frames  frame selection, in the reference's order: frames without annotated rects go (with their predictions),
                 rects without a point list go, points inside an ignore region go (even-odd rule; shapely in the
                 reference), rects that lose all points go.  Every surviving rect remembers its `slot`: its position
                 among the frame's rects that had a point list, which is how the packed arrays of
                 evaluate.pack_posetrack_frames count them.
  match_frame    the greedy PCKh matching of one frame; also the smallest decision margin
                 min |dist - thresh| / thresh over all finite distances, and which of the competition cases occurred.
  curve          one joint's precision / recall curve and VOC AP; the AP sum is math.fsum: exact up to one rounding.
  evaluate_ap    all of it -> ap / pre / rec [16] and the per-pose arrays in packed order.
Equal scores keep frame order, then pose order (a stable descending sort) -- ours; the reference leaves them open.

Seeded generators of annolists: make_annolists (noise scaled to the head size, scores falling with the noise level, so
that the curves are not flat)."""
import math

import numpy as np

J = 15
MIN_SCORE = -9999
NAMES = ['right_ankle', 'right_knee', 'right_hip', 'left_hip', 'left_knee', 'left_ankle', 'right_wrist', 'right_elbow',
         'right_shoulder', 'left_shoulder', 'left_elbow', 'left_wrist', 'neck', 'nose', 'head_top']


# ---------------------------------------------------------------------------------------- stage 1: frame selection
def point_in_polygon(x, y, poly):
    """Even-odd crossing rule, fp64; poly [n,2].  The expression of csrc/posetrack_ap.hip, operation for operation."""
    inside = False
    n = len(poly)
    j = n - 1
    for i in range(n):
        xi, yi = float(poly[i][0]), float(poly[i][1])
        xj, yj = float(poly[j][0]), float(poly[j][1])
        if (yi > y) != (yj > y):
            if x < (xj - xi) * (y - yi) / (yj - yi) + xi:
                inside = not inside
        j = i
    return inside


def _rect_has_points(rect):
    a = rect.get('annopoints')
    return a is not None and len(a) > 0 and len(a[0]) > 0 and 'point' in a[0]


def _pose(points, with_score):
    xy, sc, has = np.zeros((J, 2)), np.full(J, np.nan), np.zeros(J, bool)
    for j in range(J):
        for pt in points:                                     # getPointGTbyID: the first with that id
            if pt['id'] is not None and pt['id'][0] == j:
                xy[j] = (pt['x'][0], pt['y'][0])
                sc[j] = pt['score'][0] if (with_score and 'score' in pt) else MIN_SCORE
                has[j] = True
                break
    return xy, sc, has


def select_frames(gt_annolists, pr_annolists):
    """-> list of frames {'idx', 'polys': [[n,2]], 'n_gt_packed', 'n_pr_packed', 'gt': [{'slot', 'xy', 'has', 'head'}],
    'pr': [{'slot', 'xy', 'score', 'has'}]}.  The inputs are not modified."""
    assert len(gt_annolists) == len(pr_annolists)
    frames = []
    for idx, (gf, pf) in enumerate(zip(gt_annolists, pr_annolists)):
        if len(gf['annorect']) == 0:
            continue
        polys = [np.array([[p['x'][0], p['y'][0]] for p in reg['point']], dtype=np.float64)
                 for reg in (gf.get('ignore_regions') or [])]
        out = {'idx': idx, 'polys': polys}
        for key, src, with_score in (('gt', gf, False), ('pr', pf, True)):
            rects = [r for r in src['annorect'] if _rect_has_points(r)]
            out['n_%s_packed' % key] = len(rects)
            poses = []
            for slot, r in enumerate(rects):
                points = r['annopoints'][0]['point']
                if polys:
                    points = [pt for pt in points
                              if not any(point_in_polygon(float(pt['x'][0]), float(pt['y'][0]), q) for q in polys)]
                    if not points:
                        continue
                xy, sc, has = _pose(points, with_score)
                pose = {'slot': slot, 'xy': xy, 'has': has}
                if with_score:
                    pose['score'] = sc
                else:
                    pose['head'] = np.array([r[k][0] for k in ('x1', 'y1', 'x2', 'y2')], dtype=np.float64)
                poses.append(pose)
            out[key] = poses
        frames.append(out)
    return frames


# ---------------------------------------------------------------------------------------- stage 2: matching
def match_frame(frame, thresh=0.5):
    """-> {'label' [np,15] bool, 'assigned' [np] (index into frame['gt'], -1), 'ngt' [15], 'margin',
    'outcompeted' (predictions within the threshold of some joint of their best pose that another prediction took),
    'unmatched_gt' (annotated poses nobody matched)}."""
    pr, gt = frame['pr'], frame['gt']
    n_p, n_g = len(pr), len(gt)
    has_pr = np.array([p['has'] for p in pr], dtype=bool).reshape(n_p, J)
    has_gt = np.array([g['has'] for g in gt], dtype=bool).reshape(n_g, J)
    label = np.zeros((n_p, J), bool)
    assigned = np.full(n_p, -1, np.int64)
    res = {'label': label, 'assigned': assigned, 'ngt': has_gt.sum(0).astype(np.int64), 'margin': np.inf, 'outcompeted': 0,
           'unmatched_gt': 0}
    if n_p == 0 or n_g == 0:
        res['unmatched_gt'] = n_g
        return res
    xy_pr = np.array([p['xy'] for p in pr])
    xy_gt = np.array([g['xy'] for g in gt])
    heads = np.array([g['head'] for g in gt])
    hx, hy = heads[:, 2] - heads[:, 0], heads[:, 3] - heads[:, 1]
    head = 0.6 * np.sqrt(hx * hx + hy * hy)
    dx = xy_gt[None, :, :, 0] - xy_pr[:, None, :, 0]
    dy = xy_gt[None, :, :, 1] - xy_pr[:, None, :, 1]
    with np.errstate(divide='ignore', invalid='ignore'):
        d = np.sqrt(dx * dx + dy * dy) / head[None, :, None]
    both = has_pr[:, None, :] & has_gt[None, :, :]
    dist = np.where(both, d, np.inf)
    fin = np.isfinite(dist)
    if fin.any():
        res['margin'] = float(np.min(np.abs(dist[fin] - thresh) / thresh))
    with np.errstate(invalid='ignore'):
        match = dist <= thresh
    pck = match.sum(2).astype(np.float64)
    n_gtp = has_gt.sum(1)
    pck[:, n_gtp > 0] /= n_gtp[n_gtp > 0]
    idx = np.argmax(pck, axis=1)                              # every p keeps its best g, the first on ties
    best = pck[np.arange(n_p), idx].copy()
    only = np.zeros_like(pck)
    only[np.arange(n_p), idx] = best
    pr_to_gt = np.argmax(only, axis=0)                        # every g takes its best remaining p, the first on ties
    pr_to_gt[only.max(axis=0) == 0] = -1
    for g, p in enumerate(pr_to_gt):
        if p >= 0:
            assigned[p] = g
            label[p] = match[p, g]
    res['outcompeted'] = int(((best > 0) & (assigned < 0)).sum())
    res['unmatched_gt'] = int((pr_to_gt < 0).sum())
    return res


# ---------------------------------------------------------------------------------------- stage 3: the curve
def curve(scores, labels, ngt):
    """scores [n], labels [n] (0 / 1), in frame-then-pose order; ngt: the number of annotated joints.
    -> (ap, pre, rec) x 100 and the number of terms of the AP sum.  n = 0 gives zeros."""
    scores, labels = np.asarray(scores, dtype=np.float64), np.asarray(labels).astype(np.int64)
    n = len(scores)
    if n == 0:
        return 0.0, 0.0, 0.0, 0
    order = np.argsort(-scores, kind='stable')
    npos = np.cumsum(labels[order]).astype(np.float64)
    prec = npos / np.arange(1, n + 1, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        rec = npos / np.float64(ngt)
    mpre = np.concatenate([[0.0], prec, [0.0]])
    mrec = np.concatenate([[0.0], rec, [1.0]])
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]
    i = np.flatnonzero(~np.equal(mrec[1:], mrec[:-1])) + 1
    terms = (mrec[i] - mrec[i - 1]) * mpre[i]
    ap = math.fsum(terms) if np.isfinite(terms).all() else float(np.sum(terms))
    return ap * 100.0, float(prec[-1]) * 100.0, float(rec[-1]) * 100.0, len(terms)


def metrics(scores, labels, ngt):
    """scores / labels: per joint, the arrays of `curve`; ngt [15] -> ap, pre, rec [16] with the NaN-aware mean."""
    out = np.zeros((3, J + 1))
    for j in range(J):
        out[:, j] = curve(scores[j], labels[j], ngt[j])[:3]
    for r in range(3):
        ok = ~np.isnan(out[r, :J])
        out[r, J] = out[r, :J][ok].mean() if ok.any() else np.nan
    return out[0], out[1], out[2]


def get_cum(vals):
    groups = ((14, 12, 13), (8, 9), (7, 10), (6, 11), (2, 3), (1, 4), (0, 5))
    return [float(np.asarray(vals)[list(g)].mean()) for g in groups] + [float(vals[J])]


def _mask(bits):
    return int(sum(1 << j for j in range(J) if bits[j]))


def evaluate_ap(gt_annolists, pr_annolists, thresh=0.5):
    """-> dict: ap / pre / rec [16], cum [8], and in the packed order of evaluate.pack_posetrack_frames: pr_has / gt_has
    (masks after the ignore filter; 0 for a removed rect), label, assigned (packed frame-local index of the annotated
    pose, -1), ngt [15], ngt_frame [F,15]; margin, outcompeted, unmatched_gt, empty_gt_frames (frames with predictions and
    no annotated pose left), frame_index, scores / labels (per joint lists) and terms (the longest AP sum)."""
    frames = select_frames(gt_annolists, pr_annolists)
    scores, labels = [[] for _ in range(J)], [[] for _ in range(J)]
    pr_has, gt_has, label, assigned, ngt_frame = [], [], [], [], []
    res = {'margin': np.inf, 'outcompeted': 0, 'unmatched_gt': 0, 'empty_gt_frames': 0}
    for fr in frames:
        m = match_frame(fr, thresh)
        res['margin'] = min(res['margin'], m['margin'])
        res['outcompeted'] += m['outcompeted']
        res['unmatched_gt'] += m['unmatched_gt']
        res['empty_gt_frames'] += int(len(fr['pr']) > 0 and len(fr['gt']) == 0)
        ph, lb, asg = [0] * fr['n_pr_packed'], [0] * fr['n_pr_packed'], [-1] * fr['n_pr_packed']
        gh = [0] * fr['n_gt_packed']
        for g in fr['gt']:
            gh[g['slot']] = _mask(g['has'])
        for i, p in enumerate(fr['pr']):
            ph[p['slot']] = _mask(p['has'])
            lb[p['slot']] = _mask(m['label'][i])
            asg[p['slot']] = fr['gt'][m['assigned'][i]]['slot'] if m['assigned'][i] >= 0 else -1
            for j in range(J):
                if p['has'][j]:
                    scores[j].append(p['score'][j])
                    labels[j].append(int(m['label'][i, j]))
        pr_has += ph
        gt_has += gh
        label += lb
        assigned += asg
        ngt_frame.append(m['ngt'])
    ngt_frame = np.array(ngt_frame, dtype=np.int64).reshape(len(frames), J)
    ngt = ngt_frame.sum(0)
    ap, pre, rec = metrics(scores, labels, ngt)
    res.update({'ap': ap, 'pre': pre, 'rec': rec, 'cum': get_cum(ap), 'pr_has': np.array(pr_has, np.int32),
                'gt_has': np.array(gt_has, np.int32), 'label': np.array(label, np.int32),
                'assigned': np.array(assigned, np.int32), 'ngt': ngt.astype(np.int32), 'ngt_frame': ngt_frame.astype(np.int32),
                'frame_index': np.array([fr['idx'] for fr in frames], np.int64), 'scores': scores, 'labels': labels,
                'terms': max([curve(scores[j], labels[j], ngt[j])[3] for j in range(J)] + [0])})
    return res


# ---------------------------------------------------------------------------------------- seeded annolists
def _points(xy, present, score=None):
    pts = []
    for j in range(J):
        if present[j]:
            pt = {'id': [j], 'x': [float(xy[j, 0])], 'y': [float(xy[j, 1])]}
            if score is not None:
                pt['score'] = [float(score[j])]
            pts.append(pt)
    return pts


def _snap(a, grid):
    return a if grid is None else np.round(np.asarray(a) / grid) * grid


def make_person(rng, p_joint=0.85, grid=None):
    """-> (xy [15,2], present [15], head [4], head size).  grid: coordinates snapped to its multiples (a fixture of such
    values compresses; the arithmetic on them is as generic as on any other doubles)."""
    c = rng.uniform(100, 900, 2)
    xy = _snap(c + rng.normal(0, 80, (J, 2)), grid)
    h = rng.uniform(20, 60)
    x1, y1 = c + rng.uniform(-10, 10, 2)
    head = _snap(np.array([x1, y1, x1 + 0.8 * h, y1 + h]), grid)
    size = 0.6 * math.sqrt((head[2] - head[0]) ** 2 + (head[3] - head[1]) ** 2)
    return xy, rng.uniform(0, 1, J) < p_joint, head, size


def gt_rect(xy, present, head, track_id=0):
    return {'x1': [float(head[0])], 'y1': [float(head[1])], 'x2': [float(head[2])], 'y2': [float(head[3])],
            'track_id': [int(track_id)], 'annopoints': [{'point': _points(xy, present)}]}


def pr_rect(xy, present, score, track_id=0):
    return {'score': [float(np.mean(score))], 'track_id': [int(track_id)],
            'annopoints': [{'point': _points(xy, present, score)}]}


def make_prediction(rng, xy, size, level, p_joint=0.9, grid=None):
    """A prediction of the pose xy: noise of `level` head sizes, scores falling with the level."""
    noisy = _snap(xy + rng.normal(0, level * size, (J, 2)), grid)
    score = _snap(math.exp(-1.5 * level) * rng.uniform(0.7, 1.0, J), None if grid is None else 2.0 ** -24)
    return noisy, rng.uniform(0, 1, J) < p_joint, score


def make_annolists(rng, n_frames, max_people=4, p_detect=0.85, p_twin=0.3, p_false=0.3, p_bare=0.05, levels=(0.05, 0.9),
                   grid=None):
    """-> (gt_annolist, pr_annolist) of n_frames frames: 0 .. max_people annotated people (a frame of 0 is dropped by the
    selection), a few annotated rects without a point list (p_bare; a frame may lose all its poses that way), one
    prediction per person with p_detect, a second one of the same person with p_twin (the competition case), false
    positives with p_false.  Every rect carries a track_id."""
    gt, pr = [], []
    for f in range(n_frames):
        g_rects, p_rects = [], []
        for i in range(rng.randint(0, max_people + 1)):
            xy, present, head, size = make_person(rng, grid=grid)
            if rng.uniform() < p_bare:
                r = gt_rect(xy, present, head, i)
                r['annopoints'] = []
                g_rects.append(r)
            else:
                g_rects.append(gt_rect(xy, present, head, i))
            if rng.uniform() < p_detect:
                for _ in range(1 + int(rng.uniform() < p_twin)):
                    p_rects.append(pr_rect(*make_prediction(rng, xy, size, rng.uniform(*levels), grid=grid), track_id=len(p_rects)))
        if rng.uniform() < p_false:
            xy, present, head, size = make_person(rng, grid=grid)
            p_rects.append(pr_rect(*make_prediction(rng, xy, size, rng.uniform(0.5, 1.5), grid=grid), track_id=len(p_rects)))
        order = rng.permutation(len(p_rects))
        name = 'images/seq/%08d.jpg' % (f + 1)
        gt.append({'image': [{'name': name}], 'imgnum': [f + 1], 'annorect': g_rects})
        pr.append({'image': [{'name': name}], 'imgnum': [f + 1], 'annorect': [p_rects[i] for i in order]})
    return gt, pr


def unpack(packed):
    """The packed arrays of evaluate.pack_posetrack_frames (no polygons) -> (gt_annolist, pr_annolist) of the kept frames;
    a frame without an annotated pose gets one rect without a point list, which is how it lost them."""
    gt, pr = [], []
    bits = lambda m: [(int(m) >> j) & 1 for j in range(J)]  # noqa: E731
    for f in range(len(packed['pr_seg']) - 1):
        g_rects = [gt_rect(packed['gt_xy'][g], bits(packed['gt_has'][g]), packed['gt_head'][g], g)
                   for g in range(int(packed['gt_seg'][f]), int(packed['gt_seg'][f + 1]))]
        if not g_rects:
            g_rects = [{'x1': [0.0], 'y1': [0.0], 'x2': [1.0], 'y2': [1.0], 'track_id': [0], 'annopoints': []}]
        p_rects = [pr_rect(packed['pr_xys'][p, :, :2], bits(packed['pr_has'][p]), packed['pr_xys'][p, :, 2], p)
                   for p in range(int(packed['pr_seg'][f]), int(packed['pr_seg'][f + 1]))]
        gt.append({'annorect': g_rects})
        pr.append({'annorect': p_rects})
    return gt, pr


def load_fixture(path):
    """tests/golden/posetrack_ap.npz -> (packed dict as evaluate.pack_posetrack_frames returns it: fp64, no polygons;
    the reference's ap, pre, rec [16])."""
    g = np.load(path)
    F = len(g['pr_seg']) - 1
    packed = {k: g[k].astype(np.float64) for k in ('pr_xys', 'gt_xy', 'gt_head')}
    packed.update({k: g[k].astype(np.int32) for k in ('pr_has', 'gt_has', 'pr_seg', 'gt_seg')})
    packed.update({'poly_seg': np.zeros(F + 1, np.int32), 'vert_seg': np.zeros(1, np.int32), 'verts': np.zeros((0, 2)),
                   'frame_index': g['frame_index'].astype(np.int64)})
    return packed, (g['ap'], g['pre'], g['rec'])
