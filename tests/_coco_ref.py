"""COCO keypoint AP / AR in float64 numpy: the restatement of include/fami.h (fami_coco_kpt_match_f64 /
fami_coco_kpt_curve_f64), which restates pycocotools' cocoeval.py with iouType='keypoints' for one category.  Plain loops, no
device, nothing imported from the package: tests/test_coco_ap_host.py holds it to hand-derived numbers and
tests/test_coco_ap_gpu.py holds the kernels to it.  It works on COCO annotation dicts and result dicts directly.

Two things are measured on every input besides the result, because the device's `exp` may differ from numpy's by an ulp:
`margin`, the smallest |OKS - min(t, 1 - 1e-10)| over every kept pair and threshold, and `tie_margin`, the smallest gap
between two OKS values of one detection that can compete in a walk (both at or above the lowest threshold) and are not
bit-identical.  The tests assert both to be >= 1e-9 before they compare decisions.

Also the inputs of those tests: `cases()` (hand-made, one property each), `seeded_set()`, `caps_set()`, `ties_set()`."""
import copy

import numpy as np

SIG = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
IOU = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
ARNG = np.array([[0 ** 2, 1e5 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]], dtype=np.float64)
EPS = np.spacing(1)
NAMES = ['AP', 'AP50', 'AP75', 'AP_M', 'AP_L', 'AR', 'AR50', 'AR75', 'AR_M', 'AR_L']


# ---------------------------------------------------------------------------------------- the restatement
def prepare(gt_anns, dt_anns, img_ids=None):
    """-> (image ids ascending, {id: [gt]}, {id: [dt]}): gt = kp [J,3], area, bbox, crowd, ignore, pos; dt = kp, score,
    area (of the bounding box of its (x, y) pairs), pos (its position in dt_anns)."""
    G, D = {}, {}
    for pos, g in enumerate(gt_anns):
        kp = np.array(g['keypoints'], dtype=np.float64).reshape(-1, 3)
        crowd = int(bool(g.get('iscrowd', 0)))
        nk = g['num_keypoints'] if 'num_keypoints' in g else int((kp[:, 2] > 0).sum())
        G.setdefault(g['image_id'], []).append({'kp': kp, 'area': float(g['area']), 'bbox': [float(v) for v in g['bbox']],
                                                'crowd': crowd, 'ignore': int(crowd or nk == 0), 'pos': pos})
    for pos, d in enumerate(dt_anns):
        kp = np.array(d['keypoints'], dtype=np.float64).reshape(-1, 3)
        x, y = kp[:, 0], kp[:, 1]
        D.setdefault(d['image_id'], []).append({'kp': kp, 'score': float(d['score']), 'pos': pos,
                                                'area': float((x.max() - x.min()) * (y.max() - y.min()))})
    ids = sorted(set(G) | set(D)) if img_ids is None else sorted(set(img_ids))
    return ids, {i: G.get(i, []) for i in ids}, {i: D.get(i, []) for i in ids}


def oks(g, d, var):
    """OKS of one detection against one annotation: the joints in ascending order, one rounding per operation."""
    xg, yg, vg = g['kp'][:, 0], g['kp'][:, 1], g['kp'][:, 2]
    xd, yd = d['kp'][:, 0], d['kp'][:, 1]
    k1 = int((vg > 0).sum())
    if k1 > 0:
        dx, dy = xd - xg, yd - yg
    else:
        bx, by, bw, bh = g['bbox']
        x0, x1, y0, y1 = bx - bw, bx + bw * 2, by - bh, by + bh * 2
        dx = np.maximum(0.0, x0 - xd) + np.maximum(0.0, xd - x1)
        dy = np.maximum(0.0, y0 - yd) + np.maximum(0.0, yd - y1)
    e = (dx * dx + dy * dy) / var / (g['area'] + EPS) / 2
    ex = np.exp(-e)
    s = 0.0
    for j in range(len(ex)):
        if k1 == 0 or vg[j] > 0:
            s = s + float(ex[j])
    return s / (k1 if k1 > 0 else len(ex))


def match_image(gts, dts, max_det, var, iou, arng):
    """-> dict: kept (positions in dts, score order), oks [K,G], flags [K, A*T] uint8 (bit 0 matched, bit 1 ignored; index
    a * T + t), taken [K, A*T] (index into gts, -1), npig [A], margin, tie_margin."""
    T, A = len(iou), len(arng)
    order = np.argsort([-d['score'] for d in dts], kind='mergesort')[:max_det] if dts else np.zeros(0, int)
    kept = [dts[i] for i in order]
    M = np.array([[oks(g, d, var) for g in gts] for d in kept], dtype=np.float64).reshape(len(kept), len(gts))
    thr = np.minimum(iou, 1 - 1e-10)
    margin = float(np.abs(M[:, :, None] - thr).min()) if M.size else np.inf
    tie = np.inf
    for row in M:
        v = np.sort(row[row >= thr.min() - 1e-9])
        gaps = np.diff(v)
        if (gaps > 0).any():
            tie = min(tie, float(gaps[gaps > 0].min()))
    flags = np.zeros((len(kept), A * T), np.uint8)
    taken = -np.ones((len(kept), A * T), int)
    npig = np.zeros(A, int)
    for a, (lo, hi) in enumerate(arng):
        gig = np.array([int(g['ignore'] or g['area'] < lo or g['area'] > hi) for g in gts], int)
        walk = np.argsort(gig, kind='mergesort')
        npig[a] = int((gig == 0).sum())
        for t in range(T):
            gtm = np.zeros(len(gts), bool)
            for k, d in enumerate(kept):
                best, m = thr[t], -1
                for g in walk:
                    if gtm[g] and not gts[g]['crowd']:
                        continue
                    if m > -1 and gig[m] == 0 and gig[g] == 1:
                        break
                    if M[k, g] < best:
                        continue
                    best, m = M[k, g], g
                if m > -1:
                    gtm[m] = True
                    flags[k, a * T + t] = 1 | (gig[m] << 1)
                    taken[k, a * T + t] = m
                elif d['area'] < lo or d['area'] > hi:
                    flags[k, a * T + t] = 2
    return {'kept': [int(i) for i in order], 'oks': M, 'flags': flags, 'taken': taken, 'npig': npig, 'margin': margin,
            'tie_margin': tie}


def curve(flags, npig, rec=REC):
    """flags: the bytes of one (a, t) in descending-score order -> (precision [R], recall); -1 with npig == 0."""
    if npig == 0:
        return -np.ones(len(rec)), -1.0
    flags = np.asarray(flags, np.uint8)
    matched, ig = (flags & 1).astype(bool), (flags & 2).astype(bool)
    tp = np.cumsum(matched & ~ig).astype(np.float64)
    fp = np.cumsum(~matched & ~ig).astype(np.float64)
    nd = len(tp)
    rc = tp / npig
    pr = tp / (fp + tp + EPS)
    q = np.zeros(len(rec))
    pr = np.maximum.accumulate(pr[::-1])[::-1]            # pycocotools' backward loop `if pr[i] > pr[i-1]: pr[i-1] = pr[i]`
    for ri, pi in enumerate(np.searchsorted(rc, rec, side='left')):
        if pi < nd:
            q[ri] = pr[pi]
    return q, (float(rc[-1]) if nd else 0.0)


def summarize(precision, recall, iou=IOU):
    def one(s, thr, a):
        if a >= s.shape[-1]:
            return -1.0
        if thr is not None:
            s = s[np.where(thr == iou)[0]]
        s = s[..., a]
        s = s[s > -1]
        return -1.0 if s.size == 0 else float(np.mean(s))
    return np.array([one(s, thr, a) for s in (precision, recall) for thr, a in ((None, 0), (.5, 0), (.75, 0), (None, 1), (None, 2))])


def evaluate(gt_anns, dt_anns, max_det=20, sigmas=SIG, iou=IOU, rec=REC, arng=ARNG, img_ids=None):
    """-> dict: stats [10], precision [T,R,A], recall [T,A], images (match_image per image that has anything), image_ids
    (those images), sorted_flags [A*T, N] (what the curve sees), margin, tie_margin."""
    var = (np.asarray(sigmas, dtype=np.float64) * 2) ** 2
    ids, G, D = prepare(gt_anns, dt_anns, img_ids)
    T, A = len(iou), len(arng)
    images, used = [], []
    for i in ids:
        if not G[i] and not D[i]:
            continue
        r = match_image(G[i], D[i], max_det, var, iou, arng)
        r['rows'] = [D[i][k]['pos'] for k in r['kept']]
        r['scores'] = [D[i][k]['score'] for k in r['kept']]
        images.append(r)
        used.append(i)
    precision, recall = -np.ones((T, len(rec), A)), -np.ones((T, A))
    sorted_flags = np.zeros((A * T, 0), np.uint8)
    if images:
        sc = np.concatenate([np.asarray(r['scores'], np.float64) for r in images])
        inds = np.argsort(-sc, kind='mergesort')
        sorted_flags = np.ascontiguousarray(np.concatenate([r['flags'] for r in images], axis=0)[inds].T)
        npig = np.sum([r['npig'] for r in images], axis=0)
        for a in range(A):
            for t in range(T):
                precision[t, :, a], recall[t, a] = curve(sorted_flags[a * T + t], int(npig[a]), rec)
    return {'stats': summarize(precision, recall, iou), 'precision': precision, 'recall': recall, 'images': images,
            'image_ids': used, 'sorted_flags': sorted_flags,
            'margin': min([r['margin'] for r in images] + [np.inf]), 'tie_margin': min([r['tie_margin'] for r in images] + [np.inf])}


# ---------------------------------------------------------------------------------------- inputs
def person(rng, cx, cy, size, vis=None, image_id=1, area=None, **extra):
    """An annotation: 17 joints scattered around (cx, cy); `area` defaults to 0.6 x the area of their bounding box."""
    xy = np.array([cx, cy]) + rng.normal(0, size / 4, (17, 2))
    v = np.full(17, 2) if vis is None else np.asarray(vis)
    x0, y0 = xy.min(0)
    x1, y1 = xy.max(0)
    g = {'image_id': image_id, 'category_id': 1, 'keypoints': np.c_[xy, v].ravel().tolist(),
         'area': float((x1 - x0) * (y1 - y0) * 0.6) if area is None else float(area),
         'bbox': [float(x0), float(y0), float(x1 - x0), float(y1 - y0)], 'iscrowd': 0, 'num_keypoints': int((v > 0).sum())}
    g.update(extra)
    return g


def det_of(g, score, rng=None, noise=0.0, shift=0.0):
    """A detection at the joints of annotation g, moved by `shift` pixels and N(0, noise x sqrt(area)) per coordinate."""
    kp = np.array(g['keypoints'], dtype=np.float64).reshape(-1, 3).copy()
    kp[:, :2] += shift
    if noise:
        kp[:, :2] += rng.normal(0, noise * np.sqrt(g['area']), kp[:, :2].shape)
    kp[:, 2] = 1.0
    return {'image_id': g['image_id'], 'category_id': 1, 'keypoints': kp.ravel().tolist(), 'score': float(score)}


def cases():
    """-> {name: (gt_anns, dt_anns, max_det)}: one property each; tests/test_coco_ap_host.py derives the numbers."""
    rng = np.random.default_rng(0)
    med = dict(area=5000.0)
    g1, g2 = person(rng, 100, 100, 120, **med), person(rng, 400, 300, 120, **med)
    far = person(rng, 2000, 2000, 120, **med)
    out = {'one_of_two': ([g1, g2], [det_of(g1, .9)], 20),
           'perfect': ([g1, g2], [det_of(g1, .9), det_of(g2, .8)], 20)}
    # 19 detections of nobody between the one of g1 and the one of g2, which is the 21st by score
    junk = [det_of(far, .9 - .01 * i, shift=40.0 * i) for i in range(19)]
    out['cut'] = ([g1, g2], [det_of(g2, .01)] + junk + [det_of(g1, .99)], 20)
    out['cut_21'] = (out['cut'][0], out['cut'][1], 21)
    # a crowd annotation takes two detections, both ignored; they outscore the true positive
    crowd = person(rng, 700, 100, 120, iscrowd=1, **med)
    out['crowd'] = ([crowd, g2], [det_of(crowd, .9, shift=1.0), det_of(crowd, .85, shift=-1.0), det_of(g2, .5)], 20)
    # two bit-identical annotations: the first detection takes the later one, the second the other
    out['twins'] = ([g1, copy.deepcopy(g1)], [det_of(g1, .9, shift=1.0), det_of(g1, .8, shift=2.0)], 20)
    # a crowd copy exactly under the detection, behind a plain annotation a little off: the walk stops before the copy
    near = det_of(g1, .9, shift=3.0)
    under = dict(copy.deepcopy(g1), keypoints=[v if i % 3 != 2 else 2 for i, v in enumerate(near['keypoints'])], iscrowd=1)
    out['stop'] = ([under, g1], [near], 20)
    # large people next to a medium one: in `medium` the detection of a large one is ignored, not a false positive
    big = person(rng, 1000, 600, 400, area=20000.0)
    out['out_of_range_match'] = ([big, g2], [det_of(big, .9), det_of(g2, .8)], 20)
    # a large detection of nobody: a false positive in `all`, ignored in `medium`
    nobody = person(rng, 3000, 600, 800)
    out['out_of_range_det'] = ([g2], [det_of(nobody, .9), det_of(g2, .8)], 20)
    # areas of exactly 32^2 and 96^2
    e1, e2 = person(rng, 100, 600, 60, area=32.0 ** 2), person(rng, 600, 600, 200, area=96.0 ** 2)
    out['edge_areas'] = ([e1, e2], [det_of(e1, .9), det_of(e2, .8)], 20)
    # an annotation without a labelled joint: the box-distance branch, ignored; one detection inside its doubled box (OKS 1),
    # one outside
    blank = person(rng, 1500, 100, 120, vis=np.zeros(17, int), **med)
    bx, by, bw, bh = blank['bbox']
    outside = det_of(blank, .7, shift=2.0 * max(bw, bh) + 30.0)
    out['no_labelled_joint'] = ([blank, g2], [det_of(blank, .9, shift=0.3 * bw), outside, det_of(g2, .5)], 20)
    # nothing but a crowd annotation: npig = 0
    out['only_crowd'] = ([crowd], [det_of(crowd, .9)], 20)
    return out


def seeded_set(seed=0, images=200):
    """-> (gt_anns, dt_anns, img_ids): 0 .. 4 people per image of four sizes (a quarter of them annotated twice, a little apart), 25 % of the joints unlabelled, 8 % crowd; 0 .. 2
    detections per person at three noise levels, 0 .. 1 of nobody; images with no detection, with no annotation and with
    neither occur (img_ids lists them all)."""
    rng = np.random.default_rng(seed)
    gt, dt = [], []
    for im in range(images):
        gs = []
        for _ in range(rng.integers(0, 5)):
            size = float(rng.choice([30, 70, 150, 300]))
            vis = (rng.uniform(size=17) > 0.25).astype(int) * 2
            g = person(rng, rng.uniform(50, 600), rng.uniform(50, 400), size, vis, image_id=im)
            g['iscrowd'] = int(rng.uniform() < 0.08)
            g['id'] = len(gt) + len(gs)
            gs.append(g)
            if rng.uniform() < 0.25:                          # a second annotation of nearly the same pose: competition
                kp = np.array(g['keypoints']).reshape(17, 3).copy()
                kp[:, :2] += rng.normal(0, 0.03 * np.sqrt(g['area']), (17, 2))
                gs.append(dict(g, keypoints=kp.ravel().tolist(), iscrowd=0, id=g['id'] + 1))
        gt += gs
        for g in gs:
            for _ in range(rng.integers(0, 3)):
                dt.append(det_of(g, rng.uniform(), rng, noise=float(rng.choice([0.02, 0.06, 0.15]))))
        for _ in range(rng.integers(0, 2)):
            dt.append(det_of(person(rng, rng.uniform(50, 600), rng.uniform(50, 400), 100, image_id=im), rng.uniform() * 0.5))
    return gt, dt, list(range(images))


def caps_set(seed=3):
    """Three images: a small one, one exactly at the caps (128 annotations, 256 detections; evaluated with max_dets 64), a
    small one."""
    rng = np.random.default_rng(seed)
    gt, dt = [], []
    for im, n in ((0, 2), (1, 128), (2, 3)):
        gs = [person(rng, rng.uniform(50, 3000), rng.uniform(50, 2000), float(rng.choice([70, 150, 300])), image_id=im)
              for _ in range(n)]
        for i, g in enumerate(gs):
            g['iscrowd'] = int(n > 3 and i % 16 == 5)
        gt += gs
        for g in gs:
            for _ in range(2):
                dt.append(det_of(g, rng.uniform(), rng, noise=float(rng.choice([0.02, 0.06, 0.15]))))
    return gt, dt, [0, 1, 2]


def ties_set(seed=5):
    """One image, 6 people, 24 detections whose scores repeat in blocks of four: with max_dets 18 (and 20, 21, 22) the cut
    falls inside a block of equal scores, and list order decides who is kept."""
    rng = np.random.default_rng(seed)
    gs = [person(rng, 300 + 400 * i, 300, 150, image_id=7) for i in range(6)]
    dt = [det_of(gs[i % 6], 0.9 - 0.1 * (i // 4), rng, noise=0.05) for i in range(24)]
    return gs, dt, [7]
