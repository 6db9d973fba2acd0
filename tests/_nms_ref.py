"""float64 numpy restatement of the reference's pose NMS (datasets/process/nms.py:51-192: oks_iou, oks_nms, _rescore,
soft_oks_nms) and of the HRNet rescoring rule behind VAL/TEST.IN_VIS_THRE, in this project's words: the yardstick of
csrc/nms.hip (fami_pose_nms_f32) and of evaluate.pose_nms.

Where the reference leaves something open, the rule is the kernel's and is stated here:
  * order: descending score, equal scores by the lower position in the image's list (the reference's
    `argsort()[::-1]` leaves ties unspecified);
  * the score everything orders by is the rescored value ROUNDED TO fp32 (what the caller gets back);
  * the OKS mask reads the visibility of the compared detection only: the reference's
    `list(vg > vis_thr) and list(vd > vis_thr)` is Python's `and` on two non-empty lists, i.e. the second list.
The reference stores its OKS values as float32 and, in soft mode, squares them in float32; here everything is float64.
That is a relative difference of ~1e-7 in a compared quantity, so every function that decides something also returns
the smallest relative MARGIN of its decisions: |OKS - thr| / thr for each hard comparison, and at each pick of the soft
walk the gap between the best and the next lower working score relative to the larger magnitude.  Working scores that
are equal bit for bit are not a decision of the arithmetic (the tie rule resolves them, identically everywhere, as they
come from identical inputs) and do not enter the margin.  Inputs whose margin is >= 1e-4 cannot flip under 1e-7."""
import numpy as np

COCO_SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
EPS = np.spacing(1)                       # 2^-52, the reference's guard of the area term


def rescore(kpts, box_score, in_vis_thre):
    """kpts [n,J,3], box_score [n] -> [n] float64 holding fp32 values: box_score * mean(conf_j | conf_j > in_vis_thre),
    the mean 0 where no joint passes; the sum runs over j in ascending order (HRNet's loop), one rounding to fp32."""
    kpts = np.asarray(kpts, dtype=np.float64)
    box_score = np.asarray(box_score, dtype=np.float64)
    out = np.zeros(len(kpts), dtype=np.float64)
    for i in range(len(kpts)):
        total, cnt = 0.0, 0
        for c in kpts[i, :, 2]:
            if c > in_vis_thre:
                total += float(c)
                cnt += 1
        mean = total / cnt if cnt else 0.0
        out[i] = np.float32(float(box_score[i]) * mean)
    return out


def oks_iou(g, d, a_g, a_d, sigmas=None, vis_thr=None):
    """OKS of the picked pose g [J,3] (area a_g) against each pose of d [k,J,3] (areas a_d [k]) -> [k] float64."""
    sigmas = COCO_SIGMAS if sigmas is None else np.asarray(sigmas, dtype=np.float64)
    g, d = np.asarray(g, dtype=np.float64), np.asarray(d, dtype=np.float64).reshape(-1, len(sigmas), 3)
    a_d = np.asarray(a_d, dtype=np.float64).reshape(-1)
    var = (sigmas * 2) ** 2
    dx, dy = d[:, :, 0] - g[None, :, 0], d[:, :, 1] - g[None, :, 1]
    e = (dx ** 2 + dy ** 2) / var[None] / ((float(a_g) + a_d) / 2 + EPS)[:, None] / 2
    mask = np.ones(e.shape, dtype=bool) if vis_thr is None else d[:, :, 2] > vis_thr     # the compared pose's only
    cnt = mask.sum(1)
    s = np.where(mask, np.exp(-e), 0.0).sum(1)
    return np.where(cnt > 0, s / np.maximum(cnt, 1), 0.0)


def _best(work, alive):
    """position of the largest working score among `alive` (first one on ties), or -1"""
    idx = np.flatnonzero(alive)
    if idx.size == 0:
        return -1
    return int(idx[np.argmax(work[idx])])            # argmax returns the first maximum: the lower position


def oks_nms(kpts, scores, areas, thr, sigmas=None, vis_thr=None):
    """-> (keep: positions in pick order, margin).  Walks the detections by descending score; an unsuppressed one is
    kept and suppresses every later one whose OKS with it exceeds thr."""
    kpts, scores, areas = np.asarray(kpts, np.float64), np.asarray(scores, np.float64), np.asarray(areas, np.float64)
    alive = np.ones(len(scores), dtype=bool)
    keep, margin = [], np.inf
    while True:
        p = _best(scores, alive)
        if p < 0:
            break
        keep.append(p)
        alive[p] = False
        rest = np.flatnonzero(alive)
        if rest.size:
            o = oks_iou(kpts[p], kpts[rest], areas[p], areas[rest], sigmas, vis_thr)
            margin = min(margin, float(np.abs(o - thr).min() / abs(thr)))
            alive[rest[o > thr]] = False
    return keep, margin


def rescore_overlap(overlap, scores, thr, kind='gaussian'):
    """_rescore: the working scores after a pick whose OKS with them is `overlap`."""
    if kind == 'linear':
        return np.where(overlap >= thr, scores * (1 - overlap), scores)
    if kind != 'gaussian':
        raise ValueError(kind)
    return scores * np.exp(-overlap ** 2 / thr)


def soft_oks_nms(kpts, scores, areas, thr, max_dets=20, sigmas=None, vis_thr=None):
    """-> (keep, margin).  Keeps the detection with the largest working score, decays every other working score by
    exp(-OKS^2 / thr), and repeats until nothing is left or max_dets are kept."""
    kpts, areas = np.asarray(kpts, np.float64), np.asarray(areas, np.float64)
    work = np.array(scores, dtype=np.float64)
    alive = np.ones(len(work), dtype=bool)
    keep, margin = [], np.inf
    while len(keep) < max_dets:
        p = _best(work, alive)
        if p < 0:
            break
        lower = work[alive & (work != work[p])]                        # bit-equal scores: the tie rule, no decision
        if lower.size:
            nxt = lower.max()
            margin = min(margin, float((work[p] - nxt) / max(abs(work[p]), abs(nxt))))
        keep.append(p)
        alive[p] = False
        rest = np.flatnonzero(alive)
        if rest.size:
            o = oks_iou(kpts[p], kpts[rest], areas[p], areas[rest], sigmas, vis_thr)
            work[rest] = rescore_overlap(o, work[rest], thr)
    return keep, margin


def pose_nms_ref(preds, boxes, filenames_map, in_vis_thre=0.0, oks_thre=0.5, soft=False, max_dets=20, vis_thre=None,
                 sigmas=None):
    """What evaluate.pose_nms returns, plus the raw outputs of the kernel -> dict: scores [N] float64 (fp32 values; 0
    for a row no image lists), rank [N] int32, kept [M] int32, keep_map, margin.  The inputs are rounded to fp32 first,
    as the upload does."""
    preds = np.asarray(preds).astype(np.float32).astype(np.float64)
    boxes = np.asarray(boxes)
    area = boxes[:, 4].astype(np.float32).astype(np.float64)
    bs = boxes[:, 5].astype(np.float32).astype(np.float64)
    sig = (COCO_SIGMAS if sigmas is None else np.asarray(sigmas, np.float64)).astype(np.float32).astype(np.float64)
    N = len(preds)
    scores = np.zeros(N)
    rank = np.full(N, -1, dtype=np.int32)
    kept = np.zeros(len(filenames_map), dtype=np.int32)
    keep_map, margin = {}, np.inf
    for m, (key, rows) in enumerate(filenames_map.items()):
        rows = np.asarray(list(rows), dtype=np.int64)
        sc = rescore(preds[rows], bs[rows], in_vis_thre)
        scores[rows] = sc
        if soft:
            keep, mg = soft_oks_nms(preds[rows], sc, area[rows], oks_thre, max_dets, sig, vis_thre)
        else:
            keep, mg = oks_nms(preds[rows], sc, area[rows], oks_thre, sig, vis_thre)
        margin = min(margin, mg)
        keep = np.asarray(keep, dtype=np.int64)
        rank[rows[keep]] = np.arange(len(keep), dtype=np.int32)
        kept[m] = len(keep)
        keep_map[key] = [int(i) for i in rows[keep]]
    return {'scores': scores, 'rank': rank, 'kept': kept, 'keep_map': keep_map, 'margin': margin}


# ---------------------------------------------------------------------------------------- seeded inputs
def make_dets(rng, n, J=17, spread=(1.0, 3.0, 8.0, 20.0), per_cluster=4, conf=(0.05, 1.0)):
    """n detections of one image -> kpts [n,J,3] float32, area [n] float32, box_score [n] float32.  The poses come in
    clusters of about `per_cluster` jittered copies of a base pose (jitter sigma drawn from `spread`, in pixels), so the
    OKS values within a cluster cover (0, 1) and those between clusters are nearly 0; confidences are U(conf), box
    scores U(0.3, 1), areas U(8e3, 3e4) per cluster with 10 % jitter.  The order of the detections is shuffled."""
    kpts = np.zeros((n, J, 3))
    area, bs = np.zeros(n), rng.uniform(0.3, 1.0, n)
    i = 0
    while i < n:
        k = min(n - i, 1 + rng.randint(0, 2 * per_cluster - 1))
        base = rng.uniform([100, 100], [1800, 900])[None] + 40.0 * rng.standard_normal((J, 2))
        a = rng.uniform(8e3, 3e4)
        for _ in range(k):
            kpts[i, :, :2] = base + rng.choice(spread) * rng.standard_normal((J, 2))
            area[i] = a * rng.uniform(0.9, 1.1)
            i += 1
    kpts[:, :, 2] = rng.uniform(conf[0], conf[1], (n, J))
    order = rng.permutation(n)
    return kpts[order].astype(np.float32), area[order].astype(np.float32), bs[order].astype(np.float32)


# ---------------------------------------------------------------------------------------- the reference-made fixture
def fixture_cases(g):
    """tests/golden/pose_nms.npz -> [(c, soft, vis_thr | None, thr, max_dets, [keep positions per image])]"""
    out = []
    for c, (soft, vis, thr, md) in enumerate(g['cases']):
        keep, kseg = g['keep_%d' % c], g['kseg_%d' % c]
        out.append((c, bool(soft), None if np.isnan(vis) else float(vis), float(thr), int(md),
                    [[int(i) for i in keep[kseg[m]:kseg[m + 1]]] for m in range(len(kseg) - 1)]))
    return out


def fixture_properties(g):
    """What the fixture must exercise so that it cannot pass vacuously -> dict of counts over its hard-mode cases:
    'suppressed' detections, 'survivors_behind' (kept detections that a suppressed one outscores), and 'vis_changes'
    (images whose keep list differs between vis_thr none and 0.2 at the same threshold), plus 'soft_capped' (images
    where soft mode stopped at max_dets)."""
    seg, score = g['seg'], g['score']
    cases = fixture_cases(g)
    sup = behind = capped = vis_changes = 0
    for c, soft, vis, thr, md, keeps in cases:
        for m, keep in enumerate(keeps):
            n = int(seg[m + 1] - seg[m])
            if soft:
                capped += len(keep) == md < n
                continue
            sc = score[seg[m]:seg[m + 1]]
            gone = np.setdiff1d(np.arange(n), keep)
            sup += len(gone)
            if len(gone):
                behind += int((sc[keep] < sc[gone].max()).sum())
    for c, soft, vis, thr, md, keeps in cases:
        if vis is None:
            twin = [k for k in cases if k[1] == soft and k[2] is not None and k[3] == thr and k[4] == md][0]
            vis_changes += sum(a != b for a, b in zip(keeps, twin[5]))
    return {'suppressed': sup, 'survivors_behind': behind, 'vis_changes': vis_changes, 'soft_capped': capped}
