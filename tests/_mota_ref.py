"""Float64 numpy restatement of the PoseTrack MOTA the reference vendors (poseval/py/evaluateTracking.py:13-222
computeMetrics; the `mot` lists of eval_helpers.assignGTmulti :594-612, 648-658; py-motmetrics/motmetrics/mot.py:90-229
MOTAccumulator.update; the counts of metrics.py:196-218): the yardstick of tests/test_posetrack_mota_host.py and
tests/test_posetrack_mota_gpu.py, and what tools/gen_mota_golden.py holds against the reference's own assignGTmulti and
MOTAccumulator.update before it writes tests/golden/posetrack_mota.npz.  It does not import the package.

The rule.  Work is per sequence and per joint j: one accumulator each, its state a map m: annotated track id -> the
predicted track id it was last matched to.  Frames are those the AP's selection keeps (_ap_ref.select_frames), in order;
the LAST kept frame of every sequence is not evaluated; a sequence of one kept frame contributes nothing (the reference
raises IndexError there).  For joint j the objects of a frame are its annotated poses that still have j after the
ignore filter, the hypotheses its predicted poses that have it, d[o,h] = sqrt(dx^2 + dy^2) / headSize(o), valid iff
d <= thresh.  A frame without a predicted or without an annotated rect gives, for every joint, one object and one
hypothesis that cannot pair: one MISS, one FP.  One update (`update`):
  1. objects in order: m[o] exists, is among the hypotheses, not yet taken, pair valid -> MATCH, both taken;
  2. INV = 2 * max(valid d) + 1 (1 without a valid d); taken rows / columns and invalid pairs cost INV;
     scipy.optimize.linear_sum_assignment on that full matrix; every chosen pair of cost != INV is a SWITCH if m[o] exists
     and differs from h, else a MATCH; m[o] = h;
  3. objects left: MISS; hypotheses left: FP.
Counts per (sequence, joint): num_misses, num_switches, num_false_positives, num_detections = MATCH + SWITCH,
num_objects = MATCH + SWITCH + MISS, and sumD (math.fsum of the D of the detections).  `finish` is
evaluateTracking.py:158-192.

Two margins per (frame, joint) problem say how far the input is from a decision that rounding could turn:
  threshold   min |d - thresh| / thresh over the finite d of the problem;
  uniqueness  the assignment is solved again with each chosen valid pair forbidden (its cost set to INV) in turn; the
              smallest increase of the total cost.  0 means a second optimum with another set of valid pairs exists (a
              second optimum must lack a pair of the first: more valid pairs at equal cost is impossible, each is < INV).

Seeded generator: make_sequences (people on smooth paths with persistent ids; predictions with head-size-scaled noise,
dropped poses, twin and spurious poses, injected id swaps)."""
import math
import os
import sys

import numpy as np
from scipy.optimize import linear_sum_assignment

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ap_ref as ar  # noqa: E402

J = ar.J
COUNTS = ('num_misses', 'num_switches', 'num_false_positives', 'num_detections', 'num_objects')
MISS, SWITCH, FP, DET, OBJ = range(5)


def update(m, oids, hids, dist, margins=True):
    """One MOTAccumulator.update.  m is modified.  dist [len(oids), len(hids)], NaN where the pair is invalid.
    -> (n_match, n_switch, n_miss, n_fp, [D of the detections in event order], uniqueness margin; inf with
    margins=False, which leaves the re-solves out: what tools/bench_mota.py times)."""
    no, nh = len(oids), len(hids)
    dist = np.asarray(dist, dtype=np.float64).reshape(no, nh)
    o_taken, h_taken = np.zeros(no, bool), np.zeros(nh, bool)
    n_match = n_switch = 0
    ds, uniq = [], np.inf
    if no * nh > 0:
        valid = np.isfinite(dist)
        inv = 2.0 * dist[valid].max() + 1.0 if valid.any() else 1.0
        cost = np.where(valid, dist, inv)
        for i, o in enumerate(oids):                              # 1. carry forward
            if o not in m:
                continue
            js = [c for c, h in enumerate(hids) if h == m[o] and not h_taken[c]]
            if js and cost[i, js[0]] != inv:
                o_taken[i] = h_taken[js[0]] = True
                n_match += 1
                ds.append(cost[i, js[0]])
        cost[o_taken, :] = inv                                    # 2. the rest: minimum cost
        cost[:, h_taken] = inv
        rows, cols = linear_sum_assignment(cost)
        total = cost[rows, cols].sum()
        for i, c in zip(rows, cols) if margins else ():
            if cost[i, c] == inv:
                continue
            alt = cost.copy()
            alt[i, c] = inv
            r2, c2 = linear_sum_assignment(alt)
            uniq = min(uniq, float(alt[r2, c2].sum() - total))
        for i, c in zip(rows, cols):
            if cost[i, c] == inv:
                continue
            o, h = oids[i], hids[c]
            if o in m and m[o] != h:
                n_switch += 1
            else:
                n_match += 1
            ds.append(cost[i, c])
            o_taken[i] = h_taken[c] = True
            m[o] = h
    return n_match, n_switch, int((~o_taken).sum()), int((~h_taken).sum()), ds, uniq


def _rects(frame):
    return [r for r in frame['annorect'] if ar._rect_has_points(r)]


def frame_lists(fr, gt_frame, pr_frame, thresh=0.5):
    """fr: a frame of _ap_ref.select_frames, with the annolist frames it came from (for the track ids).
    -> None for the dummy frame, else ([(oids, hids, dist) per joint], threshold margin)."""
    if len(fr['gt']) == 0 or len(fr['pr']) == 0:
        return None
    g_rects, p_rects = _rects(gt_frame), _rects(pr_frame)
    g_ids = [g_rects[g['slot']]['track_id'][0] for g in fr['gt']]
    p_ids = [p_rects[p['slot']]['track_id'][0] for p in fr['pr']]
    out, margin = [], np.inf
    g_xy, p_xy = np.array([g['xy'] for g in fr['gt']]), np.array([p['xy'] for p in fr['pr']])
    heads = np.array([g['head'] for g in fr['gt']])
    hx, hy = heads[:, 2] - heads[:, 0], heads[:, 3] - heads[:, 1]
    head = 0.6 * np.sqrt(hx * hx + hy * hy)
    for j in range(J):
        gs = [i for i, g in enumerate(fr['gt']) if g['has'][j]]
        ps = [i for i, p in enumerate(fr['pr']) if p['has'][j]]
        dx = g_xy[gs, j, 0][:, None] - p_xy[ps, j, 0][None, :]
        dy = g_xy[gs, j, 1][:, None] - p_xy[ps, j, 1][None, :]
        with np.errstate(divide='ignore', invalid='ignore'):
            d = np.sqrt(dx * dx + dy * dy) / head[gs][:, None]
            if np.isfinite(d).any():
                margin = min(margin, float(np.min(np.abs(d[np.isfinite(d)] - thresh) / thresh)))
            dist = np.where(d <= thresh, d, np.nan)
        out.append(([g_ids[i] for i in gs], [p_ids[i] for i in ps], dist))
    return out, margin


def finish(counts, sumd):
    """counts [15,5] (the order of COUNTS), sumd [15] -> table [4,16]: mota, motp, pre, rec (evaluateTracking.py:158-192)."""
    table = np.zeros((4, J + 1))
    for j in range(J):
        miss, sw, fp, det, obj = (float(v) for v in counts[j])
        n_obj = obj if obj > 0 else np.nan
        table[0, j] = 100 * (1. - (miss + sw + fp) / n_obj)
        table[1, j] = 0.0 if det == 0 else 100 * (1. - (sumd[j] / det))
        table[2, j] = 100 * (1. * det / (fp + det if fp + det > 0 else np.nan))
        table[3, j] = 100 * (1. * det / n_obj)
    for r in range(4):
        ok = ~np.isnan(table[r, :J])
        table[r, J] = table[r, :J][ok].mean() if ok.any() else np.nan
    return table


def get_cum(table):
    return ar.get_cum(table[0]) + [float(table[r, J]) for r in (1, 2, 3)]


def sequences_of(frames, seq_ids):
    """The kept frames (_ap_ref.select_frames) grouped by sequence, in order of appearance -> [[frame, ...], ...]; a
    sequence without a kept frame has an empty list."""
    order, groups = {}, []
    for sid in seq_ids:
        if sid not in order:
            order[sid] = len(order)
            groups.append([])
    for fr in frames:
        groups[order[seq_ids[fr['idx']]]].append(fr)
    return groups


def evaluate_mota(gt_annolists, pr_annolists, seq_ids, thresh=0.5, margins=True):
    """-> dict: per_seq [S,15,5] int64, sumd_seq [S,15], the five counts [15], sum_d [15], mota / motp / pre / rec [16],
    cum [11], and of the input: thr_margin, uniq_margin (the smallest over all problems), problems (their number),
    longest (the most frames one sequence evaluates), dummy_frames."""
    groups = sequences_of(ar.select_frames(gt_annolists, pr_annolists), seq_ids)
    S = len(groups)
    per_seq, sumd_seq = np.zeros((S, J, 5), np.int64), np.zeros((S, J))
    res = {'thr_margin': np.inf, 'uniq_margin': np.inf, 'problems': 0, 'longest': 0, 'dummy_frames': 0}
    for s, frames in enumerate(groups):
        ms, ds = [{} for _ in range(J)], [[] for _ in range(J)]
        res['longest'] = max(res['longest'], len(frames) - 1)
        for fr in frames[:-1]:                                    # the last kept frame is not evaluated
            lists = frame_lists(fr, gt_annolists[fr['idx']], pr_annolists[fr['idx']], thresh)
            if lists is None:                                     # the dummy lists: one MISS, one FP
                per_seq[s, :, [MISS, FP, OBJ]] += 1
                res['dummy_frames'] += 1
                continue
            res['thr_margin'] = min(res['thr_margin'], lists[1])
            for j, (oids, hids, dist) in enumerate(lists[0]):
                n_match, n_switch, n_miss, n_fp, d, uniq = update(ms[j], oids, hids, dist, margins)
                per_seq[s, j] += (n_miss, n_switch, n_fp, n_match + n_switch, n_match + n_switch + n_miss)
                ds[j] += d
                res['uniq_margin'] = min(res['uniq_margin'], uniq)
                res['problems'] += int(len(oids) * len(hids) > 0)
        sumd_seq[s] = [math.fsum(d) for d in ds]
    counts = per_seq.sum(0)
    sum_d = np.array([math.fsum(sumd_seq[:, j]) for j in range(J)])
    table = finish(counts, sum_d)
    res.update({'per_seq': per_seq, 'sumd_seq': sumd_seq, 'sum_d': sum_d, 'table': table, 'cum': get_cum(table)})
    res.update({k: counts[:, i] for i, k in enumerate(COUNTS)})
    res.update({k: table[r] for r, k in enumerate(('mota', 'motp', 'pre', 'rec'))})
    return res


# ---------------------------------------------------------------------------------------- seeded sequences
def make_sequences(rng, n_seq, n_frames, max_people=4, noise=(0.05, 0.45), p_drop=0.12, p_twin=0.1, p_false=0.15,
                   p_swap=0.08, p_unannotated=0.05, grid=None):
    """-> (gt_annolist, pr_annolist, seq_ids): n_seq sequences of n_frames (an int or one per sequence) frames.  Every
    sequence has 2 .. max_people people who move on straight paths with a slow sway and keep their track id and their set
    of annotated joints; a person may leave for a few frames.  The tracker has an id per person: its prediction carries
    noise of `noise` head sizes, is dropped with p_drop (MISS), doubled with p_twin and joined by a stranger with p_false
    (FP, with fresh ids); with p_swap per frame two people's tracker ids are exchanged for good (SWITCH).  A frame is left
    unannotated with p_unannotated (the selection drops it)."""
    gt, pr, seq_ids = [], [], []
    lengths = [n_frames] * n_seq if np.isscalar(n_frames) else list(n_frames)
    for s in range(n_seq):
        n_people = rng.randint(2, max_people + 1)
        people = []
        for i in range(n_people):
            xy, present, head, size = ar.make_person(rng, grid=None)
            people.append({'xy': xy, 'present': present, 'head': head, 'size': size, 'vel': rng.normal(0, 6, 2),
                           'phase': rng.uniform(0, 6.28), 'gone': (rng.randint(0, lengths[s] + 1), rng.randint(0, 4))})
        ids = list(rng.permutation(n_people))                     # tracker id of person i
        fresh = n_people
        for f in range(lengths[s]):
            g_rects, p_rects = [], []
            if n_people >= 2 and rng.uniform() < p_swap:
                a, b = rng.choice(n_people, 2, replace=False)
                ids[a], ids[b] = ids[b], ids[a]
            for i, q in enumerate(people):
                if q['gone'][0] <= f < q['gone'][0] + q['gone'][1]:
                    continue
                shift = q['vel'] * f + 4.0 * np.array([math.sin(0.3 * f + q['phase']), math.cos(0.2 * f + q['phase'])])
                xy = ar._snap(q['xy'] + shift, grid)
                head = ar._snap(q['head'] + np.tile(shift, 2), grid)
                size = 0.6 * math.sqrt((head[2] - head[0]) ** 2 + (head[3] - head[1]) ** 2)
                g_rects.append(ar.gt_rect(xy, q['present'], head, 10 * i + 3))
                if rng.uniform() >= p_drop:
                    p_rects.append(ar.pr_rect(*ar.make_prediction(rng, xy, size, rng.uniform(*noise), grid=grid), track_id=int(ids[i])))
                    if rng.uniform() < p_twin:
                        p_rects.append(ar.pr_rect(*ar.make_prediction(rng, xy, size, rng.uniform(*noise), grid=grid), track_id=fresh))
                        fresh += 1
            if rng.uniform() < p_false:
                xy, present, head, size = ar.make_person(rng, grid=grid)
                p_rects.append(ar.pr_rect(*ar.make_prediction(rng, xy, size, 0.5, grid=grid), track_id=fresh))
                fresh += 1
            if rng.uniform() < p_unannotated:
                g_rects = []
            order = rng.permutation(len(p_rects))
            name = 'images/seq%02d/%08d.jpg' % (s, f + 1)
            gt.append({'image': [{'name': name}], 'imgnum': [f + 1], 'annorect': g_rects})
            pr.append({'image': [{'name': name}], 'imgnum': [f + 1], 'annorect': [p_rects[i] for i in order]})
            seq_ids.append(s)
    return gt, pr, seq_ids


def unpack(packed):
    """The arrays of evaluate.pack_posetrack_frames(gt, pr, seq_ids) (no polygons) -> (gt_annolist, pr_annolist, seq_ids)
    of the kept frames, the poses with their packed track ids."""
    gt, pr = ar.unpack(packed)
    for f, (gf, pf) in enumerate(zip(gt, pr)):
        if packed['gt_seg'][f + 1] > packed['gt_seg'][f]:
            for r, t in zip(gf['annorect'], packed['gt_track'][packed['gt_seg'][f]:packed['gt_seg'][f + 1]]):
                r['track_id'] = [int(t)]
        for r, t in zip(pf['annorect'], packed['pr_track'][packed['pr_seg'][f]:packed['pr_seg'][f + 1]]):
            r['track_id'] = [int(t)]
    return gt, pr, [int(s) for s in packed['frame_seq']]


def load_fixture(path):
    """tests/golden/posetrack_mota.npz -> (packed dict as evaluate.pack_posetrack_frames(gt, pr, seq_ids) returns it:
    fp64, no polygons; the reference's per_seq [S,15,5], sumd_seq [S,15] and table [4,16])."""
    g = np.load(path)
    F = len(g['pr_seg']) - 1
    packed = {k: g[k].astype(np.float64) for k in ('pr_xys', 'gt_xy', 'gt_head')}
    packed.update({k: g[k].astype(np.int32) for k in ('pr_has', 'gt_has', 'pr_seg', 'gt_seg', 'gt_track', 'pr_track',
                                                      'frame_seq', 'seq_seg')})
    packed.update({'poly_seg': np.zeros(F + 1, np.int32), 'vert_seg': np.zeros(1, np.int32), 'verts': np.zeros((0, 2)),
                   'frame_index': g['frame_index'].astype(np.int64)})
    return packed, (g['per_seq'].astype(np.int64), g['sumd_seq'].astype(np.float64), g['table'].astype(np.float64))
