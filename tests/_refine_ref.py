"""float64 numpy restatement of the track refinement (csrc/track_refine.hip: fami_track_fill_f32, fami_track_smooth_f32,
fami_track_score_f32; evaluate.track_refine), operation for operation, in this project's words -- the reference has no
tracker and no such step, so the rule is the one include/fami.h states:

Members: the rows the image lists name, grouped by (video, id) -- videos in the order of their first key, ids ascending --
by ascending frame number.  The inputs are rounded to fp32 first; every operation below is one float64 operation of numpy
(which contracts nothing), and a result is rounded to fp32 once.
1. Fill: consecutive members a, b with 1 <= f_b - f_a - 1 <= max_fill get a row for every f between them: t = (f - f_a) /
   (f_b - f_a); x, y and box columns 0 .. 4 are v_a + (v_b - v_a) * t; confidences and box column 5 are min(a, b) *
   fill_conf (a's value unless b's is smaller).  New rows are numbered N, N + 1, ... in (video, id, frame) order, appended
   to the list of their frame's key; a frame without one gets key_of(video, f, key of f_a's frame) behind all existing
   keys, in (video, frame) order.
2. Smooth: joint j of member i with confidence > conf_thre (both fp32): over the members k of the track with |f_k - f_i| <=
   radius in ascending frame order, those with c_kj > conf_thre: w = g[|f_k - f_i|] * c_kj; sw += w; sx += w * x; sy += w *
   y; then sx / sw, sy / sw -- unless no member other than i contributed: then x, y are copied.  g[d] = exp(-d * d / (2
   sigma^2)).  Neighbours are read unsmoothed.
3. Rescore: box column 5 of every member = (sum of the track's scores after the fill, in frame order) / count.
4. Prune: tracks with fewer than min_len members after the fill leave the lists and get id -1.

Nothing here is transcendental except the table g, which the device receives from the same numpy expression: the device's
outputs must EQUAL these, bit for bit."""
import os

import numpy as np

from _track_ref import default_frame_of


def default_key_of(video, f, sibling):
    head, name = os.path.split(sibling)
    stem, ext = os.path.splitext(name)
    return '%s/%s%s' % (head, str(f).zfill(len(stem)), ext)


def _r32(a):
    """rounded to fp32 once, held as float64"""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def track_refine_ref(preds, boxes, filenames_map, tracks, max_fill=2, fill_conf=1.0, smooth_radius=2, smooth_sigma=1.0,
                     conf_thre=0.0, rescore=False, min_len=1, frame_of=None, key_of=None):
    """What evaluate.track_refine returns, and the tables and intermediate results the raw entry points are held to ->
    dict: preds2 [N+G,J,3] float32, boxes2 [N+G,6] float64, fmap2, tracks2 [N+G] int32; fill [G,5] (end rows, frame number,
    the ends' frame numbers), mrow / mfr / mtrk [Mm] and tseg [T+1] (the members after the fill, sorted), gauss [radius+1],
    filled [N+G,J,3] float32 and boxes_filled [N+G,6] (after stage 1), score [T] float32 (the track means)."""
    frame_of = default_frame_of if frame_of is None else frame_of
    key_of = default_key_of if key_of is None else key_of
    N, J = np.shape(preds)[:2]
    kp = [k for k in _r32(preds)]
    bx = [b for b in _r32(boxes)]
    ids = [int(t) for t in tracks]
    videos, key_at, members = {}, {}, {}
    for key, rows in filenames_map.items():
        video, f = frame_of(key)
        v = videos.setdefault(video, len(videos))
        key_at[(v, int(f))] = key
        for r in rows:
            members.setdefault((v, ids[r]), []).append((int(f), int(r)))
    names = list(videos)
    fmap2 = {key: [int(r) for r in rows] for key, rows in filenames_map.items()}
    # 1. fill
    fill, fill_v, new_at = [], [], {}
    for (v, tid) in sorted(members):
        mem = sorted(members[(v, tid)])
        for (fa, a), (fb, b) in zip(mem[:-1], mem[1:]):
            if not 1 <= fb - fa - 1 <= max_fill:
                continue
            for f in range(fa + 1, fb):
                t = np.float64(f - fa) / np.float64(fb - fa)
                k, bo = np.zeros((J, 3)), np.zeros(6)
                k[:, :2] = kp[a][:, :2] + (kp[b][:, :2] - kp[a][:, :2]) * t
                k[:, 2] = np.where(kp[b][:, 2] < kp[a][:, 2], kp[b][:, 2], kp[a][:, 2]) * np.float64(fill_conf)
                bo[:5] = bx[a][:5] + (bx[b][:5] - bx[a][:5]) * t
                bo[5] = (bx[b][5] if bx[b][5] < bx[a][5] else bx[a][5]) * np.float64(fill_conf)
                row = len(kp)
                kp.append(_r32(k))
                bx.append(_r32(bo))
                ids.append(tid)
                fill.append((a, b, f, fa, fb))
                fill_v.append(v)
                members[(v, tid)].append((f, row))
                if (v, f) not in key_at and (v, f) not in new_at:
                    new_at[(v, f)] = key_of(names[v], f, key_at[(v, fa)])
                    assert frame_of(new_at[(v, f)]) == (names[v], f)
    for where in sorted(new_at):
        fmap2[new_at[where]] = []
    for g, (v, (a, b, f, fa, fb)) in enumerate(zip(fill_v, fill)):
        fmap2[key_at.get((v, f), new_at.get((v, f)))].append(N + g)
    R = len(kp)
    filled, boxes_filled = np.asarray(kp).reshape(R, J, 3), np.asarray(bx).reshape(R, 6)
    # the sorted member list
    mrow, mfr, mtrk, tseg = [], [], [], [0]
    for n, tk in enumerate(sorted(members)):
        for f, r in sorted(members[tk]):
            mrow.append(r)
            mfr.append(f)
            mtrk.append(n)
        tseg.append(len(mrow))
    T = len(tseg) - 1
    # 2. smooth
    radius = int(smooth_radius)
    d = np.arange(radius + 1, dtype=np.float64)
    gauss = np.exp(-(d * d) / (2.0 * float(smooth_sigma) * float(smooth_sigma)))
    thre = np.float32(conf_thre)
    out = filled.copy()
    if radius >= 1:
        c32 = filled[:, :, 2].astype(np.float32)
        for t in range(T):
            for i in range(tseg[t], tseg[t + 1]):
                sw, sx, sy, others = np.zeros(J), np.zeros(J), np.zeros(J), np.zeros(J, dtype=bool)
                # (frame numbers ascend strictly within a track: whatever is within `radius` frames is within `radius` members)
                for k in range(max(tseg[t], i - radius), min(tseg[t + 1], i + radius + 1)):
                    dist = abs(mfr[k] - mfr[i])
                    if dist > radius:
                        continue
                    on = c32[mrow[k]] > thre
                    w = gauss[dist] * filled[mrow[k], :, 2]
                    sw = np.where(on, sw + w, sw)
                    sx = np.where(on, sx + w * filled[mrow[k], :, 0], sx)
                    sy = np.where(on, sy + w * filled[mrow[k], :, 1], sy)
                    if k != i:
                        others |= on
                move = others & (c32[mrow[i]] > thre)
                with np.errstate(invalid='ignore', divide='ignore'):
                    out[mrow[i], :, 0] = np.where(move, _r32(sx / sw), filled[mrow[i], :, 0])
                    out[mrow[i], :, 1] = np.where(move, _r32(sy / sw), filled[mrow[i], :, 1])
    # 3. rescore
    score = np.zeros(T, dtype=np.float32)
    boxes2 = np.concatenate([np.asarray(boxes, dtype=np.float64), boxes_filled[N:]])
    for t in range(T):
        s = np.float64(0.0)
        for k in range(tseg[t], tseg[t + 1]):
            s = s + boxes_filled[mrow[k], 5]
        score[t] = np.float32(s / np.float64(tseg[t + 1] - tseg[t]))
        if rescore:
            for k in range(tseg[t], tseg[t + 1]):
                boxes2[mrow[k], 5] = score[t]
    # 4. prune
    tracks2 = np.asarray(ids, dtype=np.int32)
    for t in range(T):
        if tseg[t + 1] - tseg[t] < min_len:
            dead = set(mrow[tseg[t]:tseg[t + 1]])
            tracks2[list(dead)] = -1
            for key in fmap2:
                fmap2[key] = [r for r in fmap2[key] if r not in dead]
    i32 = lambda a: np.asarray(a, dtype=np.int32)  # noqa: E731
    return {'preds2': out.astype(np.float32), 'boxes2': boxes2, 'fmap2': fmap2, 'tracks2': tracks2,
            'fill': i32(fill).reshape(-1, 5), 'mrow': i32(mrow), 'mfr': i32(mfr), 'mtrk': i32(mtrk), 'tseg': i32(tseg),
            'gauss': gauss, 'filled': filled.astype(np.float32), 'boxes_filled': boxes_filled, 'score': score}


# ---------------------------------------------------------------------------------------- seeded inputs with known ids
def person_frames(rng, start, length, steps=(1, 1, 1, 2, 3, 4)):
    """`length` ascending frame numbers from `start`; consecutive ones differ by a draw from `steps` (step - 1 missing)."""
    return [int(f) for f in start + np.concatenate([[0], np.cumsum(rng.choice(steps, length - 1))])]


def make_set(rng, videos, J, spare=0, noise=1.5, fmt='/d/images/%s/%08d.jpg'):
    """videos: {'<set>/<name>': [frame numbers of person 0, of person 1, ...]} -> preds [N,J,3], boxes [N,6] float64 (fp32
    values), filenames_map, tracks [N] int64 -- person p of a video has id p.  Constant velocity plus i.i.d. noise of
    `noise` pixels, confidences in 0.05 .. 1.  The detections get rows in a random order (plus `spare` rows that no image
    lists, with id -1), each list is shuffled, and the keys of all videos are shuffled together: videos are interleaved and
    frames out of order in the map."""
    N = sum(len(fr) for v in videos.values() for fr in v) + spare
    rows = rng.permutation(N)
    preds = rng.uniform(0.3, 1.0, (N, J, 3)).astype(np.float32).astype(np.float64)
    boxes = rng.uniform(0.3, 100.0, (N, 6)).astype(np.float32).astype(np.float64)
    tracks = np.full(N, -1, dtype=np.int64)
    lists, i = {}, 0
    for name, people in videos.items():
        for p, frames in enumerate(people):
            shape, c0, vel = 40.0 * rng.standard_normal((J, 2)), rng.uniform(100, 900, 2), 5.0 * rng.standard_normal(2)
            b0, bv = rng.uniform(10, 100, 5), rng.standard_normal(5)
            for f in frames:
                r = int(rows[i])
                i += 1
                k = np.zeros((J, 3))
                k[:, :2] = c0 + vel * f + shape + noise * rng.standard_normal((J, 2))
                k[:, 2] = rng.uniform(0.05, 1.0, J)
                preds[r] = k.astype(np.float32)
                boxes[r, :5] = (b0 + bv * f).astype(np.float32)
                boxes[r, 5] = np.float32(rng.uniform(0.3, 1.0))
                tracks[r] = p
                lists.setdefault(fmt % (name, f), []).append(r)
    keys = list(lists)
    fmap = {}
    for j in rng.permutation(len(keys)):
        fmap[keys[j]] = [lists[keys[j]][q] for q in rng.permutation(len(lists[keys[j]]))]
    return preds, boxes, fmap, tracks


# ---------------------------------------------------------------------------------------- the families of the GPU test
def _main_family():
    """J = 17, V = 40: 31 videos of 2 ... 5 people over 8 ... 14 members each with 0 ... 3 frame numbers missing between
    members (other people present in the gap: new rows in frames WITH a key), single-person videos with tracks of 1, 2,
    63, 64, 65 and 300 members (new rows in frames WITHOUT a key), a single person with gaps of exactly 16 and 17, two
    people with gaps of 1, 2 and 3, and three rows that no image lists."""
    rng = np.random.RandomState(11)
    videos = {}
    for i in range(31):
        videos['val/v%02d' % i] = [person_frames(rng, rng.randint(0, 5), rng.randint(8, 15)) for _ in range(rng.randint(2, 6))]
    for n in (1, 2, 63, 64, 65, 300):
        videos['val/n%d' % n] = [person_frames(rng, 3, n, steps=(1, 1, 1, 1, 2, 3))]
    videos['val/wide'] = [[1, 2, 3, 20, 21, 39, 40]]                       # 16 missing, then 17
    videos['val/gaps'] = [[1, 2, 4, 7, 11, 12], [1, 3, 4, 5, 9, 12]]      # 1, 2, 3 missing; windows across filled gaps
    videos['val/solo'] = [[5]]
    assert len(videos) == 40
    preds, boxes, fmap, tracks = make_set(rng, videos, 17, spare=3)
    runs = [dict(), dict(max_fill=1, smooth_radius=1, rescore=True, min_len=3), dict(max_fill=0), dict(smooth_radius=0),
            dict(max_fill=16, smooth_radius=16, smooth_sigma=4.0, conf_thre=0.3, fill_conf=0.5, rescore=True, min_len=2),
            dict(max_fill=0, smooth_radius=0, rescore=True)]
    return preds, boxes, fmap, tracks, runs


def _j1_family():
    """J = 1, V = 1"""
    rng = np.random.RandomState(12)
    videos = {'val/dot': [person_frames(rng, 1, 12) for _ in range(4)]}
    preds, boxes, fmap, tracks = make_set(rng, videos, 1)
    return preds, boxes, fmap, tracks, [dict(conf_thre=0.5), dict(max_fill=2, smooth_radius=1, min_len=13)]


def _j32_family():
    """J = 32, V = 2"""
    rng = np.random.RandomState(13)
    videos = {'val/a': [person_frames(rng, 2, 20) for _ in range(5)], 'val/b': [person_frames(rng, 7, 9)]}
    preds, boxes, fmap, tracks = make_set(rng, videos, 32, spare=2)
    return preds, boxes, fmap, tracks, [dict(rescore=True), dict(max_fill=16, smooth_radius=16, smooth_sigma=0.5)]


FAMILIES = (('main', _main_family, 6), ('j1', _j1_family, 2), ('j32', _j32_family, 2))
CASE_IDS = ['%s-%d' % (fam, i) for fam, _, n in FAMILIES for i in range(n)]
_CASES = []


def cases():
    """Every (family, run) with its float64 reference, computed once per process -> list of dicts."""
    if not _CASES:
        for fam, make, nruns in FAMILIES:
            preds, boxes, fmap, tracks, runs = make()
            assert len(runs) == nruns
            for kw in runs:
                _CASES.append({'fam': fam, 'preds': preds, 'boxes': boxes, 'fmap': fmap, 'tracks': tracks, 'kw': kw,
                               'ref': track_refine_ref(preds, boxes, fmap, tracks, **kw)})
    return _CASES
