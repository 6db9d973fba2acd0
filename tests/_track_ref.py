"""float64 numpy restatement of the OKS pose tracker (csrc/track.hip: fami_pose_track_f32; evaluate.pose_track), in this
project's words -- the reference has no association rule, so the rule is the one include/fami.h states:

Per video, frames in ascending frame number.  A live track holds an id and the (x, y) of its J joints, the box area and
the frame number of the last detection matched to it.  Before frame f every track with f - last_frame > max_gap is
retired.  The detections of f are walked in the order of filenames_map[image]: detection d takes the live track with the
largest OKS among those not matched in this frame yet (tracks created in this frame do not compete; equal OKS: the lowest
id) if that OKS is > oks_thre -- it gets the id, the track takes d's pose, area and frame number -- and is new otherwise.
After the walk the new detections get ids next_id, next_id + 1, ... in list order and become live.  Ids start at 0 in
every video and are never reused.
    OKS(q, d) = mean_j exp(-(dx^2 + dy^2) / (2 sigma_j)^2 / ((a_q + a_d) / 2 + 2^-52) / 2)
over all joints, or with vis_thre over the joints whose confidence in d exceeds it; 0 on an empty mask.

The inputs are rounded to fp32 first, as the upload does; everything after that is float64.  The device's exp and
summation order can differ from numpy's by ~1e-16 relative, so `pose_track_ref` also returns the smallest relative MARGIN
of its decisions: |OKS - thr| / thr for every OKS that is compared with the threshold (every competing track of every
detection), and, wherever a detection takes a track, the gap between the best and the next lower OKS relative to the
larger of the two.  OKS values that are equal bit for bit come from identical inputs and are resolved by the tie rule
identically everywhere: they do not enter the margin.  Inputs whose margin is >= 1e-4 cannot flip."""
import numpy as np

COCO_SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
EPS = np.spacing(1)


def default_frame_of(key):
    parts = key.split('/')
    return parts[-3] + '/' + parts[-2], int(parts[-1].rsplit('.', 1)[0])


def oks_tracks(t_xy, t_area, d, d_area, var, vis_thr=None):
    """OKS of the tracks t_xy [k,J,2] (areas t_area [k]) against ONE detection d [J,3] (area d_area) -> [k] float64."""
    dx, dy = d[None, :, 0] - t_xy[:, :, 0], d[None, :, 1] - t_xy[:, :, 1]
    e = (dx ** 2 + dy ** 2) / var[None] / ((t_area + d_area) / 2 + EPS)[:, None] / 2
    mask = np.ones(len(var), dtype=bool) if vis_thr is None else d[:, 2] > vis_thr
    cnt = int(mask.sum())
    if cnt == 0:
        return np.zeros(len(t_xy))
    return np.exp(-e)[:, mask].sum(1) / cnt


def track_video(frames, preds, area, var, oks_thre, max_gap, vis_thre, tracks, stats):
    """frames: [(frame number, [rows])] of ONE video in ascending frame number.  Fills tracks[row]; -> (ids handed out,
    margin).  stats: dict of counters, see pose_track_ref."""
    J = preds.shape[1]
    ids = np.zeros(0, dtype=np.int64)              # the live tracks, in any order (the result does not depend on it)
    xy, ar, last = np.zeros((0, J, 2)), np.zeros(0), np.zeros(0, dtype=np.int64)
    next_id, margin, retired_before = 0, np.inf, False
    scale = abs(oks_thre) if oks_thre != 0 else 1.0
    for f, rows in frames:
        keep = f - last <= max_gap
        if not keep.all():
            stats['retired'] += int((~keep).sum())
            retired_before = True
            ids, xy, ar, last = ids[keep], xy[keep], ar[keep], last[keep]
        if len(rows) > 64 and len(ids) > 64:
            stats['big_frames'] += 1
        matched = np.zeros(len(ids), dtype=bool)
        new = []
        for r in rows:
            o_all = oks_tracks(xy, ar, preds[r], area[r], var, vis_thre)
            comp = np.flatnonzero(~matched)
            o = o_all[comp]
            take = -1
            if o.size:
                margin = min(margin, float(np.abs(o - oks_thre).min() / scale))
                best = o.max()
                if best > oks_thre:
                    cand = comp[o == best]
                    take = int(cand[np.argmin(ids[cand])])          # equal OKS: the lowest id
                    lower = o[o != best]
                    if lower.size:
                        nxt = lower.max()
                        margin = min(margin, float((best - nxt) / max(abs(best), abs(nxt))))
            if matched.any():                                       # the track it fits best went to an earlier detection
                m = o_all[matched].max()
                if m > oks_thre and (o.size == 0 or m > o.max()):
                    stats['contested'] += 1
            if take >= 0:
                if f - last[take] > 1:
                    stats['reid_across_gap'] += 1
                tracks[r] = ids[take]
                matched[take] = True
                xy[take], ar[take], last[take] = preds[r, :, :2], area[r], f
                stats['matched'] += 1
            else:
                new.append(r)
        if new:
            if retired_before:
                stats['new_after_retirement'] += len(new)
            k = len(new)
            tracks[new] = next_id + np.arange(k)
            ids = np.concatenate([ids, next_id + np.arange(k)])
            xy = np.concatenate([xy, preds[new][:, :, :2]])
            ar = np.concatenate([ar, area[new]])
            last = np.concatenate([last, np.full(k, f, dtype=np.int64)])
            next_id += k
        stats['max_live'] = max(stats['max_live'], len(ids))
    return next_id, margin


def pose_track_ref(preds, boxes, filenames_map, oks_thre=0.3, max_gap=3, vis_thre=None, sigmas=None, frame_of=None):
    """What evaluate.pose_track returns, and more -> dict: tracks [N] int32 (-1 for a row no image lists), num_tracks
    {video: ids handed out} (videos in the order of their first key), margin, and stats: counters over the whole set --
    'matched', 'retired', 'new_after_retirement' (new ids in a video after one of its tracks was retired),
    'reid_across_gap' (matches to a track last seen more than one frame number ago), 'contested' (detections whose best
    live track had been taken by an earlier detection of the frame), 'big_frames' (frames of more than 64 detections
    while more than 64 tracks are live), 'max_live' (the most live tracks behind any frame: what the kernel's 256 slots must hold)."""
    preds = np.asarray(preds).astype(np.float32).astype(np.float64)
    area = np.asarray(boxes)[:, 4].astype(np.float32).astype(np.float64)
    sig = (COCO_SIGMAS if sigmas is None else np.asarray(sigmas, np.float64)).astype(np.float32).astype(np.float64)
    var = (sig * 2) ** 2
    frame_of = default_frame_of if frame_of is None else frame_of
    videos = {}
    for key, rows in filenames_map.items():
        video, f = frame_of(key)
        videos.setdefault(video, []).append((int(f), [int(r) for r in rows]))
    tracks = np.full(len(preds), -1, dtype=np.int32)
    stats = {k: 0 for k in ('matched', 'retired', 'new_after_retirement', 'reid_across_gap', 'contested', 'big_frames',
                            'max_live')}
    num, margin = {}, np.inf
    for video, frames in videos.items():
        frames.sort(key=lambda fr: fr[0])
        num[video], mg = track_video(frames, preds, area, var, oks_thre, max_gap, vis_thre, tracks, stats)
        margin = min(margin, mg)
    return {'tracks': tracks, 'num_tracks': num, 'margin': margin, 'stats': stats}


# ---------------------------------------------------------------------------------------- seeded inputs
def make_video(rng, people, frames, J=17, max_gap=3, drop=0.06, fp_rate=0.3, jitter=1.5, speed=5.0, cross=True):
    """One video -> [(frame number, kpts [n,J,3], area [n])] for the frame numbers in `frames` (ascending ints), frames
    without a detection left out.  `people` persons move on smooth trajectories (a constant velocity of about `speed`
    pixels per frame plus a slow sine), every keypoint jittered by `jitter` pixels per frame; with cross=True every
    second person has the SHAPE of the one before and a path that meets it in the middle of the video (a crossing).
    With probability `drop` per frame a person goes missing for 1, max_gap - 1, max_gap or max_gap + 2 frames (shorter
    and longer than the tracker's patience).  Each frame gets Poisson(fp_rate) false positives: poses seen once.  The
    order of the detections within a frame is shuffled."""
    F = len(frames)
    mid = frames[F // 2]
    shape = 40.0 * rng.standard_normal((people, J, 2))
    c0 = rng.uniform([100, 100], [1800, 900], (people, 2))
    vel = speed * rng.standard_normal((people, 2))
    a0 = rng.uniform(8e3, 3e4, people)
    if cross:
        for p in range(1, people, 2):
            shape[p] = shape[p - 1]
            a0[p] = a0[p - 1]
            c0[p] = c0[p - 1] + (vel[p - 1] - vel[p]) * (mid - frames[0])       # both at the same place at frame `mid`
    phase, amp = rng.uniform(0, 6.28, people), rng.uniform(0, 10, people)
    away = np.zeros(people, dtype=np.int64)
    out = []
    for f in frames:
        ks, ar = [], []
        for p in range(people):
            if away[p] == 0 and rng.uniform() < drop:
                away[p] = rng.choice([1, max(1, max_gap - 1), max_gap, max_gap + 2])
            if away[p] > 0:
                away[p] -= 1
                continue
            c = c0[p] + vel[p] * (f - frames[0]) + amp[p] * np.sin(phase[p] + 0.3 * f)
            k = np.zeros((J, 3))
            k[:, :2] = c[None] + shape[p] + jitter * rng.standard_normal((J, 2))
            k[:, 2] = rng.uniform(0.05, 1.0, J)
            ks.append(k)
            ar.append(a0[p] * rng.uniform(0.95, 1.05))
        for _ in range(rng.poisson(fp_rate)):
            k = np.zeros((J, 3))
            k[:, :2] = rng.uniform([100, 100], [1800, 900])[None] + 40.0 * rng.standard_normal((J, 2))
            k[:, 2] = rng.uniform(0.05, 1.0, J)
            ks.append(k)
            ar.append(rng.uniform(8e3, 3e4))
        if ks:
            order = rng.permutation(len(ks))
            out.append((int(f), np.asarray(ks)[order].astype(np.float32), np.asarray(ar)[order].astype(np.float32)))
    return out


def scatter(rng, videos, J, spare=0, fmt='/d/images/%s/%08d.jpg'):
    """videos: {'<set>/<name>': make_video(...)} -> preds [N,J,3], boxes [N,6] float64 (fp32 values), filenames_map.
    The detections get rows in a random order (plus `spare` rows that no image lists), so every list is interleaved with
    the others'; the keys of all videos are shuffled together, so videos are interleaved and frames out of order."""
    N = sum(len(k) for v in videos.values() for _, k, _ in v) + spare
    rows = rng.permutation(N)
    preds, boxes = rng.uniform(0.3, 1.0, (N, J, 3)), np.zeros((N, 6))
    boxes[:, :4] = rng.uniform(0, 100, (N, 4))
    boxes[:, 4:] = rng.uniform(0.3, 1.0, (N, 2))                   # the spare rows hold ordinary values too
    items, i = [], 0
    for name, frames in videos.items():
        for f, k, a in frames:
            r = rows[i:i + len(k)]
            i += len(k)
            preds[r], boxes[r, 4] = k, a
            items.append((fmt % (name, f), [int(x) for x in r]))
    fmap = {}
    for j in rng.permutation(len(items)):
        fmap[items[j][0]] = items[j][1]
    return preds, boxes, fmap


# ---------------------------------------------------------------------------------------- the families of the GPU test
SIGMAS15 = np.array([.89, .87, 1.07, 1.07, .87, .89, .62, .72, .79, .79, .72, .62, .79, .26, .5]) / 10.0   # PoseTrack order
SEEDS = {'main': 6, 'j15': 1, 'j1': 0, 'j32': 1}       # chosen on the CPU so that every run's margin is >= MARGIN
MARGIN = 1e-4


def _main_family(seed):
    """J = 17, default sigmas, V = 40: 32 small videos (2 ... 6 people, 8 ... 14 frames, some with frame numbers that
    skip), frames of exactly 1, 63, 64, 65 and 256 detections, a video of one frame, a video whose only list is empty,
    a crowd of 70 over five frames with dropouts (more than 64 detections against more than 64 live tracks), and three
    rows that no image lists."""
    rng = np.random.RandomState(seed)
    videos = {}
    for i in range(32):
        F = rng.randint(8, 15)
        frames = list(np.cumsum(rng.choice([1, 1, 1, 2], F)) + rng.randint(0, 50))
        videos['val/v%02d' % i] = make_video(rng, rng.randint(2, 7), frames)
    videos['val/one'] = make_video(rng, 1, [7, 8, 9, 10], drop=0, fp_rate=0, cross=False)
    for n in (63, 64, 65):
        videos['val/n%d' % n] = make_video(rng, n, [1, 2, 3], drop=0, fp_rate=0)
    videos['val/n256'] = make_video(rng, 256, [5, 6], drop=0, fp_rate=0, jitter=0.5, speed=2.0, cross=False)   # all re-found: AT the cap
    videos['val/single'] = make_video(rng, 3, [12], drop=0, fp_rate=0)
    videos['val/crowd'] = make_video(rng, 70, [1, 2, 3, 4, 5], drop=0.03, fp_rate=1.0)
    preds, boxes, fmap = scatter(rng, videos, 17, spare=3)
    fmap['/d/images/val/empty/00000001.jpg'] = []
    runs = [dict(), dict(max_gap=1), dict(vis_thre=0.3, oks_thre=0.4)]
    return preds, boxes, fmap, None, runs


def _j15_family(seed):
    """J = 15 with its own sigmas, V = 3."""
    rng = np.random.RandomState(seed)
    videos = {'val/p%d' % i: make_video(rng, n, list(range(1, 11)), J=15) for i, n in enumerate((3, 5, 9))}
    preds, boxes, fmap = scatter(rng, videos, 15, spare=1)
    return preds, boxes, fmap, SIGMAS15, [dict(), dict(vis_thre=0.2, max_gap=1)]


def _j1_family(seed):
    """J = 1, V = 1: position alone."""
    rng = np.random.RandomState(seed)
    videos = {'val/dot': make_video(rng, 6, list(range(1, 13)), J=1, cross=False, speed=8.0)}
    preds, boxes, fmap = scatter(rng, videos, 1)
    return preds, boxes, fmap, np.array([0.079]), [dict(oks_thre=0.5)]


def _j32_family(seed):
    """J = 32 (more than 64 KiB of LDS), V = 2, one video with 80 people: two waves of tracks."""
    rng = np.random.RandomState(seed)
    videos = {'val/a': make_video(rng, 80, [1, 2, 4, 5], J=32, drop=0.05), 'val/b': make_video(rng, 4, list(range(3, 12)), J=32)}
    preds, boxes, fmap = scatter(rng, videos, 32, spare=2)
    return preds, boxes, fmap, rng.uniform(0.025, 0.107, 32), [dict(), dict(vis_thre=0.5, max_gap=2)]


FAMILIES = (('main', _main_family, 3), ('j15', _j15_family, 2), ('j1', _j1_family, 1), ('j32', _j32_family, 2))
_CASES = []


def cases():
    """Every (family, run) with its float64 reference, computed once per process -> list of dicts."""
    if not _CASES:
        for fam, make, nruns in FAMILIES:
            preds, boxes, fmap, sigmas, runs = make(SEEDS[fam])
            assert len(runs) == nruns
            for kw in runs:
                ref = pose_track_ref(preds, boxes, fmap, sigmas=sigmas, **kw)
                _CASES.append({'id': '%s-%s' % (fam, '-'.join('%s=%s' % (k[:3], v) for k, v in sorted(kw.items())) or 'default'),
                               'fam': fam, 'preds': preds, 'boxes': boxes, 'fmap': fmap, 'sigmas': sigmas, 'kw': kw, 'ref': ref})
    return _CASES


CASE_IDS = ['%s-%d' % (fam, i) for fam, _, n in FAMILIES for i in range(n)]


def overflow_set(seed=3):
    """Three videos; the middle one has 200 people in frame 1 and 100 other people in frame 2: 300 live tracks.
    -> preds, boxes, filenames_map, the name of the video that is too much."""
    rng = np.random.RandomState(seed)
    over = make_video(rng, 200, [1], drop=0, fp_rate=0, cross=False) + make_video(rng, 100, [2], drop=0, fp_rate=0, cross=False)
    videos = {'val/before': make_video(rng, 4, list(range(1, 9))), 'val/over': over, 'val/after': make_video(rng, 5, list(range(1, 9)))}
    preds, boxes, fmap = scatter(rng, videos, 17)
    return preds, boxes, fmap, 'val/over'
