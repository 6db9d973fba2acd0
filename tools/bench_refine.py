"""What track refinement costs on a synthetic set of validation-set size, and what it does to the tracking metrics of a
synthetic set with known truth: the kernels fami_track_fill_f32 / fami_track_smooth_f32 / fami_track_score_f32 back to back
and with cold caches, `evaluate.track_refine` end to end, and the way a user had to do it otherwise: the numpy loop over
every track (tests/_refine_ref.track_refine_ref, the float64 restatement of the rule) on the same input.

    python tools/bench_refine.py [--videos 200] [--frames 100] [--reps 20] [--rounds 5] [--out profiles/refine]
                                 [--parent DIR [--bench-steps 30] [--bench-warmup 10]]

Timing set: the set of tools/bench_track.py (`--videos` videos of `--frames` frames, 2 ... 14 people each with dropouts,
crossings and false positives, about 144000 detections of 17 joints, plus one video of two frames with 256 people),
tracked first by `evaluate.pose_track` with its defaults.  Settings: the defaults (max_fill 2, smooth_radius 2) with
rescoring, and `wide` (smooth_radius 16, smooth_sigma 4: the longest window; max_fill 3, which adds no row here -- with the
tracker's max_gap = 3 a track survives at most 2 missing frame numbers, and max_fill 2 fills those).

kernels: device events around `--reps` launches on resident inputs, the settings alternating over `--rounds` rounds,
median and min..max in us per launch; COLD = single launches, each behind a 1 GiB fill that evicts the inputs from the
caches.  For the smooth kernel `bytes` is what it must move once -- the (x, y, confidence) of every member read and written
once, and its four tables -- and `share_of_hbm_peak` is bytes / time against 8 TB/s; that a warm launch exceeds what HBM
could deliver only says that the set is cache-resident.  The window re-reads (at most 2 * radius neighbours per joint) are
cache traffic and not counted.
end_to_end: `track_refine` on the host arrays (validation, tables, keys, one upload, the launches, one download, pruning),
host clock, median of `--rounds` calls.  numpy: one call of the restatement on the same arrays (default setting only);
`outputs_equal` says that all four results are the same, the arrays bit for bit.
metrics (SYNTHETIC, reported, not asserted): a second set, built here because the timing set's builder returns no truth:
`--metric-seqs` sequences of 60 frames, 2 ... 5 people on straight paths with 15 joints, detections = truth + jitter of
0.2 head sizes, people missing for 1 ... 3 frames at a time, one-frame false positives; tracked by `pose_track`, then
`posetrack_ap` / `posetrack_mota` of the poses as tracked and as refined (defaults; defaults + rescore + min_len 3).
--parent DIR: a built checkout of the parent commit; bench.py is run alternately there and here, three times each, as
child processes (--no-cpu-baseline --no-frozen --also none), and both medians are reported.
Prints one JSON line and writes it to <out>/bench_refine.json.  Needs the GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

os.environ.setdefault('HIP_FORCE_DEV_KERNARG', '1')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK = 8.0e12
MODES = {'default': dict(max_fill=2, smooth_radius=2, smooth_sigma=1.0, rescore=True),
         'wide': dict(max_fill=3, smooth_radius=16, smooth_sigma=4.0, rescore=True)}


def _stats(ts, unit):
    return {unit: round(statistics.median(ts), 2), 'min_' + unit: round(min(ts), 2), 'max_' + unit: round(max(ts), 2)}


def metric_set(seqs, frames=60, seed=2):
    """-> (gt annolist, seq_ids, preds [N,15,3], boxes [N,6], filenames_map): truth and detections of the metric set"""
    import _ap_ref as ar
    rng = np.random.RandomState(seed)
    gt, seq_ids, preds, boxes, fmap = [], [], [], [], {}
    for s in range(seqs):
        people = []
        for i in range(rng.randint(2, 6)):
            xy, _, head, size = ar.make_person(rng)
            people.append((xy, head, size, rng.normal(0, 4, 2), 0))
        away = [0] * len(people)
        for f in range(1, frames + 1):
            key = '/d/images/val/seq%03d/%08d.jpg' % (s, f)
            g_rects, rows = [], []
            for i, (xy, head, size, vel, _) in enumerate(people):
                shift = vel * f
                g_rects.append(ar.gt_rect(xy + shift, np.ones(15, bool), head + np.tile(shift, 2), i))
                if away[i] == 0 and rng.uniform() < 0.08:
                    away[i] = rng.randint(1, 4)
                if away[i] > 0:
                    away[i] -= 1
                    continue
                rows.append(len(preds))
                preds.append(np.concatenate([xy + shift + rng.normal(0, 0.2 * size, (15, 2)), rng.uniform(0.5, 1.0, (15, 1))], 1))
                boxes.append([0, 0, 0, 0, (6.0 * size) ** 2, rng.uniform(0.6, 1.0)])
            if rng.uniform() < 0.15:
                xy, _, head, size = ar.make_person(rng)
                rows.append(len(preds))
                preds.append(np.concatenate([xy, rng.uniform(0.2, 0.6, (15, 1))], 1))
                boxes.append([0, 0, 0, 0, (6.0 * size) ** 2, rng.uniform(0.2, 0.6)])
            fmap[key] = rows
            gt.append({'image': [{'name': key}], 'imgnum': [f], 'annorect': g_rects})
            seq_ids.append(s)
    f32 = lambda a: np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)  # noqa: E731
    return gt, seq_ids, f32(preds), f32(boxes), fmap


def metrics(ev, gt, seq_ids, preds, boxes, fmap, tracks, dev):
    """PoseTrack AP and MOTA of the poses (point score = confidence x box score) with their ids against the truth"""
    import _ap_ref as ar
    pr = []
    for fr in gt:
        rows = fmap.get(fr['image'][0]['name'], [])
        pr.append({'image': fr['image'], 'imgnum': fr['imgnum'],
                   'annorect': [ar.pr_rect(preds[r, :, :2], np.ones(15, bool), preds[r, :, 2] * boxes[r, 5], int(tracks[r])) for r in rows]})
    frames = ev.pack_posetrack_frames(gt, pr, seq_ids)
    ap, res = ev.posetrack_ap(frames, device=dev)['cum'], ev.posetrack_mota(frames, device=dev)
    mot = res['cum']                                           # seven group means of MOTA, then the totals of MOTA, MOTP, Prec, Rec
    rec = {'ap_total': round(float(ap[7]), 3), 'mota_total': round(float(mot[7]), 3), 'motp_total': round(float(mot[8]), 3),
           'mot_precision': round(float(mot[9]), 3), 'mot_recall': round(float(mot[10]), 3)}
    rec.update({k: int(np.asarray(res[k])[:15].sum()) for k in ('num_misses', 'num_switches', 'num_false_positives')})
    rec['poses'] = sum(len(f['annorect']) for f in pr)
    return rec


def bench_parity(parent, steps, warmup):
    """bench.py in the parent checkout and here, alternately, three child processes each -> clips/s of every run"""
    args = ['--gpus', '1', '--steps', str(steps), '--warmup', str(warmup), '--no-cpu-baseline', '--no-frozen', '--also', 'none']
    runs = {'parent': [], 'this': []}
    for _ in range(3):
        for name, root in (('parent', parent), ('this', ROOT)):
            out = subprocess.run([sys.executable, 'bench.py'] + args, cwd=root, capture_output=True, text=True, timeout=900)
            line = [ln for ln in out.stdout.splitlines() if ln.startswith('{')]
            if out.returncode or not line:
                raise SystemExit('bench.py failed in %s (%d): %s' % (root, out.returncode, out.stderr[-2000:]))
            runs[name].append(json.loads(line[-1])['value'])
            print('bench.py %s: %s clips/s' % (name, runs[name][-1]), file=sys.stderr, flush=True)
    med = {k: statistics.median(v) for k, v in runs.items()}
    return {'args': ' '.join(args), 'clips_per_s': runs, 'median': med, 'this_over_parent': round(med['this'] / med['parent'], 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--videos', type=int, default=200)
    ap.add_argument('--frames', type=int, default=100)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--metric-seqs', type=int, default=40)
    ap.add_argument('--parent', default=None)
    ap.add_argument('--bench-steps', type=int, default=30)
    ap.add_argument('--bench-warmup', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'refine'))
    a = ap.parse_args()
    if a.videos < 1 or a.frames < 1 or a.reps < 1 or a.metric_seqs < 1:
        ap.error('--videos, --frames, --reps and --metric-seqs must be >= 1')
    if a.rounds < 5:
        ap.error('--rounds must be >= 5: the spread between rounds is part of the result')
    if not torch.cuda.is_available():
        raise SystemExit('bench_refine needs the GPU')
    import _refine_ref as rr
    import bench_track
    from fami_pose_amd import evaluate as ev
    from fami_pose_amd._lib import lib
    dev = torch.device('cuda:0')
    s = torch.cuda.current_stream(dev).cuda_stream
    preds, boxes, fmap = bench_track.make_set(a.videos, a.frames)
    boxes[:, 5] = np.random.RandomState(3).uniform(0.3, 1.0, len(boxes)).astype(np.float32)
    tracks, num = ev.pose_track(preds, boxes, fmap, device=dev)
    N, J = len(preds), preds.shape[1]
    out = {'tool': 'bench_refine', 'device': torch.cuda.get_device_name(dev), 'videos': len(num), 'frames': len(fmap), 'detections': N,
           'joints': J, 'ids': int(sum(num.values())), 'reps': a.reps, 'rounds': a.rounds, 'hbm_peak_tb_s': HBM_PEAK / 1e12}
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)  # noqa: E731
    junk = torch.empty(1 << 28, device=dev)                    # 1 GiB: four times the Infinity Cache

    def window(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps

    def cold(fn, reps=11):
        ts = []
        for r in range(reps):
            junk.fill_(float(r))
            ts.append(window(fn, 1))
        return ts

    # the launches of every setting, on resident tables
    fns, info = {}, {}
    mrow, mvid, mid, mf, videos, key_at = ev._refine_members(fmap, N, tracks, None)
    for mode, kw in MODES.items():
        fill, g_vid, g_id, srow, sf, mtrk, tseg = ev._refine_tables(mrow, mvid, mid, mf, kw['max_fill'], N)
        G, Mm, T, R, radius = len(fill), len(srow), len(tseg) - 1, N + len(fill), kw['smooth_radius']
        d = np.arange(radius + 1, dtype=np.float64)
        t = [up(x, np.int32) for x in (fill, srow, sf, mtrk, tseg)] + [up(np.exp(-(d * d) / (2.0 * kw['smooth_sigma'] ** 2)), np.float64)]
        kp, bx = torch.zeros(R, J, 3, device=dev), torch.zeros(R, 6, device=dev)
        kp[:N], bx[:N] = up(preds, np.float32), up(boxes, np.float32)
        res = [torch.empty(R, J, 3, device=dev), torch.empty(T, device=dev), torch.zeros(3, dtype=torch.int32, device=dev)]
        hold = (t, kp, bx, res)
        p = lambda x, words=0: x.data_ptr() + 4 * words  # noqa: E731
        fns[mode + '/fill'] = lambda t=t, kp=kp, bx=bx, res=res, G=G: lib().call(
            'fami_track_fill_f32', p(kp), p(bx), p(t[0]), N, J, G, 1.0, p(kp, N * J * 3), p(bx, N * 6), p(res[2]), s)
        fns[mode + '/smooth'] = lambda t=t, kp=kp, res=res, R=R, Mm=Mm, T=T, radius=radius: lib().call(
            'fami_track_smooth_f32', p(kp), p(t[1]), p(t[2]), p(t[3]), p(t[4]), p(t[5]), R, J, Mm, T, radius, 0.0, p(res[0]), p(res[2], 1), s)
        fns[mode + '/score'] = lambda t=t, bx=bx, res=res, R=R, Mm=Mm, T=T: lib().call(
            'fami_track_score_f32', p(bx), p(t[1]), p(t[4]), R, Mm, T, p(res[1]), p(res[2], 2), s)
        info[mode] = {'new_rows': G, 'members': Mm, 'tracks': T, 'hold': hold,
                      'bytes': {'fill': G * (5 * 4 + 2 * (J * 3 + 6) * 4 + (J * 3 + 6) * 4),
                                'smooth': Mm * J * 12 * 2 + Mm * 12 + (T + 1) * 4 + (radius + 1) * 8,
                                'score': Mm * 8 + (T + 1) * 4 + T * 4}}
    for fn in fns.values():
        window(fn, 3)
    us = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, fn in fns.items():
            us[k].append(window(fn, a.reps))
    for mode in MODES:
        rec = {k: info[mode][k] for k in ('new_rows', 'members', 'tracks')}
        for stage in ('fill', 'smooth', 'score'):
            k = mode + '/' + stage
            r = _stats(us[k], 'us')
            c = cold(fns[k])
            r.update({'cold_us': round(statistics.median(c), 2), 'cold_min_us': round(min(c), 2), 'cold_max_us': round(max(c), 2),
                      'bytes': info[mode]['bytes'][stage]})
            if stage == 'smooth':
                r['gb_s'] = round(r['bytes'] / r['us'] / 1e3, 1)
                r['cold_gb_s'] = round(r['bytes'] / r['cold_us'] / 1e3, 1)
                r['share_of_hbm_peak'] = round(r['bytes'] / (r['us'] * 1e-6) / HBM_PEAK, 4)
                r['cold_share_of_hbm_peak'] = round(r['bytes'] / (r['cold_us'] * 1e-6) / HBM_PEAK, 4)
            rec[stage] = r
        torch.cuda.synchronize(dev)
        rec['flags'] = info[mode]['hold'][3][2].tolist()
        out['kernels_' + mode] = rec
    del junk, fns, info
    # end to end against the numpy loop
    for mode, kw in MODES.items():
        ev.track_refine(preds, boxes, fmap, tracks, device=dev, **kw)    # warm-up
        ts = []
        for _ in range(a.rounds):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            got = ev.track_refine(preds, boxes, fmap, tracks, device=dev, **kw)
            ts.append((time.perf_counter() - t0) * 1e3)
        rec = {'end_to_end': _stats(ts, 'ms')}
        if mode != 'default':                                   # (the loop over windows of 33 takes minutes: one setting is compared)
            out[mode] = rec
            continue
        t0 = time.perf_counter()
        ref = rr.track_refine_ref(preds, boxes, fmap, tracks, **kw)
        rec['numpy_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
        rec['numpy_over_end_to_end'] = round(rec['numpy_ms'] / rec['end_to_end']['ms'], 1)
        same = lambda x, y: x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()  # noqa: E731
        rec['outputs_equal'] = bool(same(got[0], ref['preds2']) and same(got[1], ref['boxes2']) and got[2] == ref['fmap2'] and
                                    list(got[2]) == list(ref['fmap2']) and same(got[3], ref['tracks2']))
        out[mode] = rec
    # the metrics of a set with known truth (synthetic)
    import _track_ref as tr
    gt, seq_ids, mp, mb, mfmap = metric_set(a.metric_seqs)
    mtracks, mnum = ev.pose_track(mp, mb, mfmap, sigmas=tr.SIGMAS15, device=dev)
    rec = {'label': 'SYNTHETIC set with known truth (see the module docstring); reported, not asserted', 'sequences': a.metric_seqs,
           'detections': len(mp), 'ids': int(sum(mnum.values())),
           'tracked': metrics(ev, gt, seq_ids, mp, mb, mfmap, mtracks, dev)}
    for name, kw in (('refined_defaults', {}), ('refined_rescore_min_len3', dict(rescore=True, min_len=3)),
                     ('fill_only', dict(smooth_radius=0)), ('smooth_only', dict(max_fill=0))):
        p2, b2, m2, t2 = ev.track_refine(mp, mb, mfmap, mtracks, device=dev, **kw)
        rec[name] = metrics(ev, gt, seq_ids, p2, b2, m2, t2, dev)
        rec[name]['new_rows'] = len(p2) - len(mp)
    out['metrics'] = rec
    if a.parent:
        out['bench_py'] = bench_parity(a.parent, a.bench_steps, a.bench_warmup)
    else:
        out['bench_py'] = 'not measured (no --parent checkout given)'
    line = json.dumps(out)
    print(line)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, 'bench_refine.json'), 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
