"""What OKS pose tracking costs on a synthetic set of validation-set size: the kernel fami_pose_track_f32 back to back and
with cold caches, `evaluate.pose_track` end to end, and the way a user had to do it otherwise: the numpy loop over every
video (tests/_track_ref.pose_track_ref, the float64 restatement of the rule) on the same input.

    python tools/bench_track.py [--videos 200] [--frames 100] [--reps 20] [--rounds 5] [--out profiles/track]

Sizes: `--videos` videos (default 200) of `--frames` frames (default 100) with 2 ... 14 people each on the trajectories of
tests/_track_ref.make_video (dropouts, crossings, false positives), about 144000 detections of 17 joints in 20000 frames:
a video validation split after pose NMS is of this order; plus one video of two frames with 256 people each, the
kernel's cap (`kernel_without_largest` is the same launch without that last workgroup).  Settings: the defaults
(oks_thre 0.3, max_gap 3) and max_gap 1.

kernel: device events around `--reps` launches on resident inputs, the settings alternating over `--rounds` rounds,
median and min..max in us per launch; COLD = single launches, each behind a 1 GiB fill that evicts the inputs from the
caches.  One workgroup per video; `bytes` is what a launch must read and write once (inputs + outputs).  No share of a
peak is quoted: each workgroup is a chain of one dependent round per detection of its video, and the launch is sized by
that latency and by the longest video, not by bandwidth or arithmetic; `rounds_longest_video` is that chain.
end_to_end: `pose_track` on the host arrays (validation, the frame tables, one upload, the launch, one download), host
clock around calls that end with the download, median of `--rounds` calls.
numpy: one call of the restatement on the same arrays (host clock).  The results of both are compared: `rows_differing`
counts detections whose id differs (the restatement's smallest decision margin on this unselected input is printed
beside it: an id can only differ where a decision is closer than the rounding of an OKS, and one flip renumbers what
follows it in the video).
Prints one JSON line and writes it to <out>/bench_track.json.  Needs the GPU."""
import argparse
import json
import os
import statistics
import sys
import time

os.environ.setdefault('HIP_FORCE_DEV_KERNARG', '1')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

MODES = {'default': dict(oks_thre=0.3, max_gap=3), 'gap1': dict(oks_thre=0.3, max_gap=1)}


def make_set(videos, frames, seed=1):
    """-> preds [N,17,3], boxes [N,6] float64 (fp32 values), filenames_map; the last video has 2 frames of 256 people."""
    import _track_ref as tr
    rng = np.random.RandomState(seed)
    vids = {'val/v%05d' % i: tr.make_video(rng, int(rng.randint(2, 15)), list(range(1, frames + 1))) for i in range(videos)}
    vids['val/w_largest'] = tr.make_video(rng, 256, [1, 2], drop=0, fp_rate=0, jitter=0.5, speed=2.0, cross=False)  # all re-found
    preds, boxes, fmap = tr.scatter(rng, vids, 17)
    return preds, boxes, {k: fmap[k] for k in sorted(fmap)}       # videos contiguous, the largest one last


def _stats(ts, unit):
    return {unit: round(statistics.median(ts), 2), 'min_' + unit: round(min(ts), 2), 'max_' + unit: round(max(ts), 2)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--videos', type=int, default=200)
    ap.add_argument('--frames', type=int, default=100)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'track'))
    a = ap.parse_args()
    if a.videos < 1 or a.frames < 1 or a.reps < 1:
        ap.error('--videos, --frames and --reps must be >= 1')
    if a.rounds < 5:
        ap.error('--rounds must be >= 5: the spread between rounds is part of the result')
    preds, boxes, fmap = make_set(a.videos, a.frames)
    N, J = len(preds), preds.shape[1]
    import _track_ref as tr
    from fami_pose_amd import evaluate as ev
    index, fseg, fnum, vseg, videos = ev._track_tables(fmap, N)
    M, V, n = len(fnum), len(videos), len(index)
    assert videos[-1] == 'val/w_largest'
    if not torch.cuda.is_available():
        raise SystemExit('bench_track needs the GPU (the set is %d detections in %d frames of %d videos)' % (N, M, V))
    from fami_pose_amd._lib import lib
    dev = torch.device('cuda:0')
    s = torch.cuda.current_stream(dev).cuda_stream
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)  # noqa: E731
    ins = [up(preds, np.float32), up(boxes[:, 4], np.float32), up(ev.COCO_SIGMAS, np.float32), up(index, np.int32),
           up(fseg, np.int32), up(fnum, np.int32), up(vseg, np.int32)]
    outs = [torch.empty(N, dtype=torch.int32, device=dev), torch.empty(V, dtype=torch.int32, device=dev)]
    junk = torch.empty(1 << 28, device=dev)                    # 1 GiB: four times the Infinity Cache

    def launcher(kw, V=V):
        args = [t.data_ptr() for t in ins] + [N, J, n, M, V, kw['oks_thre'], kw['max_gap'], 0.0, 0]
        args += [t.data_ptr() for t in outs] + [s]
        return lambda: lib().call('fami_pose_track_f32', *args)

    def window(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps

    def cold(fn, reps):
        ts = []
        for r in range(reps):
            junk.fill_(float(r))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        return ts

    per_video = np.diff(fseg[vseg])
    out = {'tool': 'bench_track', 'device': torch.cuda.get_device_name(dev), 'videos': V, 'frames': M, 'detections': N,
           'joints': J, 'largest_frame': 256, 'rounds_longest_video': int(per_video.max()), 'reps': a.reps, 'rounds': a.rounds,
           'bytes': 4 * (N * J * 3 + N + J + n + M + 1 + M + V + 1 + N + V), 'workgroups': V,
           'bound': 'latency of the dependent rounds of the longest video (no share of peak quoted)'}
    fns = {k: launcher(kw) for k, kw in MODES.items()}
    fns['without_largest'] = launcher(MODES['default'], V - 1)     # the video of 2 x 256 is the last workgroup: leave it out
    for fn in fns.values():
        window(fn, 3)
    us = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, fn in fns.items():
            us[k].append(window(fn, a.reps))
    for k, fn in fns.items():
        rec = _stats(us[k], 'us')
        outs[1].zero_()                                         # `ids` below counts this launcher's videos only
        c = cold(fn, 11)
        rec.update({'cold_us': round(statistics.median(c), 2), 'cold_min_us': round(min(c), 2), 'cold_max_us': round(max(c), 2)})
        torch.cuda.synchronize(dev)
        rec['ids'] = int(outs[1].clamp(min=0).sum().item())
        out['kernel_' + k] = rec
    del junk
    for k, kw in MODES.items():
        ev.pose_track(preds, boxes, fmap, device=dev, **kw)    # warm-up
        ts = []
        for _ in range(a.rounds):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            tracks, num = ev.pose_track(preds, boxes, fmap, device=dev, **kw)
            ts.append((time.perf_counter() - t0) * 1e3)
        rec = {'end_to_end': _stats(ts, 'ms')}
        t0 = time.perf_counter()
        ref = tr.pose_track_ref(preds, boxes, fmap, **kw)
        rec['numpy_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
        rec['numpy_over_end_to_end'] = round(rec['numpy_ms'] / rec['end_to_end']['ms'], 1)
        rec['rows_differing'] = int((tracks != ref['tracks']).sum())
        rec['videos_differing'] = sum(num[v] != ref['num_tracks'][v] for v in num)
        rec['smallest_margin'] = float(ref['margin'])
        rec['stats'] = ref['stats']
        out[k] = rec
    line = json.dumps(out)
    print(line)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, 'bench_track.json'), 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
