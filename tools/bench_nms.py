"""What pose rescoring + OKS-NMS costs on a synthetic set of validation-set size: the kernel fami_pose_nms_f32 back to
back and with cold caches, `evaluate.pose_nms` end to end, and the way a user had to do it before: the numpy loop over
every frame (tests/_nms_ref.pose_nms_ref, the float64 restatement of the reference's functions) on the same input.

    python tools/bench_nms.py [--frames 20000] [--reps 50] [--rounds 5] [--out profiles/nms]

Sizes: `--frames` frames (default 20000) with 1 ... 16 detections each (uniform; mean 8.5, so about 170000 detections of 17
joints: a video validation split run on detector boxes is of this order), made by tests/_nms_ref.make_dets frame by
frame (clusters of near-duplicate poses, so that NMS has something to suppress), plus one frame of 256 detections, the
kernel's cap, which is the longest chain of dependent rounds a launch can contain (`kernel_hard_without_largest` is the
same launch without that last workgroup: the difference is what its chain adds to the tail).  Modes: hard (IN_VIS_THRE 0.2,
OKS_THRE 0.9: Base_PoseTrack17.yaml) and soft (same thresholds, max_dets 20).

kernel: device events around `--reps` launches on resident inputs, the modes alternating over `--rounds` rounds, median
and min..max in us per launch; COLD = single launches, each behind a 1 GiB fill that evicts the inputs from the caches.
One workgroup per frame; `bytes` is what a launch must read and write once (inputs + outputs).  No share of a peak is
quoted: each workgroup is a chain of dependent pick rounds, and the launch is sized by that latency and by the number
of workgroups per CU, not by bandwidth or arithmetic.
end_to_end: `pose_nms` on the host arrays (validation, packing, one upload, the launch, one download, the keep lists),
host clock around calls that end with the download, median of `--rounds` calls.
numpy: one call of the restatement on the same arrays (host clock).  The results of both are compared: `frames_differing`
counts frames whose keep list differs (the restatement's smallest decision margin on this unselected input is printed
beside it: a frame can only differ where a decision is closer than the rounding of an OKS).
Prints one JSON line and writes it to <out>/bench_nms.json.  Needs the GPU."""
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

MODES = {'hard': dict(in_vis_thre=0.2, oks_thre=0.9), 'soft': dict(in_vis_thre=0.2, oks_thre=0.9, soft=True, max_dets=20)}


def make_set(frames, seed=1):
    """-> preds [N,17,3], boxes [N,6] float64 (fp32 values), filenames_map; the last frame has 256 detections."""
    import _nms_ref as nr
    rng = np.random.RandomState(seed)
    sizes = list(rng.randint(1, 17, frames)) + [256]
    parts = [nr.make_dets(rng, int(n)) for n in sizes]
    preds = np.concatenate([p[0] for p in parts]).astype(np.float64)
    boxes = np.zeros((len(preds), 6))
    boxes[:, 4] = np.concatenate([p[1] for p in parts])
    boxes[:, 5] = np.concatenate([p[2] for p in parts])
    seg = np.concatenate([[0], np.cumsum(sizes)])
    fmap = {'images/val/v%05d/%08d.jpg' % (m // 100, m % 100 + 1): list(range(int(seg[m]), int(seg[m + 1])))
            for m in range(len(sizes))}
    return preds, boxes, fmap


def _stats(ts, unit):
    return {unit: round(statistics.median(ts), 2), 'min_' + unit: round(min(ts), 2), 'max_' + unit: round(max(ts), 2)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--frames', type=int, default=20000)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'nms'))
    a = ap.parse_args()
    if a.frames < 1 or a.reps < 1:
        ap.error('--frames and --reps must be >= 1')
    if a.rounds < 5:
        ap.error('--rounds must be >= 5: the spread between rounds is part of the result')
    preds, boxes, fmap = make_set(a.frames)
    N, J, M = len(preds), preds.shape[1], len(fmap)
    if not torch.cuda.is_available():
        raise SystemExit('bench_nms needs the GPU (the set is %d detections in %d frames)' % (N, M))
    import _nms_ref as nr
    from fami_pose_amd import evaluate as ev
    from fami_pose_amd._lib import lib
    dev = torch.device('cuda:0')
    s = torch.cuda.current_stream(dev).cuda_stream
    index, seg = ev._nms_lists(fmap, N)
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)  # noqa: E731
    ins = [up(preds, np.float32), up(boxes[:, 4], np.float32), up(boxes[:, 5], np.float32), up(ev.COCO_SIGMAS, np.float32),
           up(index, np.int32), up(seg, np.int32)]
    outs = [torch.empty(N, device=dev), torch.empty(N, dtype=torch.int32, device=dev), torch.empty(M, dtype=torch.int32, device=dev)]
    junk = torch.empty(1 << 28, device=dev)                    # 1 GiB: four times the Infinity Cache

    def launcher(kw, M=M):
        vis = kw.get('vis_thre')
        args = [t.data_ptr() for t in ins] + [N, J, M, kw['in_vis_thre'], kw['oks_thre'], 1 if kw.get('soft') else 0,
                                              kw.get('max_dets', 20), 0.0 if vis is None else vis, 0 if vis is None else 1]
        args += [t.data_ptr() for t in outs] + [s]
        return lambda: lib().call('fami_pose_nms_f32', *args)

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

    out = {'tool': 'bench_nms', 'device': torch.cuda.get_device_name(dev), 'frames': M, 'detections': N, 'joints': J,
           'largest_frame': 256, 'reps': a.reps, 'rounds': a.rounds,
           'bytes': 4 * (N * J * 3 + 2 * N + J + N + M + 1 + 2 * N + M), 'workgroups': M,
           'bound': 'latency of the dependent pick rounds (no share of peak quoted)'}
    fns = {k: launcher(kw) for k, kw in MODES.items()}
    fns['hard_without_largest'] = launcher(MODES['hard'], M - 1)   # the frame of 256 is the last workgroup: leave it out
    for fn in fns.values():
        window(fn, 5)
    us = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, fn in fns.items():
            us[k].append(window(fn, a.reps))
    for k, fn in fns.items():
        rec = _stats(us[k], 'us')
        outs[2].zero_()                                         # `kept` below counts this launcher's frames only
        c = cold(fn, 11)
        rec.update({'cold_us': round(statistics.median(c), 2), 'cold_min_us': round(min(c), 2), 'cold_max_us': round(max(c), 2)})
        torch.cuda.synchronize(dev)
        rec['kept'] = int(outs[2].clamp(min=0).sum().item())
        out['kernel_' + k] = rec
    del junk
    for k, kw in MODES.items():
        ev.pose_nms(preds, boxes, fmap, device=dev, **kw)      # warm-up
        ts = []
        for _ in range(a.rounds):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            scores, keep = ev.pose_nms(preds, boxes, fmap, device=dev, **kw)
            ts.append((time.perf_counter() - t0) * 1e3)
        rec = {'end_to_end': _stats(ts, 'ms')}
        t0 = time.perf_counter()
        ref = nr.pose_nms_ref(preds, boxes, fmap, **kw)
        rec['numpy_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
        rec['numpy_over_end_to_end'] = round(rec['numpy_ms'] / rec['end_to_end']['ms'], 1)
        rec['frames_differing'] = sum(keep[key] != ref['keep_map'][key] for key in fmap)
        rec['scores_bit_equal'] = bool(np.array_equal(scores.astype(np.float32).view(np.int32),
                                                      ref['scores'].astype(np.float32).view(np.int32)))
        rec['smallest_margin'] = float(ref['margin'])
        out[k] = rec
    line = json.dumps(out)
    print(line)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, 'bench_nms.json'), 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
