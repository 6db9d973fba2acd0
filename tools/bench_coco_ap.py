"""What the COCO keypoint AP costs on a synthetic set of val2017 size: the two kernels (fami_coco_kpt_match_f64,
fami_coco_kpt_curve_f64) back to back and with cold caches, `evaluate.coco_keypoint_ap` end to end, `pack_coco_keypoints`
alone (Python over dicts: reported, not hidden), and the way a user without pycocotools had to do it: the per-image
matching loop on the host (tests/_coco_ref.match_image, the float64 restatement of computeOks + evaluateImg).

    python tools/bench_coco_ap.py [--images 5000] [--reps 50] [--rounds 5] [--out profiles/coco_ap]

Sizes: `--images` seeded images (tests/_coco_ref.seeded_set scaled up: 0 .. 4 annotated people, a quarter of them twice,
detections at three noise levels and of nobody, padded with low-scored detections of nobody to about 20 per image, so
about 100 000 detections go in) plus one image at the caps (256 detections, 128 annotations), the longest workgroup a
launch can contain.  max_dets 20.
kernel: device events around `--reps` launches on resident inputs, the two kernels alternating over `--rounds` rounds,
median and min..max in us per launch; COLD = single launches, each behind a 1 GiB fill that evicts the inputs from the
caches.  `bytes` is what a launch must read and write once.  No share of a peak is quoted: the match is one short
workgroup per image (launch-rate and latency bound, fp64 divisions and exp), the curve 30 workgroups of dependent scans.
end_to_end: `coco_keypoint_ap` on the packed arrays (one upload, the match, torch's stable sort and gather, the curve,
one download), host clock around calls that end with the download, median of `--rounds` calls.
host: one call each of pack_coco_keypoints and of the restatement's whole evaluation (host clock).  The device result is
compared with the restatement's: `precision_differing` / `recall_differing` count entries that are not bit-equal (the
restatement's smallest decision margins on this input are printed beside them).
Prints one JSON line and writes it to <out>/bench_coco_ap.json.  Needs the GPU."""
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


def make_set(images, per_image=20, seed=1):
    """-> (gt_anns, dt_anns, img_ids); the last image has 128 annotations and 256 detections."""
    import _coco_ref as cr
    gt, dt, ids = cr.seeded_set(seed, images)
    rng = np.random.default_rng(seed + 1)
    have = np.bincount([d['image_id'] for d in dt], minlength=images)
    for im in range(images):
        for _ in range(max(0, per_image - int(have[im]))):
            nobody = cr.person(rng, rng.uniform(50, 600), rng.uniform(50, 400), float(rng.choice([70, 150, 300])), image_id=im)
            dt.append(cr.det_of(nobody, rng.uniform() * 0.3))
    cgt, cdt, _ = cr.caps_set(seed + 2)
    gt += [dict(g, image_id=images) for g in cgt if g['image_id'] == 1]
    dt += [dict(d, image_id=images) for d in cdt if d['image_id'] == 1]
    return gt, dt, ids + [images]


def _stats(ts, unit):
    return {unit: round(statistics.median(ts), 2), 'min_' + unit: round(min(ts), 2), 'max_' + unit: round(max(ts), 2)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--images', type=int, default=5000)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'coco_ap'))
    a = ap.parse_args()
    if a.images < 1 or a.reps < 1:
        ap.error('--images and --reps must be >= 1')
    if a.rounds < 5:
        ap.error('--rounds must be >= 5: the spread between rounds is part of the result')
    import _coco_ref as cr
    from fami_pose_amd import evaluate as ev
    from fami_pose_amd._lib import lib
    gt, dt, ids = make_set(a.images)
    host = {}
    t0 = time.perf_counter()
    k = ev.pack_coco_keypoints(gt, dt, img_ids=ids)
    host['pack_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
    G, D, M, J, K = len(k['gt_flags']), len(k['dt_score']), len(ids), 17, ev.COCO_MAX_DETS
    T, R, A = len(ev.COCO_IOU_THRS), len(ev.COCO_REC_THRS), len(ev.COCO_AREA_RNGS)
    if not torch.cuda.is_available():
        raise SystemExit('bench_coco_ap needs the GPU (the set is %d annotations / %d detections in %d images; the pack took '
                         '%.0f ms here)' % (G, D, M, host['pack_ms']))
    dev = torch.device('cuda:0')
    s = torch.cuda.current_stream(dev).cuda_stream
    up = lambda x, dt_: torch.from_numpy(np.ascontiguousarray(x, dtype=dt_).reshape(-1)).to(dev)  # noqa: E731
    names = ('gt_kpts', 'gt_area', 'gt_bbox', 'gt_flags', 'dt_kpts', 'dt_score', 'dt_area', 'gt_seg', 'dt_seg')
    ins = [up(k[n], np.int32 if n in ('gt_flags', 'gt_seg', 'dt_seg') else np.float64) for n in names]
    var = np.ascontiguousarray((ev.COCO_SIGMAS * 2) ** 2)
    iou, rec, rng = (np.ascontiguousarray(x) for x in (ev.COCO_IOU_THRS, ev.COCO_REC_THRS, ev.COCO_AREA_RNGS))
    out_score = torch.empty(M * K, dtype=torch.float64, device=dev)
    out_row = torch.empty(M * K, dtype=torch.int32, device=dev)
    out_flags = torch.empty(M * K, A * T, dtype=torch.uint8, device=dev)
    npig = torch.empty(M * A, dtype=torch.int32, device=dev)
    res = torch.empty(T * R * A + T * A, dtype=torch.float64, device=dev)
    junk = torch.empty(1 << 28, device=dev)                    # 1 GiB: four times the Infinity Cache
    match = lambda: lib().call('fami_coco_kpt_match_f64', *[t.data_ptr() for t in ins], var.ctypes.data, iou.ctypes.data,  # noqa: E731
                               rng.ctypes.data, G, D, M, J, T, A, K, out_score.data_ptr(), out_row.data_ptr(),
                               out_flags.data_ptr(), npig.data_ptr(), s)
    match()
    # the curve's input, made once as coco_keypoint_ap makes it
    slot = torch.nonzero(out_row >= 0).reshape(-1)
    order = torch.sort(out_score[slot], descending=True, stable=True).indices
    flags = out_flags[slot[order]].t().contiguous()
    N = int(slot.numel())
    curve = lambda: lib().call('fami_coco_kpt_curve_f64', flags.data_ptr(), npig.data_ptr(), rec.ctypes.data, N, M, T, A, R,  # noqa: E731
                               res.data_ptr(), res.data_ptr() + 8 * T * R * A, s)

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

    out = {'tool': 'bench_coco_ap', 'device': torch.cuda.get_device_name(dev), 'images': M, 'annotations': G,
           'detections': D, 'kept_detections': N, 'largest_image': [256, 128], 'max_dets': K, 'reps': a.reps,
           'rounds': a.rounds, 'bound': 'launch rate and latency of short workgroups (no share of peak quoted)'}
    fns = {'match': match, 'curve': curve}
    nbytes = {'match': 8 * (G * (J * 3 + 5) + D * (J * 3 + 2)) + 4 * (G + 2 * (M + 1)) + M * K * (12 + A * T) + 4 * M * A,
              'curve': A * T * N + 4 * M * A * T + 8 * (T * R * A + T * A)}
    for fn in fns.values():
        window(fn, 5)
    us = {n: [] for n in fns}
    for _ in range(a.rounds):
        for n, fn in fns.items():
            us[n].append(window(fn, a.reps))
    for n, fn in fns.items():
        r = _stats(us[n], 'us')
        c = cold(fn, 11)
        r.update({'cold_us': round(statistics.median(c), 2), 'cold_min_us': round(min(c), 2), 'cold_max_us': round(max(c), 2),
                  'bytes': nbytes[n], 'workgroups': M if n == 'match' else A * T})
        out['kernel_' + n] = r
    del junk
    ev.coco_keypoint_ap(k, device=dev)                         # warm-up
    ts = []
    for _ in range(a.rounds):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        got = ev.coco_keypoint_ap(k, device=dev)
        ts.append((time.perf_counter() - t0) * 1e3)
    out['end_to_end'] = _stats(ts, 'ms')
    t0 = time.perf_counter()
    ref = cr.evaluate(gt, dt, img_ids=ids)
    host['restatement_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
    host['restatement_over_end_to_end'] = round(host['restatement_ms'] / out['end_to_end']['ms'], 1)
    out['host'] = host
    bits = lambda x: np.ascontiguousarray(x, dtype=np.float64).view(np.int64)  # noqa: E731
    out['precision_differing'] = int((bits(got['precision']) != bits(ref['precision'])).sum())
    out['recall_differing'] = int((bits(got['recall']) != bits(ref['recall'])).sum())
    out['smallest_margin'], out['smallest_tie_margin'] = float(ref['margin']), float(ref['tie_margin'])
    out['stats'] = [round(float(v), 6) for v in got['stats']]
    line = json.dumps(out)
    print(line)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, 'bench_coco_ap.json'), 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
