"""What the PoseTrack AP costs on a synthetic set of validation-set size: the two kernels (fami_posetrack_assign_f64,
fami_posetrack_curve_f64) back to back and with cold caches, `evaluate.posetrack_ap` end to end, `pack_posetrack_frames`
alone (Python over dicts: reported, not hidden), and the way a user had to do it before: the matching loop over every frame
on the host (tests/_ap_ref.match_frame, the float64 restatement of the reference's assignGTmulti, which is vectorised per
frame where the reference runs triple Python loops -- so it flatters the host side).

    python tools/bench_ap.py [--frames 20000] [--reps 50] [--rounds 5] [--out profiles/ap]

Sizes: `--frames` seeded frames (tests/_ap_ref.make_annolists: 0 ... 4 annotated people, detections, twins and false
positives; frames without an annotated person are dropped by the selection) plus one frame of 256 predictions against 64
annotated poses, the caps, which is the longest workgroup a launch can contain.
kernel: device events around `--reps` launches on resident inputs, the two kernels alternating over `--rounds` rounds,
median and min..max in us per launch; COLD = single launches, each behind a 1 GiB fill that evicts the inputs from the
caches.  `bytes` is what a launch must read and write once.  No share of a peak is quoted: the assignment is one short
workgroup per frame (launch-rate and latency bound), the curve 15 workgroups of dependent scans.
end_to_end: `posetrack_ap` on the packed arrays (one upload, the assignment, torch's stable sort and gathers, the curve,
one download), host clock around calls that end with the download, median of `--rounds` calls.
host: one call each of pack_posetrack_frames, _ap_ref.select_frames and the match_frame loop (host clock).  The device
result is compared with the restatement's: `label_differing` / `assigned_differing` count poses, `ap_max_abs_diff` is on
the 0-100 scale (the restatement's smallest decision margin on this unselected input is printed beside them).
Prints one JSON line and writes it to <out>/bench_ap.json.  Needs the GPU."""
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


def make_set(frames, seed=1):
    """-> (gt_annolist, pr_annolist); the last frame has 64 annotated poses and 256 predictions."""
    import _ap_ref as ar
    rng = np.random.RandomState(seed)
    gt, pr = ar.make_annolists(rng, frames)
    g_rects, p_rects = [], []
    for i in range(64):
        xy, present, head, size = ar.make_person(rng)
        g_rects.append(ar.gt_rect(xy, present, head, i))
        for _ in range(4):
            p_rects.append(ar.pr_rect(*ar.make_prediction(rng, xy, size, rng.uniform(0.05, 0.9)), track_id=len(p_rects)))
    gt.append({'annorect': g_rects})
    pr.append({'annorect': p_rects})
    return gt, pr


def _stats(ts, unit):
    return {unit: round(statistics.median(ts), 2), 'min_' + unit: round(min(ts), 2), 'max_' + unit: round(max(ts), 2)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--frames', type=int, default=20000)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ap'))
    a = ap.parse_args()
    if a.frames < 1 or a.reps < 1:
        ap.error('--frames and --reps must be >= 1')
    if a.rounds < 5:
        ap.error('--rounds must be >= 5: the spread between rounds is part of the result')
    import _ap_ref as ar
    from fami_pose_amd import evaluate as ev
    from fami_pose_amd._lib import lib
    gt, pr = make_set(a.frames)
    host = {}
    t0 = time.perf_counter()
    k = ev.pack_posetrack_frames(gt, pr)
    host['pack_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
    P, G, F = len(k['pr_has']), len(k['gt_has']), len(k['pr_seg']) - 1
    if not torch.cuda.is_available():
        raise SystemExit('bench_ap needs the GPU (the set is %d predicted / %d annotated poses in %d frames; the pack took '
                         '%.0f ms here)' % (P, G, F, host['pack_ms']))
    dev = torch.device('cuda:0')
    s = torch.cuda.current_stream(dev).cuda_stream
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt).reshape(-1)).to(dev)  # noqa: E731
    f64 = [up(k[n], np.float64) for n in ('pr_xys', 'gt_xy', 'gt_head', 'verts')]
    i32 = [up(k[n], np.int32) for n in ('pr_has', 'gt_has', 'pr_seg', 'gt_seg', 'poly_seg', 'vert_seg')]
    outs = [torch.empty(max(n, 1), dtype=torch.int32, device=dev) for n in (P, G, P, P, F * 15)]
    res, ngt = torch.empty(48, dtype=torch.float64, device=dev), torch.empty(15, dtype=torch.int32, device=dev)
    junk = torch.empty(1 << 28, device=dev)                    # 1 GiB: four times the Infinity Cache
    a_args = [f64[0].data_ptr(), i32[0].data_ptr(), f64[1].data_ptr(), i32[1].data_ptr(), f64[2].data_ptr(), i32[2].data_ptr(),
              i32[3].data_ptr(), i32[4].data_ptr(), i32[5].data_ptr(), f64[3].data_ptr(), P, G, F, 0, 0, 0.5] + \
             [t.data_ptr() for t in outs] + [s]
    assign = lambda: lib().call('fami_posetrack_assign_f64', *a_args)  # noqa: E731
    assign()
    # the curve's input, made once as posetrack_ap makes it
    bits = torch.arange(15, dtype=torch.int32, device=dev)[:, None]
    present = ((outs[0][None, :P] >> bits) & 1).bool()
    score = f64[0].view(P, 15, 3)[:, :, 2].t()
    order = torch.sort(torch.where(present, score, score.new_tensor(float('-inf'))), dim=1, descending=True, stable=True).indices
    lab = ((outs[2][:P][order] >> bits) & 1).to(torch.uint8).contiguous()
    n_valid = present.sum(1, dtype=torch.int32).contiguous()
    curve = lambda: lib().call('fami_posetrack_curve_f64', lab.data_ptr(), n_valid.data_ptr(), outs[4].data_ptr(), P, F,  # noqa: E731
                               res.data_ptr(), ngt.data_ptr(), s)

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

    out = {'tool': 'bench_ap', 'device': torch.cuda.get_device_name(dev), 'frames': F, 'predicted_poses': P,
           'annotated_poses': G, 'largest_frame': [256, 64], 'reps': a.reps, 'rounds': a.rounds,
           'bound': 'launch rate and latency of short workgroups (no share of peak quoted)'}
    fns = {'assign': assign, 'curve': curve}
    nbytes = {'assign': 8 * (P * 45 + G * 34) + 4 * (2 * P + 2 * G + 3 * (F + 1) + 2 * P + F * 15),
              'curve': 15 * P + 4 * (15 + F * 15) + 8 * 48 + 4 * 15}
    for fn in fns.values():
        window(fn, 5)
    us = {n: [] for n in fns}
    for _ in range(a.rounds):
        for n, fn in fns.items():
            us[n].append(window(fn, a.reps))
    for n, fn in fns.items():
        rec = _stats(us[n], 'us')
        c = cold(fn, 11)
        rec.update({'cold_us': round(statistics.median(c), 2), 'cold_min_us': round(min(c), 2), 'cold_max_us': round(max(c), 2),
                    'bytes': nbytes[n], 'workgroups': F if n == 'assign' else 15})
        out['kernel_' + n] = rec
    del junk
    ev.posetrack_ap(k, device=dev)                             # warm-up
    ts = []
    for _ in range(a.rounds):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        got = ev.posetrack_ap(k, device=dev)
        ts.append((time.perf_counter() - t0) * 1e3)
    out['end_to_end'] = _stats(ts, 'ms')
    t0 = time.perf_counter()
    sel = ar.select_frames(gt, pr)
    host['restatement_select_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
    t0 = time.perf_counter()
    matched = [ar.match_frame(fr) for fr in sel]
    host['restatement_match_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
    host['match_over_end_to_end'] = round(host['restatement_match_ms'] / out['end_to_end']['ms'], 1)
    out['host'] = host
    ref = ar.evaluate_ap(gt, pr)
    out['label_differing'] = int((got['label'] != ref['label']).sum())
    out['assigned_differing'] = int((got['assigned'] != ref['assigned']).sum())
    out['ap_max_abs_diff'] = float(np.nanmax(np.abs(got['ap'] - ref['ap'])))
    out['smallest_margin'] = float(min(m['margin'] for m in matched))
    out['total_ap'] = float(got['ap'][15])
    line = json.dumps(out)
    print(line)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, 'bench_ap.json'), 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
