"""What the PoseTrack MOTA costs on a synthetic set of validation-set size: the MOT launch (fami_posetrack_mot_f64 with
its closing fami_posetrack_mot_final_f64) back to back and with cold caches, `evaluate.posetrack_mota` end to end,
`pack_posetrack_frames(..., seq_ids)` alone (Python over dicts: reported, not hidden), and the way a user had to do it
before: the per-frame loop on the host (tests/_mota_ref.evaluate_mota with margins=False, the float64 restatement of the
reference's assignGTmulti lists and MOTAccumulator.update -- numpy distances and scipy's linear_sum_assignment where the
reference runs Python loops and a pandas row insert per event, so it flatters the host side).

    python tools/bench_mota.py [--seqs 50] [--frames 150] [--reps 50] [--rounds 5] [--out profiles/mota]

Sizes: `--seqs` seeded sequences of `--frames` frames (tests/_mota_ref.make_sequences: 2 .. 4 people with persistent
ids, dropped, doubled and spurious predictions, id swaps; PoseTrack17 val has 50 sequences) plus one sequence of two
frames whose first has 64 annotated and 256 predicted poses, the caps: the longest single update a launch can contain.
The launch is one 64-lane wavefront per (sequence, joint) that walks the sequence's frames in order, so its time is set
by the LONGEST CHAIN (`longest_chain_frames`), not by the number of chains (`chains`).
kernel: device events around `--reps` launches on resident inputs over `--rounds` rounds, median and min..max in us per
launch; COLD = single launches, each behind a 1 GiB fill that evicts the inputs from the caches.  No share of a peak is
quoted: the launch is latency bound (dependent frames, a handful of poses each).
end_to_end: `posetrack_mota` on the packed arrays (one upload, the assign launch, the two MOT launches, one download),
host clock around calls that end with the download, median of `--rounds` calls.
host: one call each of pack_posetrack_frames and of the restatement's loop (host clock, `--rounds` runs of the loop for
its spread).  The device counts are compared with the restatement's: `counts_differing` counts (sequence, joint, count)
entries -- on this unselected input a decision may lie within rounding (the restatement's margins are printed beside).
Prints one JSON line and writes it to <out>/bench_mota.json.  Needs the GPU."""
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


def make_set(seqs, frames, seed=1):
    """-> (gt_annolist, pr_annolist, seq_ids); the last sequence has a frame of 64 annotated x 256 predicted poses."""
    import _ap_ref as ar
    import _mota_ref as mr
    rng = np.random.RandomState(seed)
    gt, pr, seq = mr.make_sequences(rng, seqs, frames)
    g_rects, p_rects = [], []
    for i in range(64):
        xy, present, head, size = ar.make_person(rng)
        g_rects.append(ar.gt_rect(xy, present, head, i))
        for _ in range(4):
            p_rects.append(ar.pr_rect(*ar.make_prediction(rng, xy, size, rng.uniform(0.05, 0.45)), track_id=len(p_rects)))
    for _ in range(2):
        gt.append({'annorect': g_rects})
        pr.append({'annorect': p_rects})
        seq.append(seqs)
    return gt, pr, seq


def _stats(ts, unit):
    return {unit: round(statistics.median(ts), 2), 'min_' + unit: round(min(ts), 2), 'max_' + unit: round(max(ts), 2)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--seqs', type=int, default=50)
    ap.add_argument('--frames', type=int, default=150)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mota'))
    a = ap.parse_args()
    if a.seqs < 1 or a.frames < 2 or a.reps < 1:
        ap.error('--seqs and --reps must be >= 1, --frames >= 2')
    if a.rounds < 5:
        ap.error('--rounds must be >= 5: the spread between rounds is part of the result')
    import _mota_ref as mr
    from fami_pose_amd import evaluate as ev
    from fami_pose_amd._lib import lib
    gt, pr, seq = make_set(a.seqs, a.frames)
    host = {}
    t0 = time.perf_counter()
    k = ev.pack_posetrack_frames(gt, pr, seq)
    host['pack_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
    P, G, F, S = len(k['pr_has']), len(k['gt_has']), len(k['pr_seg']) - 1, len(k['seq_seg']) - 1
    longest = int(np.diff(k['seq_seg']).max()) - 1
    if not torch.cuda.is_available():
        raise SystemExit('bench_mota needs the GPU (the set is %d predicted / %d annotated poses in %d frames of %d '
                         'sequences; the pack took %.0f ms here)' % (P, G, F, S, host['pack_ms']))
    dev = torch.device('cuda:0')
    s = torch.cuda.current_stream(dev).cuda_stream
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt).reshape(-1)).to(dev)  # noqa: E731
    f64 = [up(k[n], np.float64) for n in ('pr_xys', 'gt_xy', 'gt_head', 'verts')]
    i32 = {n: up(k[n], np.int32) for n in ('pr_has', 'gt_has', 'pr_seg', 'gt_seg', 'poly_seg', 'vert_seg', 'pr_track',
                                           'gt_track', 'seq_seg')}
    outs = [torch.empty(max(n, 1), dtype=torch.int32, device=dev) for n in (P, G, P, P, F * 15)]
    lib().call('fami_posetrack_assign_f64', f64[0].data_ptr(), i32['pr_has'].data_ptr(), f64[1].data_ptr(),
               i32['gt_has'].data_ptr(), f64[2].data_ptr(), i32['pr_seg'].data_ptr(), i32['gt_seg'].data_ptr(),
               i32['poly_seg'].data_ptr(), i32['vert_seg'].data_ptr(), f64[3].data_ptr(), P, G, F, 0, 0, 0.5,
               *[t.data_ptr() for t in outs], s)
    counts = torch.empty(S * 75, dtype=torch.int32, device=dev)
    status, totals = torch.empty(S, dtype=torch.int32, device=dev), torch.empty(75, dtype=torch.int32, device=dev)
    sumd, fin = torch.empty(S * 15, dtype=torch.float64, device=dev), torch.empty(15 + 64, dtype=torch.float64, device=dev)
    junk = torch.empty(1 << 28, device=dev)                    # 1 GiB: four times the Infinity Cache

    def mot():
        lib().call('fami_posetrack_mot_f64', f64[0].data_ptr(), outs[0].data_ptr(), f64[1].data_ptr(), outs[1].data_ptr(),
                   f64[2].data_ptr(), i32['pr_seg'].data_ptr(), i32['gt_seg'].data_ptr(), i32['poly_seg'].data_ptr(),
                   i32['pr_track'].data_ptr(), i32['gt_track'].data_ptr(), i32['seq_seg'].data_ptr(), P, G, F, S, 0.5,
                   counts.data_ptr(), sumd.data_ptr(), status.data_ptr(), s)
        lib().call('fami_posetrack_mot_final_f64', counts.data_ptr(), sumd.data_ptr(), status.data_ptr(), S,
                   totals.data_ptr(), fin.data_ptr(), fin[15:].data_ptr(), s)

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

    out = {'tool': 'bench_mota', 'device': torch.cuda.get_device_name(dev), 'sequences': S, 'frames': F,
           'predicted_poses': P, 'annotated_poses': G, 'chains': S * 15, 'longest_chain_frames': longest,
           'largest_frame': [256, 64], 'reps': a.reps, 'rounds': a.rounds,
           'bound': 'latency of the longest chain of dependent frames (no share of peak quoted)'}
    window(mot, 5)
    us = [window(mot, a.reps) for _ in range(a.rounds)]
    rec = _stats(us, 'us')
    c = cold(mot, 11)
    rec.update({'cold_us': round(statistics.median(c), 2), 'cold_min_us': round(min(c), 2), 'cold_max_us': round(max(c), 2),
                'us_per_frame_of_longest_chain': round(statistics.median(us) / max(longest, 1), 3), 'workgroups': S * 15})
    out['kernel_mot'] = rec
    del junk
    ev.posetrack_mota(k, device=dev)                               # warm-up
    ts = []
    for _ in range(a.rounds):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        got = ev.posetrack_mota(k, device=dev)
        ts.append((time.perf_counter() - t0) * 1e3)
    out['end_to_end'] = _stats(ts, 'ms')
    ts = []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        mr.evaluate_mota(gt, pr, seq, margins=False)
        ts.append((time.perf_counter() - t0) * 1e3)
    host['restatement_loop'] = _stats(ts, 'ms')
    host['loop_over_end_to_end'] = round(host['restatement_loop']['ms'] / out['end_to_end']['ms'], 1)
    out['host'] = host
    ref = mr.evaluate_mota(gt, pr, seq)
    out['counts_differing'] = int((got['per_seq'] != ref['per_seq']).sum())
    out['metric_max_abs_diff'] = float(max(np.nanmax(np.abs(got[n] - ref[n])) for n in ('mota', 'motp', 'pre', 'rec')))
    out['smallest_threshold_margin'], out['smallest_uniqueness_margin'] = float(ref['thr_margin']), float(ref['uniq_margin'])
    out['problems'] = int(ref['problems'])
    out['total'] = {n: float(got[n][15]) for n in ('mota', 'motp', 'pre', 'rec')}
    line = json.dumps(out)
    print(line)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, 'bench_mota.json'), 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
