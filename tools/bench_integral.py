"""What the integral L1 coordinate term costs: the launches between the forward and the backward pass of a training step
(targets, loss, seeds) without and with the term, the integral decode next to the standard one, and the step time of the bench
workload with and without the term.

    python tools/bench_integral.py kernels [--reps 200] [--rounds 5] [--out profiles/integral]
    python tools/bench_integral.py steps [--modes f32,bf16] [--steps 20] [--warmup 5] [--rounds 5] [--out profiles/integral]

kernels: on [4,17,96,72] (the W48 head of a batch of 4), joints as bench.py draws them.
    off       fami_gauss_target_f32, fami_wmse_fwd_f32 (two launches: rows, sum), fami_wmse_bwd_f32
    on        ... + fami_softargmax_fwd_f32, fami_heatmap_xy_f32, fami_integral_l1_fwd_f32 (two launches: rows, sum) behind
              the loss and fami_integral_l1_bwd_f32 (accumulating) behind the seed
    decode    fami_final_preds_f32 (two launches) and fami_softargmax_preds_f32 (one)
Each entry point alone and the seam as a whole.  Device events around `--reps` back-to-back launches, the variants
alternating over `--rounds` rounds, median and min..max in us per call; COLD = single calls, each behind a 1 GiB fill
that evicts the operands from the caches.  All of them are launch-latency-sized: no share of a peak is quoted.

steps: bench.py's workload (W48, 384x288, 4 supporting frames, batch 4, graph replay, targets from joints) per compute
mode: a default Trainer (the launch sequence of a Trainer without the option, launch for launch) and one with
integral_l1_weight=1.0 in ONE process, windows of `--steps` steps alternating between the two over `--rounds` rounds after a
warm-up of both; each window ends in a synchronise (host clock).  The figure to read: `on minus off` against the default's own
min..max spread.  Prints one JSON line per sub-command and writes it to <out>/<sub-command>.json.  Needs the GPU."""
import argparse
import json
import os
import statistics
import sys
import time

os.environ.setdefault('HIP_FORCE_DEV_KERNARG', '1')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

B, S, H, W, J = 4, 4, 384, 288, 17
BETA = 20.0


def _emit(a, name, out):
    line = json.dumps(out)
    print(line)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, name + '.json'), 'w') as f:
        f.write(line + '\n')


def _stats(ts):
    return {'us': round(statistics.median(ts), 2), 'min_us': round(min(ts), 2), 'max_us': round(max(ts), 2)}


def _batch(dev, seed=1):
    g = torch.Generator().manual_seed(seed)
    kf = torch.randn(B, 3, H, W, generator=g)
    sup = torch.randn(B, 3 * S, H, W, generator=g)
    joints = torch.rand(B, J, 2, generator=g) * torch.tensor([W, H], dtype=torch.float32)
    vis = (torch.rand(B, J, generator=g) < 0.8).float()
    return kf.to(dev), sup.to(dev), joints.to(dev), vis.to(dev)


def kernels(a):
    from fami_pose_amd._lib import lib
    dev = torch.device('cuda:0')
    s = torch.cuda.current_stream(dev).cuda_stream
    junk = torch.empty(1 << 28, device=dev)                    # 1 GiB: four times the Infinity Cache
    Hh, Wh = H // 4, W // 4
    L, R = Hh * Wh, B * J
    _, _, joints, vis = _batch(dev)
    pred = torch.randn(B, J, Hh, Wh, device=dev) * 0.1
    target, weight = torch.empty(B, J, Hh, Wh, device=dev), torch.empty(R, device=dev)
    ws, loss, iloss, dpred = torch.empty(R, device=dev), torch.empty(1, device=dev), torch.empty(1, device=dev), torch.empty_like(pred)
    coords, stats, txy = (torch.empty(R, 2, device=dev) for _ in range(3))
    center, scale = torch.full((B, 2), 150.0, device=dev), torch.full((B, 2), 1.25, device=dev)
    preds, maxvals, idx = torch.empty(R, 2, device=dev), torch.empty(R, device=dev), torch.empty(R, dtype=torch.int64, device=dev)
    p = lambda t: t.data_ptr()  # noqa: E731
    call = lib().call
    runs = {
        'gauss_target': lambda: call('fami_gauss_target_f32', p(joints), p(vis), p(target), p(weight), B, J, Hh, Wh, H, W, 3, s),
        'wmse_fwd': lambda: call('fami_wmse_fwd_f32', p(pred), p(target), p(weight), p(loss), R, L, 1.0 / (B * L * J), p(ws), s),
        'wmse_bwd': lambda: call('fami_wmse_bwd_f32', p(pred), p(target), p(weight), p(dpred), R, L, 1.0 / (B * L * J), None, 0, s),
        'softargmax_fwd': lambda: call('fami_softargmax_fwd_f32', p(pred), p(coords), p(stats), R, Hh, Wh, BETA, s),
        'heatmap_xy': lambda: call('fami_heatmap_xy_f32', p(joints), p(txy), R, Hh, Wh, H, W, s),
        'integral_l1_fwd': lambda: call('fami_integral_l1_fwd_f32', p(coords), p(txy), p(weight), p(iloss), R, Hh, Wh, 1.0 / R, p(ws), s),
        'integral_l1_bwd': lambda: call('fami_integral_l1_bwd_f32', p(pred), p(coords), p(stats), p(txy), p(weight), p(dpred), R, Hh,
                                        Wh, BETA, 1.0 / R, None, 1, s),
        'final_preds': lambda: call('fami_final_preds_f32', p(pred), p(center), p(scale), p(preds), p(maxvals), p(idx), B, J, Hh, Wh, s),
        'softargmax_preds': lambda: call('fami_softargmax_preds_f32', p(pred), p(center), p(scale), BETA, p(preds), p(maxvals), B, J,
                                         Hh, Wh, s),
    }
    seam_off = ('gauss_target', 'wmse_fwd', 'wmse_bwd')
    seam_on = ('gauss_target', 'wmse_fwd', 'softargmax_fwd', 'heatmap_xy', 'integral_l1_fwd', 'wmse_bwd', 'integral_l1_bwd')
    runs['seam off'] = lambda: [runs[n]() for n in seam_off]
    runs['seam on'] = lambda: [runs[n]() for n in seam_on]

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

    for fn in runs.values():
        window(fn, 20)
    us = {n: [] for n in runs}
    for _ in range(a.rounds):
        for n, fn in runs.items():
            us[n].append(window(fn, a.reps))
    out = {'tool': 'bench_integral kernels', 'device': torch.cuda.get_device_name(dev), 'reps': a.reps, 'rounds': a.rounds,
           'shape': [B, J, Hh, Wh], 'beta': BETA, 'bound': 'launch latency (no share of peak quoted)'}
    for n, fn in runs.items():
        rec = _stats(us[n])
        c = cold(fn, 21)
        rec.update({'cold_us': round(statistics.median(c), 2), 'cold_min_us': round(min(c), 2), 'cold_max_us': round(max(c), 2)})
        out[n] = rec
    out['seam on']['minus_off_us'] = round(out['seam on']['us'] - out['seam off']['us'], 2)
    out['seam on']['cold_minus_off_us'] = round(out['seam on']['cold_us'] - out['seam off']['cold_us'], 2)
    _emit(a, 'kernels', out)


def steps(a):
    import gc
    import fami_pose_amd as fp
    from fami_pose_amd.init import realistic_init_
    from fami_pose_amd.train import Trainer
    dev = torch.device('cuda:0')
    batch = _batch(dev)
    out = {'tool': 'bench_integral steps', 'device': torch.cuda.get_device_name(dev), 'steps': a.steps, 'rounds': a.rounds,
           'batch': B, 'shape': [H, W], 'num_sup': S, 'beta': BETA}
    for mode in a.modes.split(','):
        trainers = {}
        for name, kw in (('off', {}), ('on', dict(integral_l1_weight=1.0, integral_beta=BETA))):
            torch.manual_seed(19970808)
            model = fp.build_model(fp.default_cfg(48, image_size=(W, H), num_sup=S), 'train')
            realistic_init_(model, seed=19970808)
            model.set_compute_dtype(mode)
            trainers[name] = Trainer(model.to(dev), lr=1e-3, use_mi=True, use_graph=True, targets_from_joints=True, **kw)

        def window(tr, n):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(n):
                tr.step(*batch)
            torch.cuda.synchronize(dev)
            return (time.perf_counter() - t0) * 1e3 / n

        for tr in trainers.values():
            window(tr, a.warmup)
        ms = {n: [] for n in trainers}
        for _ in range(a.rounds):
            for n, tr in trainers.items():
                ms[n].append(window(tr, a.steps))
        rec = {}
        for n in trainers:
            m = statistics.median(ms[n])
            rec[n] = {'ms_per_step': round(m, 3), 'min_ms': round(min(ms[n]), 3), 'max_ms': round(max(ms[n]), 3),
                      'clips_per_s': round(B / m * 1e3, 2)}
        rec['off']['spread_ms'] = round(rec['off']['max_ms'] - rec['off']['min_ms'], 3)
        rec['on']['minus_off_ms'] = round(rec['on']['ms_per_step'] - rec['off']['ms_per_step'], 3)
        rec['on']['inside_off_spread'] = abs(rec['on']['minus_off_ms']) <= rec['off']['spread_ms']
        rec['on']['integral_loss_last_step'] = trainers['on'].integral_loss_value()
        out[mode] = rec
        del trainers
        gc.collect()
        torch.cuda.synchronize(dev)
        torch.cuda.empty_cache()
    _emit(a, 'steps', out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('what', choices=['kernels', 'steps'])
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--modes', default='f32,bf16')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'integral'))
    a = ap.parse_args()
    if a.reps < 1 or a.steps < 1 or a.warmup < 1:
        ap.error('--reps, --steps and --warmup must be >= 1')
    if a.rounds < 5:
        ap.error('--rounds must be >= 5: the spread between rounds is part of the result')
    if not torch.cuda.is_available():
        raise SystemExit('bench_integral needs the GPU')
    kernels(a) if a.what == 'kernels' else steps(a)


if __name__ == '__main__':
    main()
