"""What the options of the supervision cost: the three launches between the forward and the backward pass of a training
step (targets, loss, seeds) with the defaults and with every option on, and the step time of the bench workload with and
without the options.

    python tools/bench_loss.py kernels [--reps 200] [--rounds 5] [--out profiles/loss_options]
    python tools/bench_loss.py steps [--modes f32,bf16] [--steps 20] [--warmup 5] [--rounds 5] [--out profiles/loss_options]

kernels: on [4,17,96,72] (the W48 head of a batch of 4), joints as bench.py draws them.
    default   fami_gauss_target_f32, fami_wmse_fwd_f32 (two launches: rows, sum), fami_wmse_bwd_f32
    options   fami_gauss_target_ex_f32 (PoseTrack weights, sub-pixel), fami_ohkm_fwd_f32 (rows, selection; k = 8),
              fami_wmse_bwd_f32 on the selected weights
Each entry point alone and the seam as a whole.  Device events around `--reps` back-to-back launches, the variants
alternating over `--rounds` rounds, median and min..max in us per call; COLD = single calls, each behind a 1 GiB fill
that evicts the operands from the caches.  All of them are launch-latency-sized: no share of a peak is quoted.

steps: bench.py's workload (W48, 384x288, 4 supporting frames, batch 4, graph replay, targets from joints) per compute
mode: a default Trainer and one with target_encoding='subpixel', joint_weights=JOINTS_WEIGHT, ohkm_topk=8 in ONE
process, windows of `--steps` steps alternating between the two over `--rounds` rounds after a warm-up of both; each
window ends in a synchronise (host clock).  The figure to read: `options minus default` against the default's own
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
    from fami_pose_amd.data import JOINTS_WEIGHT
    dev = torch.device('cuda:0')
    s = torch.cuda.current_stream(dev).cuda_stream
    junk = torch.empty(1 << 28, device=dev)                    # 1 GiB: four times the Infinity Cache
    Hh, Wh, k = H // 4, W // 4, 8
    L = Hh * Wh
    _, _, joints, vis = _batch(dev)
    jw = torch.tensor(JOINTS_WEIGHT, device=dev)
    pred = torch.randn(B, J, Hh, Wh, device=dev) * 0.1
    target, weight = torch.empty(B, J, Hh, Wh, device=dev), torch.empty(B * J, device=dev)
    sel_w, ws = torch.empty(B * J, device=dev), torch.empty(B * J, device=dev)
    loss, dpred = torch.empty(1, device=dev), torch.empty_like(pred)
    p = lambda t: t.data_ptr()  # noqa: E731
    call = lib().call
    runs = {
        'gauss_target': lambda: call('fami_gauss_target_f32', p(joints), p(vis), p(target), p(weight), B, J, Hh, Wh, H, W, 3, s),
        'gauss_target_ex': lambda: call('fami_gauss_target_ex_f32', p(joints), p(vis), p(jw), p(target), p(weight), B, J, Hh,
                                        Wh, H, W, 3, 1, s),
        'wmse_fwd': lambda: call('fami_wmse_fwd_f32', p(pred), p(target), p(weight), p(loss), B * J, L, 1.0 / (B * L * J), p(ws), s),
        'ohkm_fwd': lambda: call('fami_ohkm_fwd_f32', p(pred), p(target), p(weight), p(loss), p(sel_w), B, J, L, k,
                                 1.0 / (B * L * k), p(ws), s),
        'wmse_bwd': lambda: call('fami_wmse_bwd_f32', p(pred), p(target), p(weight), p(dpred), B * J, L, 1.0 / (B * L * J), None, 0, s),
        'wmse_bwd_selected': lambda: call('fami_wmse_bwd_f32', p(pred), p(target), p(sel_w), p(dpred), B * J, L,
                                          1.0 / (B * L * k), None, 0, s),
    }
    seam_default = ('gauss_target', 'wmse_fwd', 'wmse_bwd')
    seam_options = ('gauss_target_ex', 'ohkm_fwd', 'wmse_bwd_selected')
    runs['seam default'] = lambda: [runs[n]() for n in seam_default]
    runs['seam options'] = lambda: [runs[n]() for n in seam_options]

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
    out = {'tool': 'bench_loss kernels', 'device': torch.cuda.get_device_name(dev), 'reps': a.reps, 'rounds': a.rounds,
           'shape': [B, J, Hh, Wh], 'ohkm_topk': k, 'bound': 'launch latency (no share of peak quoted)'}
    for n, fn in runs.items():
        rec = _stats(us[n])
        c = cold(fn, 21)
        rec.update({'cold_us': round(statistics.median(c), 2), 'cold_min_us': round(min(c), 2), 'cold_max_us': round(max(c), 2)})
        out[n] = rec
    out['seam options']['minus_default_us'] = round(out['seam options']['us'] - out['seam default']['us'], 2)
    out['seam options']['cold_minus_default_us'] = round(out['seam options']['cold_us'] - out['seam default']['cold_us'], 2)
    _emit(a, 'kernels', out)


def steps(a):
    import gc
    import fami_pose_amd as fp
    from fami_pose_amd.data import JOINTS_WEIGHT
    from fami_pose_amd.init import realistic_init_
    from fami_pose_amd.train import Trainer
    dev = torch.device('cuda:0')
    batch = _batch(dev)
    out = {'tool': 'bench_loss steps', 'device': torch.cuda.get_device_name(dev), 'steps': a.steps, 'rounds': a.rounds,
           'batch': B, 'shape': [H, W], 'num_sup': S}
    options = dict(target_encoding='subpixel', joint_weights=JOINTS_WEIGHT, ohkm_topk=8)
    for mode in a.modes.split(','):
        trainers = {}
        for name, kw in (('default', {}), ('options', options)):
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
        rec['default']['spread_ms'] = round(rec['default']['max_ms'] - rec['default']['min_ms'], 3)
        rec['options']['minus_default_ms'] = round(rec['options']['ms_per_step'] - rec['default']['ms_per_step'], 3)
        rec['options']['inside_default_spread'] = abs(rec['options']['minus_default_ms']) <= rec['default']['spread_ms']
        rec['options']['selected_joints_last_step'] = int(trainers['options'].ohkm_selection().sum().item())
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'loss_options'))
    a = ap.parse_args()
    if a.reps < 1 or a.steps < 1 or a.warmup < 1:
        ap.error('--reps, --steps and --warmup must be >= 1')
    if a.rounds < 5:
        ap.error('--rounds must be >= 5: the spread between rounds is part of the result')
    if not torch.cuda.is_available():
        raise SystemExit('bench_loss needs the GPU')
    kernels(a) if a.what == 'kernels' else steps(a)


if __name__ == '__main__':
    main()
