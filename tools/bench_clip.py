"""What gradient clipping and the dynamic loss scale cost: kernel time of the norm passes on the W48 gradient arena
(64,655,204 fp32 elements) and step time of the bench workload with and without the options.

    python tools/bench_clip.py kernels [--reps 100] [--rounds 3]
    python tools/bench_clip.py steps [--modes f32,bf16,f16] [--steps 20] [--warmup 5] [--rounds 3]

kernels: fami_sumsq_f32 (reads 4 n bytes), fami_unscale_check_sumsq_f32 (reads and writes: 8 n) and the existing
fami_unscale_check_f32 (8 n, the yardstick) back to back on one seeded arena -- device events around `--reps` calls, the
kernels alternating over `--rounds` rounds, median and min..max reported; the share is of the 8 TB/s HBM3E peak.  Run
it under `rocprofv3 --kernel-trace --stats -- python tools/bench_clip.py kernels` for per-dispatch times.

steps: the bench.py workload (W48, 5-frame 384x288 clips, batch 4, MI loss on, Adam, hipGraph replay).  Per compute
mode one default Trainer and its variants -- f32 / bf16: max_grad_norm set (threshold far above the norm, the cost is
the same); f16: max_grad_norm, loss_scale='dynamic', and both -- each a model of its own from the same seed, timed in
windows of `--steps` replays that alternate between the variants over `--rounds` rounds.  Reports the median window and
the spread of each variant and the added ms per step.  Prints one JSON line per sub-command.  Needs the GPU."""
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

N_W48 = 64655204
PEAK_BPS = 8.0e12


def kernels(a):
    from fami_pose_amd._lib import lib
    dev = torch.device('cuda:0')
    n = a.n
    g = torch.empty(n, device=dev).normal_(generator=torch.Generator(device=dev).manual_seed(0)).mul_(1e-2)
    parts = torch.zeros(lib().cdll.fami_sumsq_parts(), device=dev)
    flag = torch.zeros(2, dtype=torch.int32, device=dev)
    one = torch.ones(1, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    # (every read-write pass multiplies by 1: the arena stays what it is over any number of calls)
    runs = {
        'sumsq': (4, lambda: lib().call('fami_sumsq_f32', g.data_ptr(), n, parts.data_ptr(), s)),
        'unscale_check_sumsq': (8, lambda: lib().call('fami_unscale_check_sumsq_f32', g.data_ptr(), n, 1.0, one.data_ptr(),
                                                     flag.data_ptr(), parts.data_ptr(), s)),
        'unscale_check_sumsq_no_norm': (8, lambda: lib().call('fami_unscale_check_sumsq_f32', g.data_ptr(), n, 1.0, None,
                                                             flag.data_ptr(), None, s)),
        'unscale_check': (8, lambda: lib().call('fami_unscale_check_f32', g.data_ptr(), n, 1.0, flag.data_ptr(), s)),
    }

    def window(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    for _, fn in runs.values():
        window(fn, 10)
    ms = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, (_, fn) in runs.items():
            ms[k].append(window(fn, a.reps))
    out = {'tool': 'bench_clip kernels', 'device': torch.cuda.get_device_name(dev), 'n': n, 'reps': a.reps,
           'rounds': a.rounds, 'peak_tbps': PEAK_BPS / 1e12}
    for k, (words, _) in runs.items():
        t = statistics.median(ms[k]) * 1e-3
        out[k] = {'us': round(t * 1e6, 2), 'min_us': round(min(ms[k]) * 1e3, 2), 'max_us': round(max(ms[k]) * 1e3, 2),
                  'bytes': words * n, 'tbps': round(words * n / t / 1e12, 3), 'hbm_share': round(words * n / t / PEAK_BPS, 3)}
    assert flag[0].item() == 0
    print(json.dumps(out))


def steps(a):
    import fami_pose_amd as fp
    from fami_pose_amd.init import realistic_init_
    from fami_pose_amd.train import Trainer
    dev = torch.device('cuda:0')
    B, S, H, W, J = 4, 4, 384, 288, 17
    gen = torch.Generator().manual_seed(1)
    batch = (torch.randn(B, 3, H, W, generator=gen).to(dev), torch.randn(B, 3 * S, H, W, generator=gen).to(dev),
             (torch.rand(B, J, 2, generator=gen) * torch.tensor([W, H], dtype=torch.float32)).to(dev),
             (torch.rand(B, J, generator=gen) < 0.8).float().to(dev))

    def make(mode, **kw):
        cfg = fp.default_cfg(48, image_size=(W, H), num_sup=S)
        torch.manual_seed(19970808)
        model = fp.build_model(cfg, 'train')
        realistic_init_(model, seed=19970808)
        model.set_compute_dtype(mode)
        return Trainer(model.to(dev), lr=1e-3, use_mi=True, targets_from_joints=True, **kw)

    def window(tr, n):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(n):
            tr.step(*batch)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3 / n

    out = {'tool': 'bench_clip steps', 'device': torch.cuda.get_device_name(dev), 'steps': a.steps, 'rounds': a.rounds}
    for mode in a.modes.split(','):
        variants = {'default': {}, 'clip': dict(max_grad_norm=1e9)}
        if mode == 'f16':
            variants['dynamic'] = dict(loss_scale='dynamic', scaler=dict(init_scale=8192.0))
            variants['clip_dynamic'] = dict(max_grad_norm=1e9, loss_scale='dynamic', scaler=dict(init_scale=8192.0))
        trs = {k: make(mode, **kw) for k, kw in variants.items()}
        for tr in trs.values():
            window(tr, a.warmup)
        ms = {k: [] for k in trs}
        for _ in range(a.rounds):
            for k, tr in trs.items():
                ms[k].append(window(tr, a.steps))
        rec = {}
        base = statistics.median(ms['default'])
        for k in trs:
            med = statistics.median(ms[k])
            rec[k] = {'ms': round(med, 3), 'min_ms': round(min(ms[k]), 3), 'max_ms': round(max(ms[k]), 3),
                      'added_ms': round(med - base, 3), 'in_backward_split': trs[k]._adam_split is not None,
                      'skipped': trs[k].skipped_steps()}
        out[mode] = rec
        del trs
        import gc
        gc.collect()
        torch.cuda.synchronize(dev)
        torch.cuda.empty_cache()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('what', choices=['kernels', 'steps'])
    ap.add_argument('--n', type=int, default=N_W48)
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--modes', default='f32,bf16,f16')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    if a.reps < 1 or a.rounds < 1 or a.steps < 1:
        ap.error('--reps, --rounds and --steps must be >= 1')
    if not torch.cuda.is_available():
        raise SystemExit('bench_clip needs the GPU')
    kernels(a) if a.what == 'kernels' else steps(a)


if __name__ == '__main__':
    main()
