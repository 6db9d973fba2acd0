"""What gradient accumulation costs: kernel time of the window-closing pass on the W48 gradient arena (64,655,204 fp32
elements) against the two launches it replaces, and time per micro-batch of the bench workload with and without it.

    python tools/bench_accum.py kernels [--reps 100] [--rounds 5]
    python tools/bench_accum.py steps [--modes f32,bf16] [--accum 4] [--steps 20] [--warmup 8] [--rounds 5]

kernels: fami_accum_unscale_check_sumsq_f32 (reads g and acc, writes g: 12 n bytes), the two-launch form of the parent
commit -- fami_axpby_f32(acc, g, g, 1, 1) (12 n) then fami_unscale_check_sumsq_f32 (8 n): 20 n -- and, as the yardstick,
fami_unscale_check_sumsq_f32 alone (8 n), on one seeded arena: device events around `--reps` calls, the variants
alternating over `--rounds` rounds, median and min..max reported; the share is of the 8 TB/s HBM3E peak.  Flag and
slab are requested everywhere.  (acc is zero and the factor 1: the arena stays what it is over any number of calls.)
Run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_accum.py kernels` for per-dispatch times.

steps: the bench.py workload (W48, 5-frame 384x288 clips, batch 4, MI loss on, Adam, hipGraph replay).  Per compute mode a
default Trainer and one with accum_steps = --accum, each a model of its own from the same seed, timed in windows of
`--steps` calls (a multiple of --accum) that alternate between the two over `--rounds` rounds: ms per micro-batch
(host clock around a window that ends in a synchronise), and device-event time of every call of the accumulating
trainer by window position (closing against non-closing).  Prints one JSON line per sub-command.  Needs the GPU."""
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
    acc = torch.zeros(n, device=dev)
    parts = torch.zeros(lib().cdll.fami_sumsq_parts(), device=dev)
    flag = torch.zeros(2, dtype=torch.int32, device=dev)
    one = torch.ones(1, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    want = g.clone()

    def fused():
        lib().call('fami_accum_unscale_check_sumsq_f32', g.data_ptr(), acc.data_ptr(), n, 1.0, one.data_ptr(), flag.data_ptr(),
                   parts.data_ptr(), s)

    def unscale():
        lib().call('fami_unscale_check_sumsq_f32', g.data_ptr(), n, 1.0, one.data_ptr(), flag.data_ptr(), parts.data_ptr(), s)

    def two_launch():
        lib().call('fami_axpby_f32', acc.data_ptr(), g.data_ptr(), g.data_ptr(), n, 1.0, 1.0, s)
        unscale()

    def axpby():
        lib().call('fami_axpby_f32', acc.data_ptr(), g.data_ptr(), g.data_ptr(), n, 1.0, 1.0, s)

    runs = {'accum_unscale_check_sumsq': (12, fused), 'axpby_then_unscale_check_sumsq': (20, two_launch),
            'unscale_check_sumsq': (8, unscale), 'axpby': (12, axpby)}

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
    out = {'tool': 'bench_accum kernels', 'device': torch.cuda.get_device_name(dev), 'n': n, 'reps': a.reps,
           'rounds': a.rounds, 'peak_tbps': PEAK_BPS / 1e12}
    for k, (words, _) in runs.items():
        t = statistics.median(ms[k]) * 1e-3
        out[k] = {'us': round(t * 1e6, 2), 'min_us': round(min(ms[k]) * 1e3, 2), 'max_us': round(max(ms[k]) * 1e3, 2),
                  'bytes': words * n, 'tbps': round(words * n / t / 1e12, 3), 'hbm_share': round(words * n / t / PEAK_BPS, 3)}
    assert flag[0].item() == 0 and torch.equal(g, want)
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

    def window(tr, n, per_call=None):
        torch.cuda.synchronize(dev)
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)] if per_call is not None else None
        t0 = time.perf_counter()
        for k in range(n):
            if evs:
                evs[k].record()
            tr.step(*batch)
        if evs:
            evs[n].record()
        torch.cuda.synchronize(dev)
        dt = (time.perf_counter() - t0) * 1e3 / n
        if evs:
            for k in range(n):
                per_call[k % a.accum].append(evs[k].elapsed_time(evs[k + 1]))
        return dt

    out = {'tool': 'bench_accum steps', 'device': torch.cuda.get_device_name(dev), 'steps': a.steps, 'rounds': a.rounds,
           'accum_steps': a.accum}
    for mode in a.modes.split(','):
        trs = {'default': make(mode), 'accum': make(mode, accum_steps=a.accum)}
        for tr in trs.values():
            window(tr, a.warmup)
        assert trs['accum'].window_position == 0
        ms = {k: [] for k in trs}
        per_call = [[] for _ in range(a.accum)]
        for _ in range(a.rounds):
            ms['default'].append(window(trs['default'], a.steps))
            ms['accum'].append(window(trs['accum'], a.steps, per_call))
        rec = {}
        for k in trs:
            rec[k] = {'ms_per_micro_batch': round(statistics.median(ms[k]), 3), 'min_ms': round(min(ms[k]), 3),
                      'max_ms': round(max(ms[k]), 3), 'in_backward_split': trs[k]._adam_split is not None}
        rec['accum']['added_ms'] = round(rec['accum']['ms_per_micro_batch'] - rec['default']['ms_per_micro_batch'], 3)
        # device events between consecutive calls, by window position: the last position is the closing call
        rec['accum']['call_ms_by_position'] = [
            {'ms': round(statistics.median(v), 3), 'min_ms': round(min(v), 3), 'max_ms': round(max(v), 3)} for v in per_call]
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
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--modes', default='f32,bf16')
    ap.add_argument('--accum', type=int, default=4)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=8)
    a = ap.parse_args()
    if a.reps < 1 or a.rounds < 1 or a.steps < 1 or a.accum < 2:
        ap.error('--reps, --rounds and --steps must be >= 1, --accum >= 2')
    if a.steps % a.accum or a.warmup % a.accum:
        ap.error('--steps and --warmup must be multiples of --accum: windows are never left open')
    if not torch.cuda.is_available():
        raise SystemExit('bench_accum needs the GPU')
    kernels(a) if a.what == 'kernels' else steps(a)


if __name__ == '__main__':
    main()
