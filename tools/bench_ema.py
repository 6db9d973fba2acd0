"""What the moving average of the weights costs: kernel time of the update pass (and of the arena swap) on the W48 parameter
arena (64,655,204 fp32 elements), and step time of the bench workload with the average off and on.

    python tools/bench_ema.py kernels [--reps 100] [--rounds 5] [--out profiles/ema]
    python tools/bench_ema.py steps [--modes f32,bf16] [--steps 20] [--warmup 8] [--rounds 5] [--out profiles/ema]

kernels: fami_ema_update_f32 (reads ema and p, writes ema: 12 n bytes), fami_swap_f32 (reads and writes both: 16 n) and, as
yardsticks on the same arena, fami_axpby_f32(p, ema, ema) (the same 12 n of traffic) and the read-only fami_sumsq_f32 (4 n):
device events around `--reps` calls, the variants alternating over `--rounds` rounds, median and min..max reported; the
share is of the 8 TB/s HBM3E peak on those algorithmic bytes.  The update is also run with unequal 16-byte alignment of
the two arenas.  Back to back the 258.6 MB parameter arena is partly served from the 256 MB Infinity Cache, which a
training step cannot count on, so every variant is also timed COLD: single launches, each behind a 1 GiB fill, device
events around the one launch (`cold_us`, `cold_hbm_share`) -- the figures to quote.
Run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_ema.py kernels` for
per-dispatch times.

steps: the bench.py workload (W48, 5-frame 384x288 clips, batch 4, MI loss on, Adam, hipGraph replay).  Per compute mode a
default Trainer and one with ema_decay, each a model of its own from the same seed, in the same process, timed in windows
of `--steps` calls that alternate between the two over `--rounds` rounds: ms per step (host clock around a window that
ends in a synchronise).  Prints one JSON line per sub-command and writes it to <out>/<sub-command>.json.  Needs the GPU."""
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


def _emit(a, name, out):
    line = json.dumps(out)
    print(line)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, name + '.json'), 'w') as f:
        f.write(line + '\n')


def kernels(a):
    from fami_pose_amd._lib import lib
    dev = torch.device('cuda:0')
    n = a.n
    gen = torch.Generator(device=dev).manual_seed(0)
    buf_p = torch.empty(n + 4, device=dev).normal_(generator=gen).mul_(1e-2)
    buf_e = torch.empty(n + 4, device=dev).normal_(generator=gen).mul_(1e-2)
    p, ema, ema_off = buf_p[:n], buf_e[:n], buf_e[1:n + 1]        # ema_off: 4 bytes behind p's 16-byte alignment
    assert p.data_ptr() % 16 == 0 and ema.data_ptr() % 16 == 0 and ema_off.data_ptr() % 16 == 4
    parts = torch.zeros(lib().cdll.fami_sumsq_parts(), device=dev)
    st = torch.zeros(4, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    lib().call('fami_ema_prep_f32', st.data_ptr(), None, 0.999, 0, s)

    def update():
        lib().call('fami_ema_update_f32', ema.data_ptr(), p.data_ptr(), n, st.data_ptr(), s)

    def update_unaligned():
        lib().call('fami_ema_update_f32', ema_off.data_ptr(), p.data_ptr(), n, st.data_ptr(), s)

    def swap():
        lib().call('fami_swap_f32', p.data_ptr(), ema.data_ptr(), n, s)

    def axpby():
        lib().call('fami_axpby_f32', p.data_ptr(), ema.data_ptr(), ema.data_ptr(), n, 1e-3, 0.999, s)

    def sumsq():
        lib().call('fami_sumsq_f32', p.data_ptr(), n, parts.data_ptr(), s)

    runs = {'ema_update': (12, update), 'ema_update_unequal_alignment': (12, update_unaligned), 'swap': (16, swap),
            'axpby': (12, axpby), 'sumsq_read_only': (4, sumsq)}

    def window(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    junk = torch.empty(1 << 28, device=dev)                    # 1 GiB: four times the Infinity Cache

    def cold(fn, reps):
        """one launch at a time, each behind a 1 GiB fill that evicts both arenas from the caches -> median us"""
        ts = []
        for r in range(reps):
            junk.fill_(float(r))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        return statistics.median(ts)

    for _, fn in runs.values():
        window(fn, 10)
    ms = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, (_, fn) in runs.items():
            ms[k].append(window(fn, a.reps))
    cold_us = {k: cold(fn, 21) for k, (_, fn) in runs.items()}
    out = {'tool': 'bench_ema kernels', 'device': torch.cuda.get_device_name(dev), 'n': n, 'reps': a.reps,
           'rounds': a.rounds, 'peak_tbps': PEAK_BPS / 1e12}
    for k, (words, _) in runs.items():
        t = statistics.median(ms[k]) * 1e-3
        out[k] = {'us': round(t * 1e6, 2), 'min_us': round(min(ms[k]) * 1e3, 2), 'max_us': round(max(ms[k]) * 1e3, 2),
                  'bytes': words * n, 'tbps': round(words * n / t / 1e12, 3), 'hbm_share': round(words * n / t / PEAK_BPS, 3),
                  'cold_us': round(cold_us[k], 2), 'cold_hbm_share': round(words * n / (cold_us[k] * 1e-6) / PEAK_BPS, 3)}
    assert torch.isfinite(ema).all() and st[0].item() == 1.0
    _emit(a, 'kernels', out)


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

    out = {'tool': 'bench_ema steps', 'device': torch.cuda.get_device_name(dev), 'steps': a.steps, 'rounds': a.rounds,
           'ema_decay': a.decay}
    for mode in a.modes.split(','):
        trs = {'default': make(mode), 'ema': make(mode, ema_decay=a.decay, ema_warmup=True)}
        for tr in trs.values():
            window(tr, a.warmup)
        ms = {k: [] for k in trs}
        for _ in range(a.rounds):
            for k, tr in trs.items():
                ms[k].append(window(tr, a.steps))
        rec = {}
        for k in trs:
            rec[k] = {'ms_per_step': round(statistics.median(ms[k]), 3), 'min_ms': round(min(ms[k]), 3),
                      'max_ms': round(max(ms[k]), 3), 'in_backward_split': trs[k]._adam_split is not None}
        rec['ema']['added_ms'] = round(rec['ema']['ms_per_step'] - rec['default']['ms_per_step'], 3)
        rec['ema']['updates'] = trs['ema'].ema_updates()
        assert rec['ema']['updates'] == a.warmup + a.rounds * a.steps and trs['default'].ema is None
        out[mode] = rec
        del trs
        import gc
        gc.collect()
        torch.cuda.synchronize(dev)
        torch.cuda.empty_cache()
    _emit(a, 'steps', out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('what', choices=['kernels', 'steps'])
    ap.add_argument('--n', type=int, default=N_W48)
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--modes', default='f32,bf16')
    ap.add_argument('--decay', type=float, default=0.999)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=8)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ema'))
    a = ap.parse_args()
    if a.reps < 1 or a.rounds < 1 or a.steps < 1 or a.warmup < 1 or a.n < 1:
        ap.error('--n, --reps, --rounds, --steps and --warmup must be >= 1')
    if not torch.cuda.is_available():
        raise SystemExit('bench_ema needs the GPU')
    kernels(a) if a.what == 'kernels' else steps(a)


if __name__ == '__main__':
    main()
