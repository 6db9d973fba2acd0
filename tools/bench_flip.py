"""What flip testing costs: kernel time of the two flip kernels on the W48 evaluation shapes, and clips per second of
`predict` plain, with flip=True, and as the two plain calls the same protocol needs without it.

    python tools/bench_flip.py kernels [--reps 200] [--rounds 5] [--out profiles/flip]
    python tools/bench_flip.py eval [--modes f32,bf16] [--steps 40] [--warmup 5] [--rounds 5] [--out profiles/flip]

kernels: fami_mirror_cat_f32 on the two inputs of a W48 batch of 4 ([4,3,384,288] key frames, [4,12,384,288] supporting
frames; reads n floats, writes 2 n) and fami_flip_merge_f32 on the heatmaps of that doubled batch ([8,17,96,72] -> [4,17,96,72]).
Device events around `--reps` launches, the variants alternating over `--rounds` rounds, median and min..max in us per
launch.  Back to back the mirror's 16 / 64 MB sit in the 256 MB Infinity Cache, so it is also timed COLD (single launches,
each behind a 1 GiB fill); both shares are of the 8 TB/s HBM3E peak on the algorithmic 12 n bytes.  The merge moves 1.4 MB:
it is launch-latency-sized and no share of peak is quoted for it.

eval: a val-phase W48 model at 384x288, 4 supporting frames, batch 4, per compute mode.  `plain` is predict(x); `flip` is
predict(x, flip=True) (one forward on the doubled batch, mirror and merge on the device); `two_calls` is predict(x) and
predict(pre-mirrored x), the two forwards the parent commit needs for the same protocol, WITHOUT any merge -- a yardstick
that flatters itself.  Every call copies its [B,J,2] coordinates and [B,J,1] confidences to the host, as the evaluation
loop does per batch.  Windows of `--steps` calls alternate between the variants over `--rounds` rounds after a warm-up
of every shape; each window ends in a synchronise (host clock).  clips/s counts the 4 clips of the batch per call (per pair of
calls for two_calls).  Prints one JSON line per sub-command and writes it to <out>/<sub-command>.json.  Needs the GPU."""
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

PEAK_BPS = 8.0e12
B, S, H, W, J = 4, 4, 384, 288, 17


def _emit(a, name, out):
    line = json.dumps(out)
    print(line)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, name + '.json'), 'w') as f:
        f.write(line + '\n')


def _stats(ts):
    return {'us': round(statistics.median(ts), 2), 'min_us': round(min(ts), 2), 'max_us': round(max(ts), 2)}


def kernels(a):
    from fami_pose_amd._lib import lib
    from fami_pose_amd.evaluate import flip_perm
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(0)
    s = torch.cuda.current_stream(dev).cuda_stream
    kf = torch.empty(B, 3, H, W, device=dev).normal_(generator=gen)
    sup = torch.empty(B, 3 * S, H, W, device=dev).normal_(generator=gen)
    kf2, sup2 = torch.empty(2 * B, 3, H, W, device=dev), torch.empty(2 * B, 3 * S, H, W, device=dev)
    hm2 = torch.empty(2 * B, J, H // 4, W // 4, device=dev).normal_(generator=gen)
    hm = torch.empty(B, J, H // 4, W // 4, device=dev)
    perm = torch.tensor(flip_perm(J), dtype=torch.int32, device=dev)

    def mirror(x, out):
        return lambda: lib().call('fami_mirror_cat_f32', x.data_ptr(), out.data_ptr(), x.numel() // W, W, s)

    def merge(shift):
        return lambda: lib().call('fami_flip_merge_f32', hm2.data_ptr(), perm.data_ptr(), hm.data_ptr(), B, J, H // 4, W // 4,
                                  shift, s)

    runs = {'mirror_cat_kf': (12 * kf.numel(), mirror(kf, kf2)), 'mirror_cat_sup': (12 * sup.numel(), mirror(sup, sup2)),
            'flip_merge': (None, merge(0)), 'flip_merge_shift': (None, merge(1))}

    def window(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps

    junk = torch.empty(1 << 28, device=dev)                    # 1 GiB: four times the Infinity Cache

    def cold(fn, reps):
        """one launch at a time, each behind a 1 GiB fill that evicts the operands from the caches -> us"""
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

    for _, fn in runs.values():
        window(fn, 20)
    us = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, (_, fn) in runs.items():
            us[k].append(window(fn, a.reps))
    out = {'tool': 'bench_flip kernels', 'device': torch.cuda.get_device_name(dev), 'reps': a.reps, 'rounds': a.rounds,
           'peak_tbps': PEAK_BPS / 1e12, 'shapes': {'kf': list(kf.shape), 'sup': list(sup.shape), 'hm2': list(hm2.shape)}}
    for k, (nbytes, fn) in runs.items():
        rec = _stats(us[k])
        if nbytes is None:
            rec['bytes'] = 12 * hm.numel()
            rec['bound'] = 'launch latency (no share of peak quoted)'
        else:
            c = cold(fn, 21)
            rec.update({'bytes': nbytes, 'hbm_share': round(nbytes / (rec['us'] * 1e-6) / PEAK_BPS, 3),
                        'cold_us': round(statistics.median(c), 2), 'cold_min_us': round(min(c), 2), 'cold_max_us': round(max(c), 2)})
            rec['cold_hbm_share'] = round(nbytes / (rec['cold_us'] * 1e-6) / PEAK_BPS, 3)
        out[k] = rec
    assert torch.equal(kf2[B:], kf.flip(3)) and torch.equal(sup2[:B], sup) and torch.isfinite(hm).all()
    _emit(a, 'kernels', out)


def evaluate(a):
    import gc
    import numpy as np
    import fami_pose_amd as fp
    from fami_pose_amd.evaluate import predict
    from fami_pose_amd.init import realistic_init_
    dev = torch.device('cuda:0')
    gen = torch.Generator().manual_seed(1)
    kf, sup = torch.randn(B, 3, H, W, generator=gen).to(dev), torch.randn(B, 3 * S, H, W, generator=gen).to(dev)
    kf_m, sup_m = kf.flip(3).contiguous(), sup.flip(3).contiguous()
    center = np.tile(np.array([[320.0, 240.5]], np.float32), (B, 1))
    scale = np.tile(np.array([[1.5, 2.0]], np.float32), (B, 1))
    out = {'tool': 'bench_flip eval', 'device': torch.cuda.get_device_name(dev), 'steps': a.steps, 'rounds': a.rounds,
           'batch': B, 'shape': [H, W], 'num_sup': S}
    for mode in a.modes.split(','):
        torch.manual_seed(19970808)
        model = fp.build_model(fp.default_cfg(48, image_size=(W, H), num_sup=S), fp.VAL_PHASE)
        realistic_init_(model, seed=19970808)
        model.set_compute_dtype(mode)
        model = model.to(dev).eval()

        def call(x, y, **kw):
            preds, maxvals, _ = predict(model, x, y, center, scale, **kw)
            return preds.cpu(), maxvals.cpu()

        variants = {
            'plain': lambda: call(kf, sup),
            'flip': lambda: call(kf, sup, flip=True),
            'two_calls': lambda: (call(kf, sup), call(kf_m, sup_m)),
        }

        def window(fn, n):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize(dev)
            return (time.perf_counter() - t0) * 1e3 / n

        for fn in variants.values():
            window(fn, a.warmup)
        ms = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items():
                ms[k].append(window(fn, a.steps))
        rec = {}
        for k in variants:
            m = statistics.median(ms[k])
            rec[k] = {'ms_per_call': round(m, 3), 'min_ms': round(min(ms[k]), 3), 'max_ms': round(max(ms[k]), 3),
                      'clips_per_s': round(B / m * 1e3, 2)}
        rec['flip']['vs_two_calls'] = round(rec['flip']['ms_per_call'] / rec['two_calls']['ms_per_call'], 4)
        rec['flip']['vs_plain'] = round(rec['flip']['ms_per_call'] / rec['plain']['ms_per_call'], 4)
        out[mode] = rec
        del model, variants
        gc.collect()
        torch.cuda.synchronize(dev)
        torch.cuda.empty_cache()
    _emit(a, 'eval', out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('what', choices=['kernels', 'eval'])
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--modes', default='f32,bf16')
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'flip'))
    a = ap.parse_args()
    if a.reps < 1 or a.steps < 1 or a.warmup < 1:
        ap.error('--reps, --steps and --warmup must be >= 1')
    if a.rounds < 5:
        ap.error('--rounds must be >= 5: the spread between rounds is part of the result')
    if not torch.cuda.is_available():
        raise SystemExit('bench_flip needs the GPU')
    kernels(a) if a.what == 'kernels' else evaluate(a)


if __name__ == '__main__':
    main()
