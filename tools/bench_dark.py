"""What the DARK decode costs: kernel time of fami_dark_preds_f32 next to fami_final_preds_f32 on the W48 evaluation
heatmaps, and the time of `predict` with decode='dark', with the standard decode, and the way a user had to do it
before: both heatmap stacks copied to the host and the numpy statement run on them.

    python tools/bench_dark.py kernels [--reps 200] [--rounds 5] [--out profiles/dark]
    python tools/bench_dark.py eval [--modes f32,bf16] [--steps 40] [--warmup 5] [--rounds 5] [--out profiles/dark]

kernels: both decodes on [4,17,96,72] (one head of a batch of 4) and [8,17,96,72] (both heads), k = 11, plus k = 17 and
the 128x96 map for the DARK kernel.  Maps are construction 1 of tests/_dark_ref.make_maps (sigma-3 peaks plus noise).
Device events around `--reps` launches, the variants alternating over `--rounds` rounds, median and min..max in us per
call; COLD = single calls, each behind a 1 GiB fill that evicts the maps from the caches.  fami_final_preds_f32 is two
launches (argmax, decode), fami_dark_preds_f32 one.  Both are launch-latency-sized (68 / 136 workgroups): no share of a
peak is quoted; `flop` is the count of the two blur passes as the kernel runs them when the peak is inside the guard
(per output and pass (k-1)/2 pair additions, one multiplication and (k-1)/2 multiply-adds: 3 (k-1)/2 + 1 operations).

eval: a val-phase W48 model at 384x288, 4 supporting frames, batch 4, per compute mode.  `standard` is predict(x);
`dark` is predict(x, decode='dark'); `host_dark` is predict(x) followed by what the parent commit leaves a user to do
for the same result on both heads: the forward's two heatmap stacks to the host, tests/_dark_ref.dark_ref on each (numpy;
float64).  `standard` and `dark` copy their [B,J,2] coordinates and [B,J,1] confidences to the host, as the evaluation
loop does per batch -- for one head, as predict returns one; `host_dark` pays for two.  Windows of `--steps` calls
alternate between the variants over `--rounds` rounds after a warm-up of every shape; each window ends in a synchronise
(host clock).  Prints one JSON line per sub-command and writes it to <out>/<sub-command>.json.  Needs the GPU."""
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
    import _dark_ref as dr
    from fami_pose_amd import loss as FL
    from fami_pose_amd._lib import lib
    dev = torch.device('cuda:0')
    s = torch.cuda.current_stream(dev).cuda_stream
    junk = torch.empty(1 << 28, device=dev)                    # 1 GiB: four times the Infinity Cache

    def setup(shape, k):
        Bq, Jq, Hq, Wq = shape
        hm = torch.from_numpy(dr.make_maps(np.random.RandomState(1), *shape)).to(dev)
        c = torch.tensor([[320.0, 240.5]] * Bq, device=dev)
        sc = torch.tensor([[1.5, 2.0]] * Bq, device=dev)
        preds, mx = torch.empty(Bq, Jq, 2, device=dev), torch.empty(Bq, Jq, device=dev)
        ws = torch.empty(Bq * Jq, dtype=torch.int64, device=dev)
        taps = torch.from_numpy(FL.gaussian_taps(k)).to(dev)
        keep = (hm, c, sc, preds, mx, ws, taps)
        std = lambda: lib().call('fami_final_preds_f32', hm.data_ptr(), c.data_ptr(), sc.data_ptr(), preds.data_ptr(),  # noqa: E731
                                 mx.data_ptr(), ws.data_ptr(), Bq, Jq, Hq, Wq, s)
        dark = lambda: lib().call('fami_dark_preds_f32', hm.data_ptr(), c.data_ptr(), sc.data_ptr(), taps.data_ptr(), k,  # noqa: E731
                                  preds.data_ptr(), mx.data_ptr(), Bq, Jq, Hq, Wq, s)
        return keep, std, dark

    runs, keep = {}, []
    for shape, k in (((4, 17, 96, 72), 11), ((8, 17, 96, 72), 11), ((8, 17, 96, 72), 17), ((8, 17, 128, 96), 11)):
        kp, std, dark = setup(shape, k)
        keep.append(kp)
        tag = 'x'.join(map(str, shape))
        if k == 11:
            runs['final_preds %s' % tag] = (shape, k, std)
        runs['dark_preds %s k%d' % (tag, k)] = (shape, k, dark)

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

    for _, _, fn in runs.values():
        window(fn, 20)
    us = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, (_, _, fn) in runs.items():
            us[k].append(window(fn, a.reps))
    out = {'tool': 'bench_dark kernels', 'device': torch.cuda.get_device_name(dev), 'reps': a.reps, 'rounds': a.rounds}
    for name, (shape, k, fn) in runs.items():
        rec = _stats(us[name])
        c = cold(fn, 21)
        n = shape[0] * shape[1] * shape[2] * shape[3]
        rec.update({'cold_us': round(statistics.median(c), 2), 'cold_min_us': round(min(c), 2), 'cold_max_us': round(max(c), 2),
                    'workgroups': shape[0] * shape[1], 'bytes': 4 * n, 'bound': 'launch latency (no share of peak quoted)'})
        if name.startswith('dark'):
            rec['flop'] = 2 * n * ((k - 1) // 2 + 2 * ((k - 1) // 2) + 1)
            rec['lds_bytes'] = int(lib().cdll.fami_dark_preds_lds_bytes(shape[2], shape[3], k))
        out[name] = rec
    _emit(a, 'kernels', out)


def evaluate(a):
    import gc
    import _dark_ref as dr
    import fami_pose_amd as fp
    from fami_pose_amd.evaluate import predict
    from fami_pose_amd.init import realistic_init_
    dev = torch.device('cuda:0')
    gen = torch.Generator().manual_seed(1)
    kf, sup = torch.randn(B, 3, H, W, generator=gen).to(dev), torch.randn(B, 3 * S, H, W, generator=gen).to(dev)
    center = np.tile(np.array([[320.0, 240.5]], np.float32), (B, 1))
    scale = np.tile(np.array([[1.5, 2.0]], np.float32), (B, 1))
    out = {'tool': 'bench_dark eval', 'device': torch.cuda.get_device_name(dev), 'steps': a.steps, 'rounds': a.rounds,
           'batch': B, 'shape': [H, W], 'num_sup': S}
    for mode in a.modes.split(','):
        torch.manual_seed(19970808)
        model = fp.build_model(fp.default_cfg(48, image_size=(W, H), num_sup=S), fp.VAL_PHASE)
        realistic_init_(model, seed=19970808)
        model.set_compute_dtype(mode)
        model = model.to(dev).eval()

        def call(**kw):
            preds, maxvals, _ = predict(model, kf, sup, center, scale, **kw)
            return preds.cpu(), maxvals.cpu()

        def host_dark():
            with torch.no_grad():
                o = model(kf, sup)
            return [dr.dark_ref(o[h].float().cpu().numpy(), center, scale, 11)['preds'] for h in range(2)]

        variants = {'standard': lambda: call(), 'dark': lambda: call(decode='dark'), 'host_dark': host_dark}

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
                ms[k].append(window(fn, a.steps if k != 'host_dark' else max(2, a.steps // 8)))
        rec = {}
        for k in variants:
            m = statistics.median(ms[k])
            rec[k] = {'ms_per_call': round(m, 3), 'min_ms': round(min(ms[k]), 3), 'max_ms': round(max(ms[k]), 3),
                      'clips_per_s': round(B / m * 1e3, 2)}
        rec['dark']['minus_standard_ms'] = round(rec['dark']['ms_per_call'] - rec['standard']['ms_per_call'], 3)
        rec['standard']['spread_ms'] = round(rec['standard']['max_ms'] - rec['standard']['min_ms'], 3)
        d = np.abs(call(decode='dark')[0].numpy() - host_dark()[0]).max()
        rec['dark']['vs_host_float64_px'] = float(d)
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'dark'))
    a = ap.parse_args()
    if a.reps < 1 or a.steps < 1 or a.warmup < 1:
        ap.error('--reps, --steps and --warmup must be >= 1')
    if a.rounds < 5:
        ap.error('--rounds must be >= 5: the spread between rounds is part of the result')
    if not torch.cuda.is_available():
        raise SystemExit('bench_dark needs the GPU')
    kernels(a) if a.what == 'kernels' else evaluate(a)


if __name__ == '__main__':
    main()
