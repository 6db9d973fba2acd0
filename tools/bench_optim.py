"""Kernel time and HBM share of the flat optimizers' update on the W48 parameter arena (64,655,204 fp32 elements).

    python tools/bench_optim.py [--reps 200] [--warmup 20] [--rounds 3]

Times fami_adam_f32 (torch.optim.Adam, the default TRAIN.OPTIMIZER) and fami_sgd_f32 (torch.optim.SGD with momentum
0.9, weight decay 1e-4: TRAIN.OPTIMIZER 'sgd' with the reference defaults; and without momentum) on seeded arenas:
device events around `--reps` back-to-back calls after `--warmup` calls, the kernels alternating over `--rounds`
rounds, the median round reported.  Bytes are the algorithm's: Adam reads p, g, m, v and writes p, m, v (7 x 4 n);
SGD with momentum reads p, g, buf and writes p, buf (5 x 4 n); SGD without momentum 3 x 4 n.  The share is of the
8 TB/s HBM3E peak (the float4-copy ceiling is ~6.3 TB/s, 0.79).  Prints one JSON line.  Needs the GPU: there is no
CPU fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

N_W48 = 64655204
PEAK_BPS = 8.0e12


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--n', type=int, default=N_W48)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--seed', type=int, default=0)
    a = ap.parse_args()
    if a.reps < 1 or a.rounds < 1:
        ap.error('--reps and --rounds must be >= 1')
    if not torch.cuda.is_available():
        raise SystemExit('bench_optim needs the GPU')
    from fami_pose_amd.train import FlatAdam, FlatSGD
    dev = torch.device('cuda:0')
    n = a.n
    gen = torch.Generator().manual_seed(a.seed)
    p0 = torch.randn(n, generator=gen).to(dev)
    g0 = (torch.randn(n, generator=gen) * 1e-2).to(dev)

    adam = FlatAdam(p0.clone(), lr=1e-3)
    adam.grad.copy_(g0)
    adam.prep()
    sgd = FlatSGD(p0.clone(), lr=1e-3, momentum=0.9, weight_decay=1e-4)
    sgd.grad.copy_(g0)
    sgd.prep()
    sgd.prep()                # step 2: the running momentum rule (step 1 reads the buffer too, but overwrites it)
    plain = FlatSGD(p0.clone(), lr=1e-3)
    plain.grad.copy_(g0)
    plain.prep()
    del p0, g0
    kernels = {'adam': (adam, 7), 'sgd': (sgd, 5), 'sgd_no_momentum': (plain, 3)}

    def window(opt, reps):
        s = torch.cuda.current_stream(dev).cuda_stream
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            opt._launch(0, n, s)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    for opt, _ in kernels.values():
        window(opt, a.warmup)
    ms = {k: [] for k in kernels}
    for _ in range(a.rounds):
        for k, (opt, _) in kernels.items():
            ms[k].append(window(opt, a.reps))
    out = {'tool': 'bench_optim', 'device': torch.cuda.get_device_name(dev), 'n': n, 'reps': a.reps,
           'rounds': a.rounds, 'peak_tbps': PEAK_BPS / 1e12}
    for k, (opt, words) in kernels.items():
        t = statistics.median(ms[k]) * 1e-3
        nbytes = words * 4 * n
        out[k] = {'kernel': 'fami_adam_f32' if k == 'adam' else 'fami_sgd_f32', 'ms': round(t * 1e3, 4),
                  'ms_rounds': [round(x, 4) for x in ms[k]], 'bytes': nbytes, 'tbps': round(nbytes / t / 1e12, 3),
                  'frac_peak': round(nbytes / t / PEAK_BPS, 3)}
        if not torch.isfinite(opt.p).all():
            raise SystemExit('%s: non-finite parameters after the timed calls' % k)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
