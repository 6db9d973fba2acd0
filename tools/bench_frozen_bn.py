"""What BatchNorm with frozen statistics costs and saves: the one-pass backward fami_bn_eval_bwd_* against the two launches of
fami_bn_bwd2_* on the same tensors, and step time / launches per step of the bench workload with frozen_bn None, 'backbone'
and 'all'.

    python tools/bench_frozen_bn.py kernels [--reps 50] [--rounds 7] [--out profiles/frozen_bn]
    python tools/bench_frozen_bn.py steps [--modes f32,bf16] [--steps 20] [--warmup 8] [--rounds 5] [--out profiles/frozen_bn]

kernels: [20*96*72, 48], [20*48*36, 96] and [20*12*9, 384] in f32 / bf16 / f16 with ReLU (mask from y), no residual:
`eval_bwd` (dx + parameter sums: the data pass and the channel-sized finalize), `eval_bwd_frozen_params` (dgamma = dbeta =
NULL: one launch, x not read) and `bwd2` (the train-mode backward's two launches, slot rows cleared outside the timed
window's launches by one memset per call, which is timed on its own as `memset` and NOT subtracted).  Every shape is warmed
up; device events around `--reps` calls; the variants alternate inside one call over `--rounds` rounds; median and
min..max of the windows are reported beside every difference.  hbm_share is of the 8 TB/s peak on ALGORITHMIC bytes computed
from the shape: (dy + y + x + dx) elements x element size, x dropped with frozen parameters; the train-mode backward is
given the same bytes although it reads dy, x and y twice.  Back to back these tensors (at most 26.5 MB each) are served
partly from the 256 MB Infinity Cache: the comparison between variants is like for like, the share is an upper bound on
what a step sees.

steps: the bench.py workload (W48, 5-frame 384x288 clips, batch 4, MI loss on, Adam, hipGraph replay); per compute mode
three Trainers from the same seed in one process, timed in windows of `--steps` calls that alternate over `--rounds`
rounds (host clock around a window that ends in a synchronise), and the entry-point calls of one eager step of each.
Prints one JSON line per sub-command and writes it to <out>/<sub-command>.json.  Needs the GPU."""
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
SHAPES = [(20 * 96 * 72, 48), (20 * 48 * 36, 96), (20 * 12 * 9, 384)]
DTYPES = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}


def _emit(a, name, out):
    line = json.dumps(out)
    print(line)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, name + '.json'), 'w') as f:
        f.write(line + '\n')


def _stat(v, scale=1.0):
    return {'median': round(statistics.median(v) * scale, 3), 'min': round(min(v) * scale, 3), 'max': round(max(v) * scale, 3)}


def kernels(a):
    from fami_pose_amd._lib import lib
    L = lib()
    dev = torch.device('cuda:0')
    s = torch.cuda.current_stream(dev).cuda_stream

    def window(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3          # us per call

    out = {'tool': 'bench_frozen_bn kernels', 'device': torch.cuda.get_device_name(dev), 'reps': a.reps, 'rounds': a.rounds,
           'peak_tbps': PEAK_BPS / 1e12, 'cases': []}
    for P, C in SHAPES:
        for dt, tdt in DTYPES.items():
            gen = torch.Generator(device=dev).manual_seed(P + C)
            mk = lambda *sh: torch.empty(*sh, device=dev).normal_(generator=gen)
            dy, x, y = mk(P, C).to(tdt), (mk(P, C) * 2 + 0.7).to(tdt), mk(P, C).to(tdt)
            dx = torch.empty_like(x)
            mean, invstd, gamma, beta = mk(C) * 0.3, mk(C).abs() + 0.5, mk(C).abs() + 0.5, mk(C)
            dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
            ws = torch.empty(L.cdll.fami_bn_workspace(C) // 4, device=dev)
            slots = torch.zeros(L.cdll.fami_bn_slots_bytes(C), dtype=torch.uint8, device=dev)
            p = lambda t: t.data_ptr()

            def eval_bwd():
                L.call('fami_bn_eval_bwd_' + dt, p(dy), p(x), p(y), p(mean), p(invstd), p(gamma), p(dx), p(dg), p(db), None, P, C,
                       1, 0, 0, 0, p(ws), s)

            def eval_bwd_frozen_params():
                L.call('fami_bn_eval_bwd_' + dt, p(dy), None, p(y), None, p(invstd), p(gamma), p(dx), None, None, None, P, C,
                       1, 0, 0, 0, None, s)

            def memset():
                slots.zero_()

            def bwd2():
                slots.zero_()
                L.call('fami_bn_bwd2_' + dt, p(dy), p(x), p(y), p(mean), p(invstd), p(gamma), p(beta), p(dx), p(dg), p(db), None,
                       P, C, 1, 0, 0, 0, p(slots), s)

            runs = {'eval_bwd': eval_bwd, 'eval_bwd_frozen_params': eval_bwd_frozen_params, 'bwd2': bwd2, 'memset': memset}
            for fn in runs.values():
                window(fn, 10)
            us = {k: [] for k in runs}
            for _ in range(a.rounds):
                for k, fn in runs.items():
                    us[k].append(window(fn, a.reps))
            esz = dy.element_size()
            nbytes = {'eval_bwd': 4 * P * C * esz, 'eval_bwd_frozen_params': 3 * P * C * esz, 'bwd2': 4 * P * C * esz}
            rec = {'P': P, 'C': C, 'dtype': dt, 'small_one_launch_train_form': bool(L.cdll.fami_bn_is_small(P, C))}
            for k in runs:
                rec[k] = {'us': _stat(us[k])}
                if k in nbytes:
                    t = statistics.median(us[k]) * 1e-6
                    rec[k].update(bytes=nbytes[k], hbm_share=round(nbytes[k] / t / PEAK_BPS, 3))
            # per-round differences (the variants of one round ran back to back): median and spread
            rec['bwd2_minus_eval_bwd_us'] = _stat([b - e for b, e in zip(us['bwd2'], us['eval_bwd'])])
            rec['bwd2_minus_memset_minus_eval_bwd_us'] = _stat([b - m - e for b, m, e in zip(us['bwd2'], us['memset'], us['eval_bwd'])])
            rec['eval_bwd_minus_frozen_params_us'] = _stat([e - f for e, f in zip(us['eval_bwd'], us['eval_bwd_frozen_params'])])
            out['cases'].append(rec)
            assert torch.isfinite(dx.float()).all() and torch.isfinite(dg).all()
    _emit(a, 'kernels', out)


def steps(a):
    import fami_pose_amd as fp
    from fami_pose_amd.init import realistic_init_
    from fami_pose_amd.train import Trainer
    from fami_pose_amd._lib import lib
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

    def count_calls(mode, scope):
        """entry-point calls of one eager step (a Trainer of its own; BatchNorm-related ones apart)"""
        tr = make(mode, frozen_bn=scope, use_graph=False)
        tr.step(*batch)
        L, names = lib(), []
        call, call_routed = L.call, L.call_routed
        L.call = lambda name, *ar: (names.append(name), call(name, *ar))[1]
        L.call_routed = lambda route, name, *ar: (names.append(name), call_routed(route, name, *ar))[1]
        try:
            tr.step(*batch)
        finally:
            del L.call, L.call_routed
        torch.cuda.synchronize(dev)
        return {'calls': len(names), 'bn_calls': sum(n.startswith('fami_bn_') for n in names),
                'bn_eval_bwd': sum(n.startswith('fami_bn_eval_bwd_') for n in names),
                'conv_stats_epilogues': sum(n.startswith('fami_conv2d_fwd_stats_') for n in names)}

    out = {'tool': 'bench_frozen_bn steps', 'device': torch.cuda.get_device_name(dev), 'steps': a.steps, 'rounds': a.rounds}
    scopes = {'none': None, 'backbone': 'backbone', 'all': 'all'}
    for mode in a.modes.split(','):
        trs = {k: make(mode, frozen_bn=v) for k, v in scopes.items()}
        for tr in trs.values():
            window(tr, a.warmup)
        ms = {k: [] for k in trs}
        for _ in range(a.rounds):
            for k, tr in trs.items():
                ms[k].append(window(tr, a.steps))
        rec = {k: {'ms_per_step': _stat(ms[k]), 'frozen_modules': len(trs[k].frozen_bn_names())} for k in trs}
        for k in ('backbone', 'all'):
            rec[k]['minus_none_ms'] = _stat([x - y for x, y in zip(ms[k], ms['none'])])
        del trs
        import gc
        gc.collect()
        torch.cuda.synchronize(dev)
        torch.cuda.empty_cache()
        for k, v in scopes.items():
            rec[k]['eager_step'] = count_calls(mode, v)
            gc.collect()
            torch.cuda.empty_cache()
        out[mode] = rec
    _emit(a, 'steps', out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('what', choices=['kernels', 'steps'])
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--modes', default='f32,bf16')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=8)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'frozen_bn'))
    a = ap.parse_args()
    if a.reps < 1 or a.rounds < 1 or a.steps < 1 or a.warmup < 1:
        ap.error('--reps, --rounds, --steps and --warmup must be >= 1')
    if not torch.cuda.is_available():
        raise SystemExit('bench_frozen_bn needs the GPU')
    kernels(a) if a.what == 'kernels' else steps(a)


if __name__ == '__main__':
    main()
