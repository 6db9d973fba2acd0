"""What the structure (limb-direction cosine) term costs: the launches between the forward and the backward pass of a training
step (targets, loss, seeds) without and with the term, alone and on top of the integral L1 term, and the step time of the bench
workload with and without it -- also against a checkout of the parent commit.

    python tools/bench_structure.py kernels [--reps 200] [--rounds 5] [--out profiles/structure]
    python tools/bench_structure.py steps [--modes f32,bf16] [--steps 20] [--warmup 5] [--rounds 5] [--variants off,on,both]
                                          [--root DIR] [--label NAME] [--out profiles/structure]
    python tools/bench_structure.py compare [--out profiles/structure]

kernels: on [4,17,96,72] (the W48 head of a batch of 4), joints as bench.py draws them, data.LIMB_PAIRS.
    off            fami_gauss_target_f32, fami_wmse_fwd_f32 (two launches: rows, sum), fami_wmse_bwd_f32
    structure      ... + fami_softargmax_fwd_f32, fami_heatmap_xy_f32, fami_structure_cos_fwd_f32 (two launches) behind the
                   loss, fami_structure_cos_bwd_f32 and fami_softargmax_bwd_f32 (accumulating) behind the seed
    integral       off + the integral term's launches (tools/bench_integral.py's `seam on`)
    both           integral + fami_structure_cos_fwd_f32, fami_structure_cos_bwd_f32, fami_softargmax_bwd_f32: the soft-argmax and
                   the target positions are launched ONCE and shared
Each new entry point alone and the seams as wholes.  Device events around `--reps` back-to-back launches, the variants
alternating over `--rounds` rounds, median and min..max in us per call; COLD = single calls, each behind a 1 GiB fill that
evicts the operands from the caches.  All of them are launch-latency-sized: no share of a peak is quoted.

steps: bench.py's workload (W48, 384x288, 4 supporting frames, batch 4, graph replay, targets from joints) per compute mode:
a default Trainer (`off`: the launch sequence of a Trainer without the option, launch for launch), one with
structure_cos_weight=1.0 (`on`) and one with integral_l1_weight=1.0 as well (`both`) in ONE process, windows of `--steps` steps
alternating between them over `--rounds` rounds after a warm-up of all; each window ends in a synchronise (host clock).
--root DIR imports the package from another checkout (the parent commit, built there; `--variants off` is all it can run) and
--label NAME writes <out>/steps_NAME.json instead of steps.json.

compare: reads <out>/steps.json and <out>/steps_parent.json and says, per mode, whether `off` here minus `off` of the parent
and `on` minus `off` leave the parent's own min..max spread between windows.  No GPU needed.

Prints one JSON line per sub-command and writes it to <out>/<name>.json.  kernels and steps need the GPU."""
import argparse
import json
import os
import statistics
import sys
import time

os.environ.setdefault('HIP_FORCE_DEV_KERNARG', '1')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

B, S, H, W, J = 4, 4, 384, 288, 17
BETA, MIN_LEN, EPS = 20.0, 1.0, 1e-8
VARIANTS = {'off': {}, 'on': dict(structure_cos_weight=1.0), 'both': dict(structure_cos_weight=1.0, integral_l1_weight=1.0)}


def _emit(a, name, out):
    line = json.dumps(out)
    print(line)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, name + '.json'), 'w') as f:
        f.write(line + '\n')


def _stats(ts):
    return {'us': round(statistics.median(ts), 2), 'min_us': round(min(ts), 2), 'max_us': round(max(ts), 2)}


def _batch(torch, dev, seed=1):
    g = torch.Generator().manual_seed(seed)
    kf = torch.randn(B, 3, H, W, generator=g)
    sup = torch.randn(B, 3 * S, H, W, generator=g)
    joints = torch.rand(B, J, 2, generator=g) * torch.tensor([W, H], dtype=torch.float32)
    vis = (torch.rand(B, J, generator=g) < 0.8).float()
    return kf.to(dev), sup.to(dev), joints.to(dev), vis.to(dev)


def kernels(a):
    import torch
    from fami_pose_amd._lib import lib
    from fami_pose_amd.data import LIMB_PAIRS
    dev = torch.device('cuda:0')
    s = torch.cuda.current_stream(dev).cuda_stream
    junk = torch.empty(1 << 28, device=dev)                    # 1 GiB: four times the Infinity Cache
    Hh, Wh = H // 4, W // 4
    L, R, P = Hh * Wh, B * J, len(LIMB_PAIRS)
    _, _, joints, vis = _batch(torch, dev)
    pred = torch.randn(B, J, Hh, Wh, device=dev) * 0.1
    target, weight = torch.empty(B, J, Hh, Wh, device=dev), torch.empty(R, device=dev)
    ws, dpred = torch.empty(max(R, B * P), device=dev), torch.empty_like(pred)
    loss, iloss, sloss = (torch.empty(1, device=dev) for _ in range(3))
    coords, stats, txy, gcoords = (torch.empty(R, 2, device=dev) for _ in range(4))
    pairs = torch.tensor(LIMB_PAIRS, dtype=torch.int32).to(dev)
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
        'structure_cos_fwd': lambda: call('fami_structure_cos_fwd_f32', p(coords), p(txy), p(weight), p(pairs), p(sloss), B, J, P,
                                          MIN_LEN, EPS, 1.0 / (B * P), p(ws), s),
        'structure_cos_bwd': lambda: call('fami_structure_cos_bwd_f32', p(coords), p(txy), p(weight), p(pairs), p(gcoords), B, J, P,
                                          MIN_LEN, EPS, 1.0 / (B * P), None, s),
        'softargmax_bwd': lambda: call('fami_softargmax_bwd_f32', p(pred), p(coords), p(stats), p(gcoords), p(dpred), R, Hh, Wh, BETA,
                                       1, s),
    }
    seams = {
        'seam off': ('gauss_target', 'wmse_fwd', 'wmse_bwd'),
        'seam structure': ('gauss_target', 'wmse_fwd', 'softargmax_fwd', 'heatmap_xy', 'structure_cos_fwd', 'wmse_bwd',
                           'structure_cos_bwd', 'softargmax_bwd'),
        'seam integral': ('gauss_target', 'wmse_fwd', 'softargmax_fwd', 'heatmap_xy', 'integral_l1_fwd', 'wmse_bwd', 'integral_l1_bwd'),
        'seam both': ('gauss_target', 'wmse_fwd', 'softargmax_fwd', 'heatmap_xy', 'integral_l1_fwd', 'structure_cos_fwd', 'wmse_bwd',
                      'integral_l1_bwd', 'structure_cos_bwd', 'softargmax_bwd'),
    }
    for name, seq in seams.items():
        runs[name] = lambda seq=seq: [runs[n]() for n in seq]

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
    out = {'tool': 'bench_structure kernels', 'device': torch.cuda.get_device_name(dev), 'reps': a.reps, 'rounds': a.rounds,
           'shape': [B, J, Hh, Wh], 'limbs': P, 'beta': BETA, 'min_len': MIN_LEN, 'bound': 'launch latency (no share of peak quoted)'}
    for n, fn in runs.items():
        rec = _stats(us[n])
        c = cold(fn, 21)
        rec.update({'cold_us': round(statistics.median(c), 2), 'cold_min_us': round(min(c), 2), 'cold_max_us': round(max(c), 2)})
        out[n] = rec
    for on, off in (('seam structure', 'seam off'), ('seam both', 'seam integral')):
        out[on]['minus'] = off
        out[on]['minus_us'] = round(out[on]['us'] - out[off]['us'], 2)
        out[on]['cold_minus_us'] = round(out[on]['cold_us'] - out[off]['cold_us'], 2)
    _emit(a, 'kernels', out)


def steps(a):
    import gc
    import torch
    import fami_pose_amd as fp
    from fami_pose_amd.init import realistic_init_
    from fami_pose_amd.train import Trainer
    dev = torch.device('cuda:0')
    batch = _batch(torch, dev)
    variants = a.variants.split(',')
    out = {'tool': 'bench_structure steps', 'device': torch.cuda.get_device_name(dev), 'steps': a.steps, 'rounds': a.rounds,
           'batch': B, 'shape': [H, W], 'num_sup': S, 'beta': BETA, 'min_len': MIN_LEN, 'label': a.label}
    for mode in a.modes.split(','):
        trainers = {}
        for name in variants:
            torch.manual_seed(19970808)
            model = fp.build_model(fp.default_cfg(48, image_size=(W, H), num_sup=S), 'train')
            realistic_init_(model, seed=19970808)
            model.set_compute_dtype(mode)
            trainers[name] = Trainer(model.to(dev), lr=1e-3, use_mi=True, use_graph=True, targets_from_joints=True, **VARIANTS[name])

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
                      'spread_ms': round(max(ms[n]) - min(ms[n]), 3), 'clips_per_s': round(B / m * 1e3, 2)}
        if 'off' in rec:
            for n in rec:
                if n != 'off':
                    rec[n]['minus_off_ms'] = round(rec[n]['ms_per_step'] - rec['off']['ms_per_step'], 3)
                    rec[n]['inside_off_spread'] = abs(rec[n]['minus_off_ms']) <= rec['off']['spread_ms']
        for n in rec:
            if n != 'off':
                rec[n]['structure_loss_last_step'] = trainers[n].structure_loss_value()
        out[mode] = rec
        del trainers
        gc.collect()
        torch.cuda.synchronize(dev)
        torch.cuda.empty_cache()
    _emit(a, 'steps' if not a.label else 'steps_' + a.label, out)


def compare(a):
    def load(name):
        with open(os.path.join(a.out, name + '.json')) as f:
            return json.loads(f.readline())
    here, parent = load('steps'), load('steps_parent')
    out = {'tool': 'bench_structure compare'}
    for mode in ('f32', 'bf16'):
        if mode not in here or mode not in parent:
            continue
        p, h = parent[mode]['off'], here[mode]
        rec = {'parent_off_ms': p['ms_per_step'], 'parent_spread_ms': p['spread_ms'], 'off_ms': h['off']['ms_per_step'],
               'off_minus_parent_ms': round(h['off']['ms_per_step'] - p['ms_per_step'], 3)}
        rec['off_leaves_parent_spread'] = abs(rec['off_minus_parent_ms']) > p['spread_ms']
        for n in ('on', 'both'):
            if n in h:
                rec[n + '_minus_off_ms'] = h[n]['minus_off_ms']
                rec[n + '_leaves_parent_spread'] = abs(h[n]['minus_off_ms']) > p['spread_ms']
        out[mode] = rec
    _emit(a, 'compare', out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('what', choices=['kernels', 'steps', 'compare'])
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--modes', default='f32,bf16')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--variants', default='off,on,both')
    ap.add_argument('--root', default=ROOT, help='the checkout whose package is imported (default: this one)')
    ap.add_argument('--label', default='', help='steps: write steps_LABEL.json')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'structure'))
    a = ap.parse_args()
    if a.reps < 1 or a.steps < 1 or a.warmup < 1:
        ap.error('--reps, --steps and --warmup must be >= 1')
    if a.rounds < 5:
        ap.error('--rounds must be >= 5: the spread between rounds is part of the result')
    if not a.variants or any(v not in VARIANTS for v in a.variants.split(',')):
        ap.error('--variants is a comma-separated list of ' + ', '.join(VARIANTS))
    if a.what == 'compare':
        return compare(a)
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_structure needs the GPU')
    kernels(a) if a.what == 'kernels' else steps(a)


if __name__ == '__main__':
    main()
