"""What degrading the crop costs: fami_warp_degrade_batch_u8 against fami_warp_normalize_batch_u8 on the same batch and
the same descriptor table, and the bench workload's training step fed by ClipBatcher.prepare with and without a `degrade`
field on every sample.

    python tools/bench_degrade.py [--steps 10] [--warmup 3] [--rounds 5] [--reps 50] [--no-step]
                                  [--parent-lib PATH] [--out profiles/degrade]

Shapes: B = 4 clips of F = 5 frames, 1920x1080 8-bit sources (every clip its own five frames), (W, H) = (288, 384)
crops; per clip a different box, rotation and flip (seeded).  Settings of the degraded launch:
  off             every flag off (the output is checked to be the plain launch's, bit for bit, before anything is timed)
  colour_occlude  colour on every frame, four rectangles (two constant, two noise) on every frame
  blur15          15 taps on every frame, a 30-crop-pixel line at a different angle per frame

kernel: the launches alone (tables already on the device): device events around `--reps` launches back to back, the
variants alternating over `--rounds` rounds, and COLD (single launches, each behind a 1 GiB fill that evicts sources and
outputs from the caches).  `--parent-lib`: a libfami_hip.so built from the parent commit; its plain launch is timed in the
same rounds as `parent_plain`, so that the refactored plain kernel is compared with the parent's and not with itself.
Bytes are ALGORITHMIC: the fp32 outputs plus the distinct source bytes the bilinear samples touch (for a blurred frame the
union over its taps; `per_tap` is the plain sample's count, which every tap repeats at its own offset).
step: windows of `--steps` calls of prepare + Trainer.step (f32, the bench workload's shapes: width 48, 384x288, 4
supporting frames, graph replay, targets from joints) alternate between plain and degraded samples; ms per step: median and
min..max over the rounds.  Prints one JSON line and writes it to <out>/degrade.json.  Needs the GPU."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

os.environ.setdefault('HIP_FORCE_DEV_KERNARG', '1')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

PEAK_BPS = 8.0e12
B, F, HS, WS, SIZE, J = 4, 5, 1080, 1920, (288, 384), 17
RECTS = [(20, 30, 120, 150, (124, 116, 104)), (150, 200, 330, 300, 'noise'), (-10, 340, 100, 400, (0, 0, 0)),
         (200, 10, 260, 90, 'noise')]
SETTINGS = {
    'off': lambda k: {},
    'colour_occlude': lambda k: {'colour': (1.2, -10.0, 0.8), 'occluders': [list(RECTS)] * F, 'seed': 1234 + k},
    'blur15': lambda k: {'blur': [(15, 30.0, 36.0 * f + 10.0 * k) for f in range(F)]},
}


def touched_bytes(mi, flip, steps):
    """distinct source bytes one frame's samples read: the union, over the taps' offsets `steps` (in 1/1024 source pixel),
    of the four bilinear neighbours of every output pixel that lie inside the image (csrc/preproc.hip's coordinates)"""
    W, H = SIZE
    x, y = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
    ad, bd = np.rint(mi[0, 0] * x * 1024.0).astype(np.int64), np.rint(mi[1, 0] * x * 1024.0).astype(np.int64)
    PX = np.rint((mi[0, 1] * y + mi[0, 2]) * 1024.0).astype(np.int64) + 16 + ad
    PY = np.rint((mi[1, 1] * y + mi[1, 2]) * 1024.0).astype(np.int64) + 16 + bd
    mask = np.zeros((HS, WS), bool)
    for dx_, dy_ in steps:
        sx, sy = ((PX + dx_) >> 5) >> 5, ((PY + dy_) >> 5) >> 5
        for dy in (0, 1):
            for dx in (0, 1):
                yy, xx = sy + dy, sx + dx
                ok = (yy >= 0) & (yy < HS) & (xx >= 0) & (xx < WS)
                mask[yy[ok], (WS - 1 - xx[ok]) if flip else xx[ok]] = True
    return 3 * int(mask.sum())


def _range(ts, unit='ms', digits=4):
    return {unit: round(statistics.median(ts), digits), 'min_' + unit: round(min(ts), digits),
            'max_' + unit: round(max(ts), digits)}


def make_samples(dev):
    rng = np.random.RandomState(B)
    gen = torch.Generator(device=dev).manual_seed(B)
    samples = []
    for k in range(B):
        st = torch.randint(0, 256, (F, HS, WS, 3), dtype=torch.uint8, device=dev, generator=gen)
        joints = np.zeros((J, 3), np.float32)
        joints[:, 0], joints[:, 1] = rng.uniform(0, WS, J), rng.uniform(0, HS, J)
        vis = np.ones((J, 3), np.float32)
        vis[:, 2] = 0
        h = rng.uniform(400, 900)                                   # person box height in pixels, 3:4 like the crop
        samples.append({'frames': [st[f] for f in range(F)], 'joints': joints, 'joints_vis': vis,
                        'center': np.array([rng.uniform(300, WS - 300), rng.uniform(250, HS - 250)]),
                        'scale': np.array([h * 0.75 / 200, h / 200]) * 1.25, 'rot': float(np.clip(rng.randn() * 45, -90, 90)),
                        'flip': bool(rng.rand() < 0.5)})
    return samples


def events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def run_kernels(a, dev, samples):
    from fami_pose_amd import data as D
    from fami_pose_amd._lib import lib
    W, H = SIZE
    batcher = D.ClipBatcher(B, F, SIZE, num_joints=J, device=dev)
    trans = batcher.prepare(samples)[4]
    ref = (batcher.kf_x.clone(), batcher.sup_x.clone())
    table, s = batcher._buffers()['dev'].data_ptr(), torch.cuda.current_stream(dev).cuda_stream
    kf_x, sup_x = batcher.kf_x, batcher.sup_x
    tail = (kf_x.data_ptr(), sup_x.data_ptr(), B, F, H, W, 0, *D.MEAN, *D.STD, s)
    inverse = [D.invert_affine(t) for t in trans]
    records, nbytes = {}, {}
    out_bytes = B * F * 3 * W * H * 4
    per_tap = sum(F * touched_bytes(mi, smp['flip'], [(0, 0)]) for mi, smp in zip(inverse, samples))
    for name, make in SETTINGS.items():
        rec = np.stack([D.degrade_records(make(k) or None, F, inverse[k]) for k in range(B)])
        records[name] = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(dev)
        src = 0
        for k, smp in enumerate(samples):
            for f in range(F):
                r = rec[k, f]
                taps = int(r['taps']) if r['flags'] & D.DEGRADE_BLUR else 1
                steps = [(t * int(r['step_x']), t * int(r['step_y'])) for t in range(-(taps - 1) // 2, (taps - 1) // 2 + 1)]
                src += touched_bytes(inverse[k], smp['flip'], steps)
        nbytes[name] = {'source_bytes_touched': src, 'output_bytes': out_bytes, 'bytes': src + out_bytes}
    nbytes['plain'] = {'source_bytes_touched': per_tap, 'output_bytes': out_bytes, 'bytes': per_tap + out_bytes}
    variants = {'plain': lambda: lib().call('fami_warp_normalize_batch_u8', table, *tail)}
    for name in SETTINGS:
        variants[name] = (lambda p: lambda: lib().call('fami_warp_degrade_batch_u8', table, p, *tail))(records[name].data_ptr())
    if a.parent_lib:
        parent = ctypes.CDLL(a.parent_lib)
        fn = parent.fami_warp_normalize_batch_u8
        fn.restype, fn.argtypes = ctypes.c_int, lib().protos['fami_warp_normalize_batch_u8'][1]

        def parent_plain():
            if fn(table, *tail) != 0:
                raise RuntimeError('parent fami_warp_normalize_batch_u8 failed')
        variants['parent_plain'] = parent_plain
        nbytes['parent_plain'] = nbytes['plain']
    # every variant that must equal the plain crop does, before anything is timed
    for name in ('off', 'parent_plain', 'plain'):
        if name in variants:
            kf_x.zero_(), sup_x.zero_()
            variants[name]()
            torch.cuda.synchronize(dev)
            assert torch.equal(kf_x, ref[0]) and torch.equal(sup_x, ref[1]), name + ' differs from the plain crop'
    for fn_ in variants.values():
        events(fn_, 10)
    warm = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn_ in variants.items():
            warm[k].append(events(fn_, a.reps))
    junk = torch.empty(1 << 28, device=dev)                        # 1 GiB: four times the Infinity Cache
    cold = {k: [] for k in variants}
    for r in range(11):
        for k, fn_ in variants.items():
            junk.fill_(float(r))
            cold[k].append(events(fn_, 1))
    del junk
    out = {'per_tap_source_bytes': per_tap}
    for k in variants:
        wu, cu = statistics.median(warm[k]), statistics.median(cold[k])
        out[k] = dict(_range(warm[k], 'us', 2), **{'cold_' + n: v for n, v in _range(cold[k], 'us', 2).items()}, **nbytes[k],
                      hbm_share=round(nbytes[k]['bytes'] / (wu * 1e-6) / PEAK_BPS, 4),
                      cold_hbm_share=round(nbytes[k]['bytes'] / (cu * 1e-6) / PEAK_BPS, 4))
    p = out['plain']
    for k in variants:
        if k != 'plain':
            out[k]['vs_plain'] = round(out[k]['us'] / p['us'], 4)
            out[k]['cold_vs_plain'] = round(out[k]['cold_us'] / p['cold_us'], 4)
    spread = p['max_us'] - p['min_us']
    out['off_slower_than_plain_beyond_its_spread'] = bool(out['off']['us'] - p['us'] > spread)
    if a.parent_lib:
        out['plain_slower_than_parent_beyond_its_spread'] = bool(
            p['us'] - out['parent_plain']['us'] > out['parent_plain']['max_us'] - out['parent_plain']['min_us'])
    return out


def run_steps(a, dev, samples):
    import fami_pose_amd as fp
    from fami_pose_amd import data as D
    from fami_pose_amd.init import realistic_init_
    from fami_pose_amd.train import Trainer
    cfg = fp.default_cfg(48, image_size=SIZE, num_sup=F - 1)
    torch.manual_seed(19970808)
    model = fp.build_model(cfg, 'train')
    realistic_init_(model, seed=19970808)
    model.set_compute_dtype('f32')
    trainer = Trainer(model.to(dev), lr=1e-3, use_mi=True, use_graph=True, targets_from_joints=True)
    batcher = D.ClipBatcher(B, F, SIZE, num_joints=J, device=dev)
    rng = np.random.RandomState(7)
    feeds = {'plain': samples,
             'degraded': [dict(s, degrade=D.draw_degradation(F, SIZE, {'photo_prob': 1.0, 'occlude_prob': 1.0, 'blur_prob_key': 1.0,
                                                                       'blur_prob_sup': 1.0, 'occlude_frames': 'all'}, rng))
                          for s in samples]}

    def window(feed, n):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(n):
            trainer.step(*batcher.prepare(feed)[:4])
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3 / n

    for feed in feeds.values():
        window(feed, a.warmup)
    ms = {k: [] for k in feeds}
    for _ in range(a.rounds):
        for k, feed in feeds.items():
            ms[k].append(window(feed, a.steps))
    out = {k: _range(ms[k]) for k in feeds}
    out['degraded_vs_plain'] = round(out['degraded']['ms'] / out['plain']['ms'], 4)
    out['beyond_spread'] = bool(out['degraded']['min_ms'] > out['plain']['max_ms'] or out['plain']['min_ms'] > out['degraded']['max_ms'])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--no-step', action='store_true', help='the launches only, not the training step')
    ap.add_argument('--parent-lib', default=None, help="a libfami_hip.so of the parent commit: its plain launch is timed too")
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'degrade'))
    a = ap.parse_args()
    if a.reps < 1 or a.steps < 1 or a.warmup < 1:
        ap.error('--reps, --steps and --warmup must be >= 1')
    if a.rounds < 5:
        ap.error('--rounds must be >= 5: the spread between rounds is part of the result')
    if not torch.cuda.is_available():
        raise SystemExit('bench_degrade needs the GPU')
    dev = torch.device('cuda:0')
    samples = make_samples(dev)
    out = {'tool': 'bench_degrade', 'device': torch.cuda.get_device_name(dev), 'steps': a.steps, 'rounds': a.rounds,
           'reps': a.reps, 'peak_tbps': PEAK_BPS / 1e12, 'clips': B, 'frames': F, 'source': [HS, WS], 'crop_wh': list(SIZE),
           'parent_lib': bool(a.parent_lib)}
    out['kernel'] = run_kernels(a, dev, samples)
    if not a.no_step:
        out['step'] = run_steps(a, dev, samples)
    line = json.dumps(out)
    print(line)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, 'degrade.json'), 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
