"""What preparing a batch of clips costs: ClipBatcher.prepare (one upload, one launch of fami_warp_normalize_batch_u8)
against the loop of B prepare_clip calls (2 B launches of fami_warp_normalize_u8, 2 B ctypes calls, the joints and the
visibilities uploaded as two arrays) writing into the same batch tensors.

    python tools/bench_prepare.py [--steps 20] [--warmup 3] [--rounds 5] [--reps 50] [--out profiles/prepare]

Shapes: F = 5 frames per clip, 1280x720 8-bit sources, (W, H) = (288, 384) crops; per clip a different box, rotation and
flip (seeded).  Cases: b4_private and b32_private (every clip its own five frames; both paths read the same memory: the
per-clip path a contiguous [5,720,1280,3] stack per clip, the batcher its five slices) and b32_shared, the evaluation
case (32 person boxes on ONE stack of five frames, key frame first in every clip -- the order that lets the per-clip
path use the stack as it is, without duplicating or re-slicing frames).

host: windows of `--steps` calls alternate between the two variants over `--rounds` rounds after a warm-up of both;
each window is a host clock around work that ends in a device synchronise.  ms per batch: median and min..max over the
rounds; `batched_vs_loop` is the ratio of the medians, and `beyond_spread` says whether the two min..max ranges are
disjoint.
kernel: the batched launch alone (table already on the device), device events around `--reps` launches back to back,
and COLD (single launches, each behind a 1 GiB fill that evicts sources and outputs from the caches).  Both shares are of
the 8 TB/s HBM3E peak on the ALGORITHMIC bytes: the fp32 outputs plus the DISTINCT source bytes the bilinear taps touch
(`touched_bytes` below restates the kernel's fixed-point coordinates per clip and unions the masks of clips that share a
frame).  Prints one JSON line and writes it to <out>/prepare.json.  Needs the GPU."""
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

PEAK_BPS = 8.0e12
F, HS, WS, SIZE, J = 5, 720, 1280, (288, 384), 17
CASES = (('b4_private', 4, False), ('b32_private', 32, False), ('b32_shared', 32, True))


def touched_mask(mi, flip, Hs, Ws, size):
    """[Hs,Ws] bool: the source pixels the four bilinear taps of any output pixel read (csrc/preproc.hip's coordinates)."""
    W, H = size
    x, y = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
    ad, bd = np.rint(mi[0, 0] * x * 1024.0).astype(np.int64), np.rint(mi[1, 0] * x * 1024.0).astype(np.int64)
    X0 = np.rint((mi[0, 1] * y + mi[0, 2]) * 1024.0).astype(np.int64) + 16
    Y0 = np.rint((mi[1, 1] * y + mi[1, 2]) * 1024.0).astype(np.int64) + 16
    sx, sy = ((X0 + ad) >> 5) >> 5, ((Y0 + bd) >> 5) >> 5
    mask = np.zeros((Hs, Ws), bool)
    for dy in (0, 1):
        for dx in (0, 1):
            yy, xx = sy + dy, sx + dx
            ok = (yy >= 0) & (yy < Hs) & (xx >= 0) & (xx < Ws)
            cols = Ws - 1 - xx[ok] if flip else xx[ok]
            mask[yy[ok], cols] = True
    return mask


def algorithmic_bytes(samples, trans, size):
    """fp32 outputs + distinct source bytes touched (clips that name the same frame share its mask)"""
    from fami_pose_amd.data import invert_affine
    masks = {}
    for s, t in zip(samples, trans):
        m = touched_mask(invert_affine(t), s['flip'], HS, WS, size)
        for fr in s['frames']:
            p = fr.data_ptr()
            masks[p] = m | masks[p] if p in masks else m
    src = 3 * int(sum(m.sum() for m in masks.values()))
    out = len(samples) * F * 3 * size[0] * size[1] * 4
    return src + out, src, out


def _range(ts):
    return {'ms': round(statistics.median(ts), 4), 'min_ms': round(min(ts), 4), 'max_ms': round(max(ts), 4)}


def run_case(a, dev, name, B, shared):
    from fami_pose_amd import data as D
    from fami_pose_amd._lib import lib
    rng = np.random.RandomState(B + shared)
    gen = torch.Generator(device=dev).manual_seed(B)
    n_stacks = 1 if shared else B
    stacks = [torch.randint(0, 256, (F, HS, WS, 3), dtype=torch.uint8, device=dev, generator=gen) for _ in range(n_stacks)]
    samples = []
    for k in range(B):
        st = stacks[0 if shared else k]
        joints = np.zeros((J, 3), np.float32)
        joints[:, 0], joints[:, 1] = rng.uniform(0, WS, J), rng.uniform(0, HS, J)
        vis = np.ones((J, 3), np.float32)
        vis[:, 2] = 0
        h = rng.uniform(250, 650)                                   # person box height in pixels, 3:4 like the crop
        samples.append({'stack': st, 'frames': [st[f] for f in range(F)], 'joints': joints, 'joints_vis': vis,
                        'center': np.array([rng.uniform(200, WS - 200), rng.uniform(150, HS - 150)]),
                        'scale': np.array([h * 0.75 / 200, h / 200]) * 1.25, 'rot': float(np.clip(rng.randn() * 45, -90, 90)),
                        'flip': bool(rng.rand() < 0.5)})
    batcher = D.ClipBatcher(B, F, SIZE, num_joints=J, device=dev)
    kf_x, sup_x = batcher.kf_x, batcher.sup_x
    j_dev, v_dev = torch.empty(B, J, 2, device=dev), torch.empty(B, J, device=dev)
    j_np, v_np = np.zeros((B, J, 2), np.float32), np.zeros((B, J), np.float32)

    def batched():
        batcher.prepare(samples)

    def loop():
        for k, s in enumerate(samples):
            _, _, j, v = D.prepare_clip(s['stack'], s['joints'], s['joints_vis'], s['center'], s['scale'], s['rot'], SIZE,
                                        flip=s['flip'], out_key=kf_x[k], out_sup=sup_x[k])
            j_np[k], v_np[k] = j[:, :2], v[:, 0]
        j_dev.copy_(torch.from_numpy(j_np), non_blocking=True)
        v_dev.copy_(torch.from_numpy(v_np), non_blocking=True)

    variants = {'batched': batched, 'loop': loop}

    def window(fn, n):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3 / n

    for fn in variants.values():
        window(fn, a.warmup)
    # the two paths agree before anything is timed
    loop()
    ref = (kf_x.clone(), sup_x.clone(), j_dev.clone(), v_dev.clone())
    kf_x.zero_(), sup_x.zero_()
    got = batcher.prepare(samples)
    assert all(torch.equal(x, y) for x, y in zip(got[:4], ref)), 'batched and per-clip paths differ'
    ms = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            ms[k].append(window(fn, a.steps))
    rec = {k: _range(ms[k]) for k in variants}
    rec['batched_vs_loop'] = round(rec['batched']['ms'] / rec['loop']['ms'], 4)
    rec['beyond_spread'] = bool(rec['batched']['max_ms'] < rec['loop']['min_ms'] or rec['loop']['max_ms'] < rec['batched']['min_ms'])

    # the batched launch alone: the table of the last prepare is still on the device
    table, s = batcher._buffers()['dev'].data_ptr(), torch.cuda.current_stream(dev).cuda_stream

    def launch():
        lib().call('fami_warp_normalize_batch_u8', table, kf_x.data_ptr(), sup_x.data_ptr(), B, F, SIZE[1], SIZE[0], 0,
                   *D.MEAN, *D.STD, s)

    def events(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps

    events(launch, 10)
    warm = [events(launch, a.reps) for _ in range(a.rounds)]
    junk = torch.empty(1 << 28, device=dev)                        # 1 GiB: four times the Infinity Cache
    cold = []
    for r in range(11):
        junk.fill_(float(r))
        cold.append(events(launch, 1))
    del junk
    assert torch.equal(kf_x, ref[0]) and torch.equal(sup_x, ref[1])
    nbytes, src, out = algorithmic_bytes(samples, got[4], SIZE)
    wu, cu = statistics.median(warm), statistics.median(cold)
    rec['kernel'] = {'us': round(wu, 2), 'min_us': round(min(warm), 2), 'max_us': round(max(warm), 2),
                     'cold_us': round(cu, 2), 'cold_min_us': round(min(cold), 2), 'cold_max_us': round(max(cold), 2),
                     'bytes': nbytes, 'source_bytes_touched': src, 'output_bytes': out,
                     'hbm_share': round(nbytes / (wu * 1e-6) / PEAK_BPS, 4),
                     'cold_hbm_share': round(nbytes / (cu * 1e-6) / PEAK_BPS, 4)}
    rec['launches'] = {'batched': 1, 'loop': 2 * B}
    del stacks, samples, batcher
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'prepare'))
    a = ap.parse_args()
    if a.reps < 1 or a.steps < 1 or a.warmup < 1:
        ap.error('--reps, --steps and --warmup must be >= 1')
    if a.rounds < 5:
        ap.error('--rounds must be >= 5: the spread between rounds is part of the result')
    if not torch.cuda.is_available():
        raise SystemExit('bench_prepare needs the GPU')
    dev = torch.device('cuda:0')
    out = {'tool': 'bench_prepare', 'device': torch.cuda.get_device_name(dev), 'steps': a.steps, 'rounds': a.rounds,
           'reps': a.reps, 'peak_tbps': PEAK_BPS / 1e12, 'frames': F, 'source': [HS, WS], 'crop_wh': list(SIZE)}
    for name, B, shared in CASES:
        out[name] = run_case(a, dev, name, B, shared)
    line = json.dumps(out)
    print(line)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, 'prepare.json'), 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
