"""fami_warp_degrade_batch_u8 / ClipBatcher's `degrade` field on the MI355X against the numpy restatement of fami.h's
stages (tests/_degrade_ref.py), bit for bit.  Shapes are test_prepare_batch_gpu.py's: three clips (60x90, 180x260 flipped,
97x131) whose crops reach outside the images, F = 3, crops of (W, H) = (40, 52) = eight full workgroups and a tail of 32.
Every launch writes into views inside larger NaN-filled allocations."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _degrade_ref as R  # noqa: E402

from fami_pose_amd import data as D  # noqa: E402

pytestmark = pytest.mark.gpu

SIZE = (40, 52)
W, H = SIZE
B, F = 3, 3
SRC = [(60, 90), (180, 260), (97, 131)]               # (Hs, Ws) per clip
ROT = [0.0, 31.0, -44.0]
FLIP = [False, True, False]
CENTER = [(50.5, 28.25), (140.5, 80.25), (20.0, 70.0)]          # the crops reach outside the images
SCALE = [(0.45, 0.6), (0.9, 1.2), (0.6, 0.8)]
PAD = 4096                                                      # floats of NaN before and after each output

# steps in 1/1024 source pixel; with 15 taps the outer ones are 28, 21 and 29 source pixels away: outside the 60x90 clip
STEPS = [(1500, 0), (-700, 2100), (4096, -3000)]
COLOUR = [(1.3, -20.5, 0.4), (0.6, 30.25, 1.8), (1.0 / 3, 100.0, 0.0)]        # per clip; the last one clamps at 255
RECTS = [
    # key frame: over the left and right edges, a later rectangle over part of the first, an empty one
    [(-3, 10, 4, 20, 0, (200, 10, 30)), (36, 30, 45, 40, 1, (0, 0, 0)), (2, 15, 12, 25, 0, (1, 2, 3)), (5, 5, 5, 9, 0, (9, 9, 9))],
    # first supporting frame: over the top and bottom edges, noise under a constant and a constant under noise
    [(10, -5, 20, 3, 1, (0, 0, 0)), (15, 48, 25, 60, 0, (255, 0, 128)), (12, 0, 18, 8, 0, (7, 77, 177)), (20, 44, 30, 50, 1, (0, 0, 0))],
    # second supporting frame: the whole crop and more in noise, then a constant patch and an inverted (empty) rectangle
    [(-1, -1, 41, 53, 1, (0, 0, 0)), (8, 8, 30, 40, 0, (124, 116, 104)), (30, 30, 20, 20, 0, (5, 5, 5))],
]


def _samples(dev, seed=21, n=B):
    rng = np.random.RandomState(seed)
    samples, host = [], []
    for k in range(n):
        Hs, Ws = SRC[k]
        fr = (rng.rand(F, Hs, Ws, 3) * 255).astype(np.uint8)
        joints = np.zeros((17, 3), np.float32)
        joints[:, 0], joints[:, 1] = rng.uniform(0, Ws, 17), rng.uniform(0, Hs, 17)
        vis = np.ones((17, 3), np.float32)
        samples.append({'frames': [torch.from_numpy(fr[f]).to(dev) for f in range(F)], 'joints': joints, 'joints_vis': vis,
                        'center': np.array(CENTER[k]), 'scale': np.array(SCALE[k]), 'rot': ROT[k], 'flip': FLIP[k]})
        host.append(fr)
    return samples, host


@pytest.fixture(scope='module')
def clips(dev):
    """the three clips on the device and on the host, shared and left unchanged by every test"""
    return _samples(dev)


def _records(stages, taps=3):
    """[B][F] restatement records with the chosen stages; every (clip, frame) gets its own parameters"""
    recs = []
    for k in range(B):
        row = []
        for f in range(F):
            r = {'flags': 0}
            if 'blur' in stages:
                sx, sy = STEPS[(k + f) % 3]
                r.update(flags=r['flags'] | R.BLUR, taps=taps, step_x=sx, step_y=sy)
            if 'colour' in stages:
                a, d, s = COLOUR[k]
                r.update(flags=r['flags'] | R.COLOUR, alpha=a, delta=d + f, sat=s)
            if 'occlude' in stages:
                r.update(flags=r['flags'] | R.OCCLUDE, rects=RECTS[(k + f) % 3], seed=(0x9e3779b9 * (k * F + f + 1)) & 0xffffffff)
            row.append(r)
        recs.append(row)
    return recs


def _pack(recs):
    """restatement records -> the [n][F] fami_degrade_frame_t array, field by field"""
    out = np.zeros((len(recs), F), D._DEGRADE_REC)
    for k, row in enumerate(recs):
        for f, r in enumerate(row):
            o = out[k, f]
            o['flags'] = r['flags']
            for name in ('taps', 'step_x', 'step_y', 'alpha', 'delta', 'sat', 'seed'):
                o[name] = r.get(name, 0)
            for q, (x0, y0, x1, y1, mode, fill) in enumerate(r.get('rects', [])):
                o['rect'][q] = (x0, y0, x1, y1, fill, mode)
            o['n_rect'] = len(r.get('rects', []))
    return out


def _unpack(rec):
    """one fami_degrade_frame_t (as ClipBatcher staged it) -> a restatement record"""
    return {'flags': int(rec['flags']), 'taps': int(rec['taps']), 'step_x': int(rec['step_x']), 'step_y': int(rec['step_y']),
            'alpha': rec['alpha'], 'delta': rec['delta'], 'sat': rec['sat'], 'seed': int(rec['seed']),
            'rects': [(int(q['x0']), int(q['y0']), int(q['x1']), int(q['y1']), int(q['mode']), tuple(int(v) for v in q['fill']))
                      for q in rec['rect'][:int(rec['n_rect'])]]}


def _guarded(dev, channels):
    whole = torch.full((PAD + B * channels * H * W + PAD,), float('nan'), device=dev)
    return whole, whole[PAD:PAD + B * channels * H * W].view(B, channels, H, W)


def _launch(dev, samples, packed, bgr, name='fami_warp_degrade_batch_u8'):
    """Stage the table of samples[:n] with a ClipBatcher (the plain prepare), then call the entry point itself on guarded
    outputs.  -> key [B,3,H,W], sup [B,6,H,W] (rows n.. and the guard bands checked to be NaN still), trans [n,2,3]"""
    from fami_pose_amd._lib import lib
    n = len(samples)
    b = D.ClipBatcher(B, F, SIZE, bgr=bgr, device=dev)
    trans = b.prepare(samples)[4]
    key_all, key = _guarded(dev, 3)
    sup_all, sup = _guarded(dev, 3 * (F - 1))
    args = [b._buffers()['dev'].data_ptr()]
    if packed is not None:
        rec_dev = torch.from_numpy(np.ascontiguousarray(packed).view(np.uint8).reshape(-1).copy()).to(dev)
        assert rec_dev.numel() == n * F * 128 and rec_dev.data_ptr() % 8 == 0
        args.append(rec_dev.data_ptr())
    lib().call(name, *args, key.data_ptr(), sup.data_ptr(), n, F, H, W, int(bgr), *D.MEAN, *D.STD,
               torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    for whole, view in ((key_all, key), (sup_all, sup)):
        assert torch.isnan(whole[:PAD]).all() and torch.isnan(whole[-PAD:]).all()
        assert torch.isnan(view[n:]).all() and not torch.isnan(view[:n]).any()
    return key, sup, trans


def _reference(host, trans, recs, bgr):
    from oracle import ops as O
    keys, sups = [], []
    for k in range(len(recs)):
        key, sup = R.degrade_clip(host[k], O.cv2_invert_affine(trans[k]), SIZE, FLIP[k], bgr, recs[k], D.MEAN, D.STD)
        keys.append(key), sups.append(sup)
    return np.stack(keys), np.stack(sups)


@pytest.mark.parametrize('bgr', [False, True])
@pytest.mark.parametrize('n', [2, 3])
def test_every_flag_off_is_the_plain_launch(dev, clips, n, bgr):
    samples, host = clips
    off = np.zeros((n, F), D._DEGRADE_REC)
    # parameters that would change every pixel if a stage ran with them: a flag that is off skips the stage
    off['taps'], off['step_x'], off['alpha'], off['sat'], off['n_rect'], off['seed'] = 15, 5000, 2.0, 0.0, 4, 99
    off['rect']['x1'], off['rect']['y1'] = 100, 100
    key, sup, trans = _launch(dev, samples[:n], off, bgr)
    key0, sup0, _ = _launch(dev, samples[:n], None, bgr, name='fami_warp_normalize_batch_u8')
    assert torch.equal(key[:n], key0[:n]) and torch.equal(sup[:n], sup0[:n])
    want_key, want_sup = _reference(host, trans, [[{'flags': 0}] * F] * n, bgr)
    assert np.array_equal(key[:n].cpu().numpy(), want_key) and np.array_equal(sup[:n].cpu().numpy(), want_sup)


CASES = {'taps1': (('blur',), 1), 'taps3': (('blur',), 3), 'taps15': (('blur',), 15), 'colour': (('colour',), 3),
         'occlude': (('occlude',), 3), 'all_taps3': (('blur', 'colour', 'occlude'), 3),
         'all_taps15': (('blur', 'colour', 'occlude'), 15)}


@pytest.mark.parametrize('bgr', [False, True])
@pytest.mark.parametrize('case', list(CASES))
def test_stages_against_the_restatement(dev, clips, case, bgr):
    samples, host = clips
    stages, taps = CASES[case]
    recs = _records(stages, taps)
    key, sup, trans = _launch(dev, samples, _pack(recs), bgr)
    want_key, want_sup = _reference(host, trans, recs, bgr)
    got_key, got_sup = key.cpu().numpy(), sup.cpu().numpy()
    assert np.array_equal(got_key, want_key), np.abs(got_key - want_key).max()
    assert np.array_equal(got_sup, want_sup), np.abs(got_sup - want_sup).max()
    # the stage did something on every frame of every clip, the flipped one included ...
    plain_key, plain_sup = _reference(host, trans, [[{'flags': 0}] * F] * B, bgr)
    if case != 'taps1':                       # ... except that one tap is the plain sample, whatever the steps
        assert all((got_key[k] != plain_key[k]).any() for k in range(B))
        assert all((got_sup[k, 3 * f:3 * f + 3] != plain_sup[k, 3 * f:3 * f + 3]).any() for k in range(B) for f in range(F - 1))
    else:
        assert np.array_equal(got_key, plain_key) and np.array_equal(got_sup, plain_sup)


def test_taps_leave_the_source():
    """the condition of the blur cases, on the restatement's own coordinates: with 15 taps some samples of every clip lie
    wholly outside its source, on each side"""
    from oracle import ops as O
    for k in range(B):
        c = np.array(CENTER[k])
        if FLIP[k]:
            c[0] = SRC[k][1] - c[0] - 1
        PX, PY = R.origin(O.cv2_invert_affine(O.dark_get_affine_transform(c, np.array(SCALE[k]), ROT[k], SIZE)), SIZE)
        sx = np.concatenate([((PX + t * s[0]) >> 10).ravel() for s in STEPS for t in (-7, 7)])
        sy = np.concatenate([((PY + t * s[1]) >> 10).ravel() for s in STEPS for t in (-7, 7)])
        assert sx.min() < -1 and sx.max() > SRC[k][1] and sy.min() < -1 and sy.max() > SRC[k][0]


def test_two_runs_give_equal_bits(dev, clips):
    samples, _ = clips
    packed = _pack(_records(('blur', 'colour', 'occlude'), 15))
    a = _launch(dev, samples, packed, False)
    b = _launch(dev, samples, packed, False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


DEGRADE = [
    {'colour': (1.2, -12.5, 0.7), 'blur': [(5, 6.5, 30.0), None, (15, 22.0, 100.0)],
     'occluders': [[(5, 10, 25, 30, (124, 116, 104))], [], [(-4, 40, 50, 60, 'noise'), (0, 0, 10, 10, (1, 2, 3))]], 'seed': 0xfeedbeef},
    None,
    {'blur': [None, (3, 3.0, 170.0), None], 'occluders': [[(30, -2, 44, 20, 'noise')], [], []], 'seed': 5},
]


@pytest.mark.parametrize('n', [2, 3])
def test_batcher_mixes_samples_with_and_without_the_field(dev, clips, n):
    """ClipBatcher.prepare end to end: nothing is allocated for the table before the first degraded batch; a degraded batch
    stages one record per (sample, frame) behind the joints (all flags off where the sample has no field, blur steps from
    the sample's own inverse transform) and equals the restatement; joints and visibilities are the plain batch's; a plain
    batch afterwards is the plain launch again, and rows n.. are left alone."""
    samples, host = clips
    plain = [dict(s) for s in samples[:n]]
    degraded = [dict(s, degrade=DEGRADE[k]) for k, s in enumerate(samples[:n])]
    b = D.ClipBatcher(B, F, SIZE, device=dev)
    kf0, sup0, j0, v0 = [t.clone() for t in b.prepare(plain)[:4]]
    assert 'h_degrade' not in b._bufs and b._bufs['host'].numel() == b._bufs['plain_bytes']
    b.kf_x.fill_(float('nan'))
    b.sup_x.fill_(float('nan'))
    out = b.prepare(degraded)
    kf, sup, joints, vis, trans = out[:5]
    assert kf.data_ptr() == b.kf_x.data_ptr() and joints.data_ptr() == b.joints.data_ptr() and len(out) == 7
    assert torch.equal(joints, j0) and torch.equal(vis, v0)
    staged = b._bufs['h_degrade']
    assert staged.shape == (B, F) and staged[1].tobytes() == bytes(F * 128)
    assert staged['flags'][0].tolist() == [7, 2, 7] and staged['flags'][n - 1].tolist() == ([0, 0, 0] if n == 2 else [4, 1, 0])
    from oracle import ops as O
    for k in range(n):
        want = D.degrade_records(DEGRADE[k], F, O.cv2_invert_affine(trans[k]))
        assert staged[k].tobytes() == want.tobytes(), k
    recs = [[_unpack(staged[k, f]) for f in range(F)] for k in range(n)]
    want_key, want_sup = _reference(host, trans, recs, False)
    assert np.array_equal(kf.cpu().numpy(), want_key) and np.array_equal(sup.cpu().numpy(), want_sup)
    assert torch.equal(kf[1], kf0[1]) and torch.equal(sup[1], sup0[1]) and not torch.equal(kf[0], kf0[0])
    assert torch.isnan(b.kf_x[n:]).all() and torch.isnan(b.sup_x[n:]).all() and not torch.isnan(kf).any()
    again = b.prepare(plain)
    assert torch.equal(again[0], kf0) and torch.equal(again[1], sup0) and torch.equal(again[2], j0) and torch.equal(again[3], v0)
    assert torch.isnan(b.kf_x[n:]).all()
