"""The DARK decode on the MI355X (csrc/decode.hip: fami_dark_preds_f32; loss.dark_get_final_preds;
evaluate.predict / evaluate_loop(decode='dark')) against the float64 restatement tests/_dark_ref.py of the reference's
dark_get_final_preds (datasets/process/heatmaps_process.py:84-143) and against the reference-generated fixture
tests/golden/dark_final_preds.npz (tests/test_dark_host.py says what that fixture pins).

Bounds.  `maxvals` and the integer coordinates come from the same comparison rule as fami_final_preds_f32's argmax: bit
equality.  With center = (W/2, H/2) and scale = W/200 the fp32 factor 200 scale / W is exactly 1 for every W used here
(asserted), so the transform is the identity, an unrefined coordinate must come back as the integer itself, and a
refined one is compared in heatmap pixels: 5e-5 against float64.  Basis of the 5e-5: the fp32 numpy emulation of the same
arithmetic (`dark_ref(fp32=True)`) differs from float64 by at most 3.1e-6 px on this family (noise 1e-2), the
reference's own mixed-precision code by 2.0e-6 ... 3.7e-6; the 20x margin covers logf against numpy's log, another
summation order and the fp32 rounding of a coordinate near 100.  The fixture is compared in image pixels: 1e-3, the
project's figure for fp32 affine arithmetic against float64 (g12).  All requirements on the inputs (enough maps take
the Newton step, |det| >= 1e-3 there, every planted case is what it claims, no non-finite ratio on a positive map) are
asserted on the float64 reference before any launch.  The largest deviation seen on the GPU is recorded in
docs/HISTORY.md."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _dark_ref as dr  # noqa: E402

import fami_pose_amd as fp  # noqa: E402
from fami_pose_amd import evaluate as ev, loss as FL  # noqa: E402
from fami_pose_amd._lib import lib  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_HM = 5e-5
TOL_IMG = 1e-3
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dark_final_preds.npz')
# (shape, k): 96x72 is the W48 evaluation map and 128x96 the largest of BASELINE.json; 24x18 at the smallest, the default
# and the largest kernel; odd sizes that are no multiple of anything; a map smaller than the kernel
CASES = [((2, 17, 96, 72), 11), ((3, 5, 24, 18), 11), ((3, 5, 24, 18), 9), ((3, 5, 24, 18), 17), ((2, 3, 17, 13), 11),
         ((1, 2, 8, 6), 11), ((1, 2, 128, 96), 11)]
EDGES = ('0', '1', '2', 'n-3', 'n-2', 'n-1')


def _edge(n):
    return [0, 1, 2, n - 3, n - 2, n - 1]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _identity(B, H, W):
    """-> center, scale [B,2] float32 for which transform_preds is the identity in fp32 (the factor is exactly 1)"""
    assert np.float32(np.float32(W / 200) * np.float32(200)) / np.float32(W) == 1
    return (np.tile(np.array([[W / 2, H / 2]], np.float32), (B, 1)),
            np.tile(np.array([[W / 200, H / 200]], np.float32), (B, 1)))


def _peak(rng, H, W, px, py, amp=0.8, noise=1e-2):
    """a sigma-3 peak centred on the pixel (px, py) with noise, and that pixel made the strict maximum"""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    m = amp * np.exp(-((xx - px) ** 2 + (yy - py) ** 2) / 18.0) + noise * rng.standard_normal((H, W))
    m = m.astype(np.float32)
    m[py, px] = m.max() + np.float32(0.05)
    return m


def _plant(hm, rng):
    """Replaces hm[1, 0..15] of the 96x72 stack by the planted cases -> {name: (b, j, px, py)} (px = None: no peak)."""
    H, W = hm.shape[2:]
    where = {}
    for i, (nm, px) in enumerate(zip(EDGES, _edge(W))):              # the guard 1 < px < W-2, at both of its ends
        hm[1, i] = _peak(rng, H, W, px, H // 2)
        where['x=' + nm] = (1, i, px, H // 2)
    for i, (nm, py) in enumerate(zip(EDGES, _edge(H))):              # 1 < py < H-2
        hm[1, 6 + i] = _peak(rng, H, W, W // 2, py)
        where['y=' + nm] = (1, 6 + i, W // 2, py)
    hm[1, 12] = 0.0
    where['zero'] = (1, 12, None, None)
    hm[1, 13] = -np.abs(hm[1, 13]) - np.float32(1e-3)
    where['negative'] = (1, 13, None, None)
    hm[1, 14] = _peak(rng, H, W, 30, 40)
    hm[1, 14, 60, 40] = hm[1, 14, 40, 30]                            # the same value again at a later flat index
    where['tie'] = (1, 14, 30, 40)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)                   # mirror-symmetric about its centre pixel, no noise
    hm[1, 15] = (0.7 * np.exp(-((xx - 36) ** 2 + (yy - 48) ** 2) / 18.0)).astype(np.float32)
    where['symmetric'] = (1, 15, 36, 48)
    return where


def _build():
    """Every case of the family with its float64 reference, and the assertions the issue wants made on the reference."""
    fam = []
    for n, (shape, k) in enumerate(CASES):
        rng = np.random.RandomState(300 + n)         # (seeds 100 ... 500 give 44 ... 47 of the 89 maps in the branch; the
                                                     # assertion below wants half, and 10 planted maps are outside by design)
        hm = dr.make_maps(rng, *shape)
        planted = _plant(hm, rng) if shape == (2, 17, 96, 72) else {}
        B, J, H, W = shape
        center, scale = _identity(B, H, W)
        ref = dr.dark_ref(hm, center, scale, k)
        fam.append({'shape': shape, 'k': k, 'hm': hm, 'center': center, 'scale': scale, 'ref': ref, 'planted': planted})
    maps = sum(f['ref']['branch'].size for f in fam)
    taken = sum(int(f['ref']['moved'].sum()) for f in fam)
    dets = np.concatenate([np.abs(f['ref']['det'][f['ref']['branch']]) for f in fam])
    print('family: %d of %d maps take the Newton step, |det| >= %.2e' % (taken, maps, dets.min()))
    assert 2 * taken >= maps
    assert dets.min() >= 1e-3
    for f in fam:
        r = f['ref']
        assert np.isfinite(r['ratio'][r['maxvals'][..., 0] > 0]).all()
        assert np.array_equal(r['moved'], r['branch'])
    big = fam[0]
    r, hm = big['ref'], big['hm']
    H, W = big['shape'][2:]
    for nm, (b, j, px, py) in big['planted'].items():
        if px is None:
            assert (r['maxvals'][b, j, 0] == 0) if nm == 'zero' else (r['maxvals'][b, j, 0] < 0)
            assert np.array_equal(r['intc'][b, j], [0, 0]) and not r['branch'][b, j]
            continue
        assert np.array_equal(r['intc'][b, j], [px, py]), nm
        assert r['branch'][b, j] == (1 < px < W - 2 and 1 < py < H - 2), nm
    for nm in ('x=2', 'x=n-3', 'y=2', 'y=n-3', 'tie', 'symmetric'):
        assert r['branch'][big['planted'][nm][:2]], nm
    for nm in ('x=0', 'x=1', 'x=n-2', 'x=n-1', 'y=0', 'y=1', 'y=n-2', 'y=n-1'):
        assert not r['branch'][big['planted'][nm][:2]], nm
    b, j = big['planted']['tie'][:2]
    assert (hm[b, j] == hm[b, j].max()).sum() == 2 and hm[b, j].reshape(-1).argmax() == 40 * W + 30 < 60 * W + 40
    b, j = big['planted']['symmetric'][:2]
    assert np.array_equal(hm[b, j, 48 - 35:48 + 36, 36 - 35:36 + 36], hm[b, j, 48 - 35:48 + 36, 36 - 35:36 + 36][::-1, ::-1])
    assert np.abs(r['coords'][b, j] - r['intc'][b, j]).max() < 1e-12         # its offset is 0 up to float64 rounding
    return fam


_FAMILY = []


@pytest.fixture(scope='module')
def family():
    if not _FAMILY:
        _FAMILY.extend(_build())
    return _FAMILY


# ---------------------------------------------------------------------------------------- 1. against float64
@pytest.mark.parametrize('n', range(len(CASES)), ids=['%dx%dx%dx%d-k%d' % (s + (k,)) for s, k in CASES])
def test_against_float64_in_heatmap_pixels(dev, family, n):
    f = family[n]
    r, k = f['ref'], f['k']
    hm = torch.from_numpy(f['hm']).to(dev)
    preds, maxvals = FL.dark_get_final_preds(hm, f['center'], f['scale'], blur_kernel=k)
    p_std, m_std = FL.get_final_preds(hm, f['center'], f['scale'])
    assert preds.shape == f['shape'][:2] + (2,) and maxvals.shape == f['shape'][:2] + (1,)
    got, p_std = preds.cpu().numpy(), p_std.cpu().numpy()
    # maxvals and the integer coordinates: those of get_final_preds (its quarter-pixel shift rounds away exactly), and the
    # reference's
    assert np.array_equal(_bits(maxvals.cpu().numpy()), _bits(m_std.cpu().numpy()))
    assert np.array_equal(_bits(maxvals.cpu().numpy()), _bits(r['maxvals']))
    intc = r['intc'].astype(np.float32)
    assert np.array_equal(np.rint(p_std), intc)
    # the branch decision: a map outside the guard comes back as its integer coordinate, bit for bit
    stay = ~r['moved']
    assert np.array_equal(_bits(got[stay]), _bits(intc[stay]))
    far = np.abs(r['coords'] - r['intc']).max(-1) > 1e-4
    assert (got[far] != intc[far]).any(-1).all()                     # ... and one inside it has moved
    err = np.abs(got.astype(np.float64) - r['coords'])
    print('%s k=%d: %d of %d maps refined, max |gpu - float64| = %.3e heatmap px (largest offset %.3f)'
          % (f['shape'], k, r['moved'].sum(), r['moved'].size, err.max(), np.abs(r['coords'] - r['intc']).max()))
    assert err.max() <= TOL_HM
    if f['planted']:
        b, j = f['planted']['symmetric'][:2]                        # the blur sums mirror pairs: a gradient of exactly 0
        assert np.array_equal(_bits(got[b, j]), _bits(intc[b, j]))
    # the standard decode is another function of the same maps: the keyword is no no-op
    if r['moved'].any():
        assert not np.array_equal(got, p_std)


# ---------------------------------------------------------------------------------------- 2. the fixture
def test_reference_fixture(dev):
    g = np.load(GOLD)
    preds, maxvals = FL.dark_get_final_preds(torch.from_numpy(g['hm']).to(dev), g['center'], g['scale'])
    err = np.abs(preds.cpu().numpy().astype(np.float64) - g['preds']).max()
    print('fixture: max |gpu - reference| = %.3e image px' % err)
    assert np.array_equal(maxvals.cpu().numpy(), g['maxvals'])
    assert err < TOL_IMG


# ---------------------------------------------------------------------------------------- 3. memory
GUARD = 256
SENT = 0x5a5a5a5a


def _corner_maps(shape, seed):
    """maps whose peaks sit at (2, 2) and (W-3, H-3): inside the guard, and the stencil's blur reaches every halo"""
    B, J, H, W = shape
    rng = np.random.RandomState(seed)
    hm = dr.make_maps(rng, B, J, H, W)
    hm[0, 0] = _peak(rng, H, W, 2, 2)
    hm[-1, -1] = _peak(rng, H, W, W - 3, H - 3)
    return hm


@pytest.mark.parametrize('shape', [(2, 3, 17, 13), (1, 2, 8, 6)])
def test_nothing_outside_the_arguments_is_read_or_written(dev, shape):
    B, J, H, W = shape
    hm = _corner_maps(shape, 31)
    center, scale = _identity(B, H, W)
    r = dr.dark_ref(hm, center, scale, 11)
    assert r['moved'][0, 0] and r['moved'][-1, -1]
    n = hm.size
    plain = torch.from_numpy(hm).to(dev)
    p0, m0 = FL.dark_get_final_preds(plain, center, scale)
    assert np.abs(p0.cpu().numpy() - r['coords']).max() <= TOL_HM

    poisoned = torch.full((GUARD + n + GUARD,), float('nan'), device=dev)
    poisoned[GUARD:GUARD + n] = plain.reshape(-1)
    pb = torch.full((GUARD + B * J * 2 + GUARD,), SENT, dtype=torch.int32, device=dev)
    mb = torch.full((GUARD + B * J + GUARD,), SENT, dtype=torch.int32, device=dev)
    c, s = torch.from_numpy(center).to(dev), torch.from_numpy(scale).to(dev)
    taps = torch.from_numpy(FL.gaussian_taps(11)).to(dev)
    lib().call('fami_dark_preds_f32', poisoned[GUARD:].data_ptr(), c.data_ptr(), s.data_ptr(), taps.data_ptr(), 11,
               pb[GUARD:].data_ptr(), mb[GUARD:].data_ptr(), B, J, H, W, _stream(dev))
    pg, mg = pb.cpu().numpy(), mb.cpu().numpy()
    for buf, m in ((pg, B * J * 2), (mg, B * J)):
        assert (buf[:GUARD] == SENT).all() and (buf[GUARD + m:] == SENT).all()
    assert np.array_equal(pg[GUARD:GUARD + B * J * 2], _bits(p0.cpu().numpy()).reshape(-1))
    assert np.array_equal(mg[GUARD:GUARD + B * J], _bits(m0.cpu().numpy()).reshape(-1))
    assert torch.isnan(poisoned[:GUARD]).all() and torch.isnan(poisoned[GUARD + n:]).all()
    assert torch.equal(poisoned[GUARD:GUARD + n], plain.reshape(-1))             # hm is only read


# ---------------------------------------------------------------------------------------- 4. refusals
def test_refusals(dev):
    c = lib().cdll
    B, J, H, W = 1, 1, 24, 18
    hm = torch.zeros(B, J, H, W, device=dev)
    cs = torch.ones(B, 2, device=dev)
    taps = torch.from_numpy(FL.gaussian_taps(17)).to(dev)
    pb = torch.full((B * J * 2,), SENT, dtype=torch.int32, device=dev)
    mb = torch.full((B * J,), SENT, dtype=torch.int32, device=dev)

    def call(hm, k, H, W):
        return c.fami_dark_preds_f32(hm.data_ptr(), cs.data_ptr(), cs.data_ptr(), taps.data_ptr(), k, pb.data_ptr(),
                                     mb.data_ptr(), B, J, H, W, _stream(dev))

    for k in (7, 12, 3, 5, 19, 0, -11):
        assert call(hm, k, H, W) == -1, k
    assert b'fami_dark_preds_f32' in c.fami_last_error()
    # the size limit: the padded map and its row pass must fit the LDS of one CU
    Hb, Wb = 256, 192
    limit = c.fami_dark_preds_lds_limit()
    assert c.fami_dark_preds_lds_bytes(Hb, Wb, 11) > limit
    big = torch.zeros(B, J, Hb, Wb, device=dev)
    assert call(big, 11, Hb, Wb) == -2
    assert str(limit).encode() in c.fami_last_error()
    with pytest.raises(ValueError, match=str(limit)):
        FL.dark_get_final_preds(big, np.ones((B, 2)), np.ones((B, 2)))
    torch.cuda.synchronize(dev)
    assert (pb.cpu().numpy() == SENT).all() and (mb.cpu().numpy() == SENT).all()     # no refusal wrote anything
    for kk in (7, 12):
        with pytest.raises(ValueError):
            FL.dark_get_final_preds(hm, np.ones((B, 2)), np.ones((B, 2)), blur_kernel=kk)
    assert call(hm, 17, H, W) == 0                                                # the arguments themselves were fine
    torch.cuda.synchronize(dev)
    assert (mb.cpu().numpy() == 0).all()                                          # maxvals of the all-zero map


# ---------------------------------------------------------------------------------------- 5. the front door
S, HI, WI, B = 2, 128, 96, 2
CENTER = np.array([[320.0, 240.5], [100.25, 400.0]], np.float32)
SCALE = np.array([[1.5, 2.0], [0.9, 1.2]], np.float32)


def _clips(seed, b):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(b, 3, HI, WI, generator=gen), torch.randn(b, 3 * S, HI, WI, generator=gen)


@pytest.fixture(scope='module')
def e2e(dev):
    from fami_pose_amd.init import realistic_init_
    torch.manual_seed(5)
    model = fp.build_model(fp.default_cfg(48, image_size=(WI, HI), num_sup=S), fp.VAL_PHASE)
    realistic_init_(model, seed=5)
    model = model.to(dev).eval()
    kf, sup = _clips(55, B)
    return {'model': model, 'kf': kf.to(dev), 'sup': sup.to(dev)}


@pytest.mark.parametrize('flip', [False, True])
def test_predict_dark_is_the_decode_of_its_own_map(dev, e2e, flip):
    model, kf, sup = e2e['model'], e2e['kf'], e2e['sup']
    preds, maxvals, final_hm = ev.predict(model, kf, sup, CENTER, SCALE, flip=flip, decode='dark')
    p_std, m_std, hm_std = ev.predict(model, kf, sup, CENTER, SCALE, flip=flip)
    assert torch.equal(final_hm, hm_std)                             # the forward (and the merge) do not depend on the decode
    p1, m1 = FL.dark_get_final_preds(final_hm, CENTER, SCALE)
    assert torch.equal(preds, p1) and torch.equal(maxvals, m1)
    assert torch.equal(maxvals, m_std) and not torch.equal(preds, p_std)
    pk, _, _ = ev.predict(model, kf, sup, CENTER, SCALE, flip=flip, decode='dark', blur_kernel=17)
    assert torch.equal(pk, FL.dark_get_final_preds(final_hm, CENTER, SCALE, blur_kernel=17)[0]) and not torch.equal(pk, preds)
    ref = dr.dark_ref(final_hm.cpu().numpy(), CENTER, SCALE, 11)
    err = np.abs(preds.cpu().numpy() - ref['preds']).max()
    print('predict(decode=dark, flip=%s): %d of 34 maps refined, |gpu - float64| = %.3e image px' % (flip, ref['moved'].sum(), err))
    assert err < TOL_IMG


def test_evaluate_loop_dark(dev, e2e):
    """Two batches (2 clips, 1 clip): all_preds / all_bb are the DARK decode of both heads; the PCK counters are those of
    the standard loop (PCK stays on the argmax)."""
    model = e2e['model']
    batches, want = [], [[], []]
    for k, b in enumerate((2, 1)):
        kf, sup = _clips(60 + k, b)
        gen = torch.Generator().manual_seed(65 + k)
        joints = torch.rand(b, 17, 2, generator=gen) * torch.tensor([WI, HI], dtype=torch.float32)
        vis = (torch.rand(b, 17, generator=gen) < 0.8).float()
        target, _ = FL.generate_heatmaps(joints.to(dev), vis.to(dev), 3, (WI, HI), (WI // 4, HI // 4))
        meta = {'image': ['images/val/v%d/%08d.jpg' % (k, i + 1) for i in range(b)], 'center': CENTER[:b] + k,
                'scale': SCALE[:b], 'score': np.linspace(0.5, 0.9, b)}
        batches.append((kf, sup, target.cpu(), meta))
        with torch.no_grad():
            out = model(kf.to(dev), sup.to(dev))
        for head in range(2):
            p, m = FL.dark_get_final_preds(out[head], meta['center'], meta['scale'])
            want[head].append(np.concatenate([p.cpu().numpy(), m.cpu().numpy()], 2).astype(np.float64))
    acc = ev.evaluate_loop(model, batches, 3, decode='dark')
    std = ev.evaluate_loop(model, batches, 3)
    assert acc.idx == 3
    assert np.array_equal(acc.all_preds, np.concatenate(want[0], 0))
    assert np.array_equal(acc.all_bb, np.concatenate(want[1], 0))
    assert not np.array_equal(acc.all_preds[:, :, :2], std.all_preds[:, :, :2])
    assert not np.array_equal(acc.all_bb[:, :, :2], std.all_bb[:, :, :2])
    assert np.array_equal(acc.all_preds[:, :, 2], std.all_preds[:, :, 2])          # the confidences are the same maxima
    assert acc.acc_sum == std.acc_sum and acc.acc_cnt == std.acc_cnt and acc.acc_cnt[0] > 0
    assert np.array_equal(acc.all_boxes, std.all_boxes) and acc.filenames_map == std.filenames_map


def test_standard_decode_is_the_call_without_the_keyword(dev, e2e):
    model, kf, sup = e2e['model'], e2e['kf'], e2e['sup']
    ev.predict(model, kf, sup, CENTER, SCALE)                        # warm-up of this batch size
    n0 = lib().ncalls
    a = ev.predict(model, kf, sup, CENTER, SCALE)
    n_a = lib().ncalls - n0
    n0 = lib().ncalls
    b = ev.predict(model, kf, sup, CENTER, SCALE, decode='standard', blur_kernel=17)   # blur_kernel belongs to 'dark'
    n_b = lib().ncalls - n0
    n0 = lib().ncalls
    d = ev.predict(model, kf, sup, CENTER, SCALE, decode='dark')
    n_d = lib().ncalls - n0
    assert n_a == n_b == n_d                                         # one decode entry point either way
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(a[0], d[0])
    kf2, sup2 = _clips(70, 1)
    meta = {'image': ['images/val/v0/00000001.jpg'], 'center': CENTER[:1], 'scale': SCALE[:1], 'score': np.array([0.7])}
    runs = []
    for kw in ({}, {'decode': 'standard'}):
        n0 = lib().ncalls
        acc = ev.evaluate_loop(model, [(kf2, sup2, None, meta)], 1, **kw)
        runs.append((lib().ncalls - n0, acc))
    assert runs[0][0] == runs[1][0]
    assert np.array_equal(runs[0][1].all_preds, runs[1][1].all_preds) and np.array_equal(runs[0][1].all_bb, runs[1][1].all_bb)
