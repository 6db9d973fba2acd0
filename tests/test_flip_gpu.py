"""Flip testing on the MI355X (fami_pose_amd.evaluate: mirror_cat, flip_merge, predict / evaluate_loop with flip=True):
the clip and its horizontal mirror through ONE forward as a doubled batch, the mirrored half's heatmaps mirrored back
with the left/right joint channels exchanged (flip_back, datasets/process/pose_process.py:29-42), optionally shifted by
one column (HRNet's flipped[..., 1:] = flipped.clone()[..., :-1]) and averaged with the plain half.

Bounds: both kernels are exact -- the mirror is a copy, the merge one fp32 add and one fp32 multiply by 0.5, which numpy
rounds identically -- so they are compared as int32 bit patterns.  The forward has a fixed summation order
(test_train_gpu.py:6-7), so predict(flip=True) is bit-equal to the host merge of the model's own doubled-batch forward.
Against the CPU oracle the merged map keeps the project's heatmap tolerance HM_TOL = 1e-3: the average of two maps that
each lie within HM_TOL of the oracle's lies within HM_TOL of the oracle's average."""
import numpy as np
import pytest
import torch

import fami_pose_amd as fp
from fami_pose_amd import evaluate as ev, loss as FL
from fami_pose_amd._lib import lib
from fami_pose_amd.data import FLIP_PAIRS
from oracle import model as om, ops as oops

pytestmark = pytest.mark.gpu

HM_TOL = 1e-3
S, H, W, B = 2, 128, 96, 2
CENTER = np.array([[320.0, 240.5], [100.25, 400.0]], np.float32)        # test_predict_end_to_end's boxes
SCALE = np.array([[1.5, 2.0], [0.9, 1.2]], np.float32)


def ref(hm2, perm, shift):
    B = hm2.shape[0] // 2
    fb = hm2[B:][:, perm][:, :, :, ::-1].copy()
    if shift:
        s = fb.copy()
        s[..., 1:] = fb[..., :-1]
        fb = s
    return (hm2[:B] + fb) * np.float32(0.5)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def test_ref_restates_flip_back():
    """`ref` against the semantics of the reference's flip_back for the full COCO pairing: every element of the mirrored
    half encodes (joint, column); after mirroring back, channel a of a pair (a, b) holds joint b's map and column x holds
    what was at W-1-x.  With the shift, column x >= 1 holds the unshifted column x-1 and column 0 keeps its value."""
    Bq, J, Hq, Wq = 2, 17, 3, 8
    enc = (np.arange(J, dtype=np.float32)[:, None] * 100 + np.arange(Wq, dtype=np.float32)[None, :])      # [J, W]
    hm2 = np.zeros((2 * Bq, J, Hq, Wq), np.float32)
    hm2[Bq:] = enc[None, :, None, :]
    partner = list(range(J))
    for a, b in FLIP_PAIRS:
        partner[a], partner[b] = b, a
    want = np.empty((Bq, J, Hq, Wq), np.float32)
    for j in range(J):
        for x in range(Wq):
            want[:, j, :, x] = partner[j] * 100 + (Wq - 1 - x)
    perm = ev.flip_perm(J)
    assert np.array_equal(ref(hm2, perm, False) * 2, want)
    shifted = want.copy()
    shifted[..., 1:] = want[..., :-1]
    assert np.array_equal(ref(hm2, perm, True) * 2, shifted)
    assert np.array_equal(shifted[..., 0], want[..., 0]) and np.array_equal(shifted[..., 1], want[..., 0])


# ---------------------------------------------------------------------------------------- mirror_cat
def _bit_patterns(shape, seed):
    """random 32-bit patterns viewed as floats: NaNs of every payload, infinities, -0, denormals"""
    rng = np.random.RandomState(seed)
    a = rng.randint(-2 ** 31, 2 ** 31, size=shape, dtype=np.int64).astype(np.int32)
    flat = a.reshape(-1)
    for k, v in enumerate((0x7fc00000, 0x7f800001, -0x00800000, -0x80000000, 0x7f800000, 0x00000001)):
        if k < flat.size:            # quiet NaN, signalling NaN, -inf, -0, +inf, smallest denormal
            flat[(k * 7919) % flat.size] = v
    return a


@pytest.mark.parametrize('shape', [(1, 1, 1, 1), (1, 3, 2, 7), (2, 3, 5, 30), (2, 9, 8, 24), (1, 3, 16, 96), (3, 2, 3, 260)])
def test_mirror_cat_copies_every_bit_pattern(dev, shape):
    a = _bit_patterns(shape, 11)
    x = torch.from_numpy(a).view(torch.float32).to(dev)
    out = ev.mirror_cat(x)
    assert out.shape == (2 * shape[0],) + shape[1:] and out.dtype == torch.float32 and out.is_contiguous()
    want = np.concatenate([a, a[:, :, :, ::-1]], 0)
    assert np.array_equal(out.view(torch.int32).cpu().numpy(), want)
    assert np.array_equal(x.view(torch.int32).cpu().numpy(), a)                  # the input is only read


@pytest.mark.parametrize('shape', [(2, 5, 820, 260), (1, 2, 1051, 259)])
def test_mirror_cat_beyond_one_grid(dev, shape):
    """More 16-byte chunks (first shape) / elements (second) than the 2048 x 256 threads of the largest grid: the
    grid-stride loop takes a second trip with the row and column advanced by the split stride."""
    assert (shape[0] * shape[1] * shape[2] * shape[3]) // (4 if shape[3] % 4 == 0 else 1) > 2048 * 256
    a = _bit_patterns(shape, 14)
    out = ev.mirror_cat(torch.from_numpy(a).view(torch.float32).to(dev))
    assert np.array_equal(out.view(torch.int32).cpu().numpy(), np.concatenate([a, a[:, :, :, ::-1]], 0))


def test_mirror_cat_misaligned_base_takes_the_scalar_path(dev):
    """W = 24 would allow 16-byte accesses, the bases 4 bytes into their buffers do not."""
    rows, Wq = 2 * 9 * 8, 24
    n = rows * Wq
    a = _bit_patterns((rows, Wq), 12)
    bx = torch.zeros(n + 8, dtype=torch.int32, device=dev)
    bo = torch.full((2 * n + 8,), 0x5a5a5a5a, dtype=torch.int32, device=dev)
    bx[1:1 + n] = torch.from_numpy(a.reshape(-1)).to(dev)
    x, out = bx[1:1 + n], bo[1:1 + 2 * n]
    assert x.data_ptr() % 16 == 4 and out.data_ptr() % 16 == 4
    lib().call('fami_mirror_cat_f32', x.data_ptr(), out.data_ptr(), rows, Wq, _stream(dev))
    got = bo.cpu().numpy()
    assert np.array_equal(got[1:1 + 2 * n].reshape(2 * rows, Wq), np.concatenate([a, a[:, ::-1]], 0))
    assert (got[:1] == 0x5a5a5a5a).all() and (got[1 + 2 * n:] == 0x5a5a5a5a).all()      # nothing outside out is written


def test_bad_arguments_are_refused(dev):
    from fami_pose_amd._lib import FamiError
    t = torch.zeros(64, device=dev)
    p = torch.zeros(4, dtype=torch.int32, device=dev)
    s = _stream(dev)
    for args in ((None, t.data_ptr(), 1, 4), (t.data_ptr(), None, 1, 4), (t.data_ptr(), t[32:].data_ptr(), 0, 4),
                 (t.data_ptr(), t[32:].data_ptr(), 1, 0), (t.data_ptr(), t[4:].data_ptr(), 2, 4)):       # last: overlap
        with pytest.raises(FamiError):
            lib().call('fami_mirror_cat_f32', *args, s)
    for args in ((None, p.data_ptr(), t.data_ptr(), 1, 1, 1, 4, 0), (t.data_ptr(), None, t[32:].data_ptr(), 1, 1, 1, 4, 0),
                 (t.data_ptr(), p.data_ptr(), None, 1, 1, 1, 4, 0), (t.data_ptr(), p.data_ptr(), t[32:].data_ptr(), 0, 1, 1, 4, 0),
                 (t.data_ptr(), p.data_ptr(), t[32:].data_ptr(), 1, 1, 1, -4, 0),
                 (t.data_ptr(), p.data_ptr(), t[4:].data_ptr(), 1, 1, 1, 4, 0)):                          # last: overlap
        with pytest.raises(FamiError):
            lib().call('fami_flip_merge_f32', *args, s)
    assert lib().cdll.fami_mirror_cat_f32(None, None, 1, 1, None) == -1
    assert lib().cdll.fami_flip_merge_f32(None, None, None, 1, 1, 1, 1, 0, None) == -1
    with pytest.raises(ValueError):
        ev.flip_merge(torch.zeros(3, 5, 2, 2, device=dev))                       # an odd batch is no doubled batch
    with pytest.raises(ValueError):
        ev.flip_merge(torch.zeros(2, 5, 2, 2, device=dev), pairs=((0, 5),))
    with pytest.raises(RuntimeError):
        ev.mirror_cat(torch.zeros(1, 1, 2, 2))                                   # device only, like loss.py


# ---------------------------------------------------------------------------------------- flip_merge
_PAIRS = {17: FLIP_PAIRS, 5: ((0, 4), (1, 2)), 1: ()}


def _planted(shape, pairs, seed):
    """randn [2B,J,H,W] with +inf, -inf, NaN and -0.0 planted.  -0.0 sits at [0,0,0,0] and at the element it is averaged
    with in either shift mode, so the result there is -0.0 itself; a map of two elements has room for that pair only."""
    Bq, J, Hq, Wq = shape
    hm2 = np.random.RandomState(seed).randn(2 * Bq, J, Hq, Wq).astype(np.float32)
    perm = ev.flip_perm(J, pairs)
    flat = hm2.reshape(-1)
    for k, v in enumerate((np.inf, -np.inf, np.nan, np.inf, -np.inf, np.nan)):
        if flat.size >= 16:
            flat[1 + k * (flat.size // 6)] = v                                   # spread over both halves
    hm2[0, 0, 0, 0] = -0.0
    hm2[Bq, perm[0], 0, Wq - 1] = -0.0
    return hm2, perm


@pytest.mark.parametrize('shift', [False, True])
@pytest.mark.parametrize('shape', [(1, 1, 1, 1), (1, 17, 3, 7), (2, 17, 8, 6), (2, 17, 32, 24), (1, 17, 96, 72), (3, 5, 2, 258)])
def test_flip_merge_is_bitwise_the_numpy_statement(dev, shape, shift):
    pairs = _PAIRS[shape[1]]
    hm2, perm = _planted(shape, pairs, 13)
    want = ref(hm2, perm, shift)
    t = torch.from_numpy(hm2).to(dev)
    got = ev.flip_merge(t, pairs, shift)
    assert got.shape == shape and got.dtype == torch.float32
    got = got.cpu().numpy()
    nan = np.isnan(want)
    if hm2.size >= 16:
        assert nan.any() and np.isinf(want).any()
    assert _bits(want)[0, 0, 0, 0] == -2 ** 31                                   # -0.0 survives the average
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan])
    assert np.array_equal(_bits(t.cpu().numpy()), _bits(hm2))                    # hm2 is only read


@pytest.mark.parametrize('shape', [(2, 17, 250, 260), (1, 5, 410, 259)])
def test_flip_merge_beyond_one_grid(dev, shape):
    """As test_mirror_cat_beyond_one_grid: a second trip of the grid-stride loop on the 16-byte and the scalar path."""
    assert (shape[0] * shape[1] * shape[2] * shape[3]) // (4 if shape[3] % 4 == 0 else 1) > 2048 * 256
    pairs = _PAIRS[shape[1]]
    hm2, perm = _planted(shape, pairs, 15)
    for shift in (False, True):
        want = ref(hm2, perm, shift)
        got = ev.flip_merge(torch.from_numpy(hm2).to(dev), pairs, shift).cpu().numpy()
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


# ---------------------------------------------------------------------------------------- end to end
def _pair(seed):
    orc = om.realistic_init_(om.AlignmentOracle(om.make_cfg(48), False, S, (H, W)), seed)
    model = fp.build_model(fp.default_cfg(48, image_size=(W, H), num_sup=S), fp.VAL_PHASE)
    model.load_state_dict(orc.state_dict())
    return model, orc.eval()


def _clips(seed, b):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(b, 3, H, W, generator=gen), torch.randn(b, 3 * S, H, W, generator=gen)


@pytest.fixture(scope='module')
def e2e(dev):
    """One model / oracle pair and everything the end-to-end tests compare against, computed once: the model's own
    forward on torch.cat([x, x.flip(3)]) (both heads, on the host) and the oracle's outputs for x and for x.flip(3)."""
    model, orc = _pair(7)
    model = model.to(dev).eval()
    kf, sup = _clips(77, B)
    with torch.no_grad():
        own = model(torch.cat([kf, kf.flip(3)]).to(dev), torch.cat([sup, sup.flip(3)]).to(dev))
        o_plain = orc(kf, sup)
        o_mirr = orc(kf.flip(3), sup.flip(3))
    return {'model': model, 'kf': kf.to(dev), 'sup': sup.to(dev), 'perm': ev.flip_perm(17),
            'own': [o.cpu().numpy() for o in own[:2]],
            'orc': [np.concatenate([a.numpy(), b.numpy()], 0) for a, b in zip(o_plain[:2], o_mirr[:2])]}


@pytest.mark.parametrize('sh', [False, True])
def test_predict_flip_end_to_end(dev, e2e, sh):
    preds, maxvals, final_hm = ev.predict(e2e['model'], e2e['kf'], e2e['sup'], CENTER, SCALE, flip=True, shift_heatmap=sh)
    hm = final_hm.cpu().numpy()
    assert hm.shape == (B, 17, H // 4, W // 4)
    # (a) bit-equal to the host merge of the model's own doubled-batch forward
    assert np.array_equal(_bits(hm), _bits(ref(e2e['own'][0], e2e['perm'], sh)))
    # (b) the oracle's two forwards, merged the same way
    want = ref(e2e['orc'][0], e2e['perm'], sh)
    err = np.abs(hm - want).max()
    plain = e2e['orc'][0][:B]
    moved = int((want.reshape(B * 17, -1).argmax(1) != plain.reshape(B * 17, -1).argmax(1)).sum())
    print('flip end to end (shift=%s): |final_hm - oracle merge| %.3e; merge changes the oracle map by up to %.3f and moves '
          '%d of %d argmaxes' % (sh, err, np.abs(want - plain).max(), moved, B * 17))
    assert err < HM_TOL
    assert np.abs(want - plain).max() > 0.1                     # the merge is no no-op on this model
    # (c) the decode ran on the merged map
    p1, m1 = FL.get_final_preds(final_hm, CENTER, SCALE)
    assert torch.equal(preds, p1) and torch.equal(maxvals, m1)
    p0, m0 = oops.get_final_preds(hm.copy(), CENTER, SCALE)
    assert np.array_equal(maxvals.cpu().numpy(), m0)
    assert np.abs(preds.cpu().numpy().astype(np.float64) - p0).max() < 1e-3


def test_predict_without_flip_is_the_plain_call(dev, e2e):
    """(d) flip=False: today's result bit for bit, and the same number of library calls as forward + decode."""
    model, kf, sup = e2e['model'], e2e['kf'], e2e['sup']
    with torch.no_grad():
        hm0 = model(kf, sup)[0]                                  # (also the warm-up of this batch size)
        n0 = lib().ncalls
        hm0 = model(kf, sup)[0]
        p0, m0 = FL.get_final_preds(hm0, CENTER, SCALE)
        n_plain = lib().ncalls - n0
    n0 = lib().ncalls
    pa, ma, ha = ev.predict(model, kf, sup, CENTER, SCALE)
    n_a = lib().ncalls - n0
    n0 = lib().ncalls
    pb, mb, hb = ev.predict(model, kf, sup, CENTER, SCALE, flip=False, shift_heatmap=True)     # the shift belongs to the merge
    n_b = lib().ncalls - n0
    assert n_a == n_plain and n_b == n_plain
    for p, m, h in ((pa, ma, ha), (pb, mb, hb)):
        assert torch.equal(h, hm0) and torch.equal(p, p0) and torch.equal(m, m0)
    n0 = lib().ncalls
    ev.predict(model, kf, sup, CENTER, SCALE, flip=True)
    assert lib().ncalls - n0 > n_plain                           # the counter does see the flip path


def test_forward_buffers_are_released_without_the_cycle_collector(dev, e2e):
    """An Engine keeps every buffer of its forward until the forward is enqueued; it must then go by reference count.  (Its
    routed-query helper used to hold it strongly: a cycle, and every inference call left its activations allocated until
    the cycle collector ran -- which the doubled batch of a flip call doubles.)"""
    import gc
    model, kf, sup = e2e['model'], e2e['kf'], e2e['sup']
    ev.predict(model, kf, sup, CENTER, SCALE, flip=True)         # warm-up: the cached permutation, workspaces
    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        torch.cuda.synchronize(dev)
        m0 = torch.cuda.memory_allocated(dev)
        for flip in (False, True, True):
            ev.predict(model, kf, sup, CENTER, SCALE, flip=flip)
            torch.cuda.synchronize(dev)
            assert torch.cuda.memory_allocated(dev) == m0, flip
    finally:
        if was:
            gc.enable()


def test_flip_needs_eval_mode(dev, e2e):
    model = e2e['model']
    model.train()
    try:
        with pytest.raises(RuntimeError):
            ev.predict(model, e2e['kf'], e2e['sup'], CENTER, SCALE, flip=True)
    finally:
        model.eval()


@pytest.mark.parametrize('sh', [False, True])
def test_evaluate_loop_flip(dev, e2e, sh):
    """Two batches (2 clips, 1 clip): all_preds / all_bb rows are the decode of the merged maps of both heads, and the PCK
    counters are fami_pck_accuracy_f32 on the merged maps."""
    model, perm = e2e['model'], e2e['perm']
    batches, want_rows, want_acc = [], [[], []], [[0.0, 0], [0.0, 0]]
    for k, b in enumerate((2, 1)):
        kf, sup = _clips(90 + k, b)
        gen = torch.Generator().manual_seed(95 + k)
        joints = torch.rand(b, 17, 2, generator=gen) * torch.tensor([W, H], dtype=torch.float32)
        vis = (torch.rand(b, 17, generator=gen) < 0.8).float()
        target, _ = FL.generate_heatmaps(joints.to(dev), vis.to(dev), 3, (W, H), (W // 4, H // 4))
        meta = {'image': ['images/val/v%d/%08d.jpg' % (k, i + 1) for i in range(b)], 'center': CENTER[:b] + k,
                'scale': SCALE[:b], 'score': np.linspace(0.5, 0.9, b)}
        batches.append((kf, sup, target.cpu(), meta))
        with torch.no_grad():
            own = model(torch.cat([kf, kf.flip(3)]).to(dev), torch.cat([sup, sup.flip(3)]).to(dev))
        rows = torch.empty(2, 20, device=dev)
        iws, mws = torch.empty(2 * b * 17, dtype=torch.int64, device=dev), torch.empty(2 * b * 17, device=dev)
        for head in range(2):
            merged = torch.from_numpy(ref(own[head].cpu().numpy(), perm, sh)).to(dev)
            p, m = FL.get_final_preds(merged, meta['center'], meta['scale'])
            want_rows[head].append(np.concatenate([p.cpu().numpy(), m.cpu().numpy()], 2).astype(np.float64))
            lib().call('fami_pck_accuracy_f32', merged.data_ptr(), target.data_ptr(), rows[head].data_ptr(), iws.data_ptr(),
                       mws.data_ptr(), b, 17, H // 4, W // 4, 0.5, _stream(dev))
            r = rows[head].cpu().numpy()
            want_acc[head][0] += float(r[18]) * int(r[19])
            want_acc[head][1] += int(r[19])
    acc = ev.evaluate_loop(model, batches, 3, flip=True, shift_heatmap=sh)
    assert acc.idx == 3
    assert np.array_equal(acc.all_preds, np.concatenate(want_rows[0], 0))
    assert np.array_equal(acc.all_bb, np.concatenate(want_rows[1], 0))
    for head in range(2):
        assert acc.acc_cnt[head] == want_acc[head][1] > 0 and acc.acc_sum[head] == want_acc[head][0]
    plain = ev.evaluate_loop(model, batches, 3)
    assert not np.array_equal(plain.all_preds, acc.all_preds)                    # the option is no no-op
