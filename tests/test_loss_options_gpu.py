"""The two new loss entry points on the MI355X: fami_gauss_target_ex_f32 (per-joint weights, sub-pixel encoding) and
fami_ohkm_fwd_f32 (online hard keypoint mining), with loss.generate_heatmaps / loss.JointOHKMMSELoss on top, against
tests/_target_ref.py and the reference-generated fixture tests/golden/g16_joint_weights.npz.

Bounds.  Target maps: 1e-6 absolute against the fixture and against the float64 restatement, the tolerance
test_losses_targets_decode uses for this kernel (values in [0, 1], one expf); weights, windows and everything the two
encodings share: bit equality.  OHKM kernel: integer operands (pred, gt in [-4, 4], w in {0, 1}, L <= 24 * 18: a row
sum is at most 64 * 432 = 27648 and every partial sum an exact fp32 integer), so selection and selected weights are
exact and the loss is the float64 value rounded once.  The module on random floats: 1e-6 relative (fp32 row sums of
L = 432 terms against float64)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _target_ref as tr  # noqa: E402

from fami_pose_amd import loss as FL  # noqa: E402
from fami_pose_amd._lib import lib  # noqa: E402
from fami_pose_amd.data import JOINTS_WEIGHT  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g16_joint_weights.npz')
SENT = 0x5a5a5a5a
PAD = 64
SHAPES = [(2, 17, 24, 18), (1, 3, 96, 72), (1, 5, 17, 13)]


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _guarded(n, dev):
    """-> (whole buffer of sentinel words, the float view of its middle n elements)"""
    buf = torch.full((n + 2 * PAD,), SENT, dtype=torch.int32, device=dev)
    return buf, buf[PAD:PAD + n].view(torch.float32)


def _intact(buf, n):
    return bool((buf[:PAD] == SENT).all()) and bool((buf[PAD + n:] == SENT).all())


def _joints(shape, seed, dev, integer=False):
    """joints from two strides outside the map to two strides outside (stride 4), ~80 % visible; integer: on whole,
    non-negative heatmap positions"""
    B, J, H, W = shape
    rng = np.random.RandomState(seed)
    if integer:
        c = np.stack([rng.randint(0, W + 2, (B, J)), rng.randint(0, H + 2, (B, J))], -1).astype(np.float64)
    else:
        c = np.stack([rng.uniform(-2, W + 2, (B, J)), rng.uniform(-2, H + 2, (B, J))], -1)
    vis = (rng.uniform(size=(B, J)) < 0.8).astype(np.float32)
    return torch.from_numpy((c * 4).astype(np.float32)).to(dev), torch.from_numpy(vis).to(dev)


def _target_ex(joints, vis, jw, shape, sub, dev):
    B, J, H, W = shape
    tb, t = _guarded(B * J * H * W, dev)
    wb, w = _guarded(B * J, dev)
    lib().call('fami_gauss_target_ex_f32', joints.data_ptr(), vis.data_ptr(), None if jw is None else jw.data_ptr(),
               t.data_ptr(), w.data_ptr(), B, J, H, W, 4 * H, 4 * W, 3, int(sub), _stream(dev))
    torch.cuda.synchronize(dev)
    assert _intact(tb, B * J * H * W) and _intact(wb, B * J)
    return t.reshape(shape).clone(), w.reshape(B, J).clone()


@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_target_ex_defaults_write_the_old_entry_points_bits(dev, shape):
    B, J, H, W = shape
    joints, vis = _joints(shape, 1, dev)
    t0, w0 = FL.generate_heatmaps(joints, vis, 3, (4 * W, 4 * H), (W, H))
    t1, w1 = _target_ex(joints, vis, None, shape, False, dev)
    assert torch.equal(t0, t1) and torch.equal(w0.reshape(B, J), w1)
    if J >= 17:
        assert t0.max() > 0.9 and (w0 == 0).any() and (w0 == 1).any()


@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_integer_positions_are_bit_equal_under_both_encodings(dev, shape):
    joints, vis = _joints(shape, 2, dev, integer=True)
    tq, wq = _target_ex(joints, vis, None, shape, False, dev)
    ts, ws = _target_ex(joints, vis, None, shape, True, dev)
    assert torch.equal(tq, ts) and torch.equal(wq, ws)
    assert (tq == 1).sum() >= 1


def test_joint_weights_against_the_reference_fixture(dev):
    g = np.load(GOLD)
    for sfx in ('', '_big'):
        joints = torch.from_numpy(g['joints' + sfx]).to(dev)
        vis = torch.from_numpy(g['joints_vis' + sfx]).to(dev)
        img, hm = g['image_size' + sfx], g['heatmap_size' + sfx]
        t, w = FL.generate_heatmaps(joints, vis, int(g['sigma']), img, hm, joint_weights=JOINTS_WEIGHT)
        err = np.abs(t.cpu().numpy() - g['target' + sfx]).max()
        print('g16%s: max |target - reference| %.3g' % (sfx, err))
        assert err <= 1e-6
        assert np.array_equal(w.cpu().numpy().view(np.int32), g['weight' + sfx].view(np.int32))
        t0, w0 = FL.generate_heatmaps(joints, vis, int(g['sigma']), img, hm)          # the maps do not depend on the vector
        assert torch.equal(t, t0)
        t2, w2 = FL.generate_heatmaps(joints, vis, int(g['sigma']), img, hm,
                                      joint_weights=torch.tensor(JOINTS_WEIGHT, dtype=torch.float64))
        assert torch.equal(w2, w) and torch.equal(t2, t)


@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_subpixel_maps_against_the_float64_restatement(dev, shape):
    B, J, H, W = shape
    joints, vis = _joints(shape, 3, dev)
    jw = torch.from_numpy(np.random.RandomState(4).uniform(0.5, 2.0, J).astype(np.float32)).to(dev)
    ts, ws = _target_ex(joints, vis, jw, shape, True, dev)
    tq, wq = _target_ex(joints, vis, jw, shape, False, dev)
    want, wwant = tr.gauss_targets(joints.cpu().numpy(), vis.cpu().numpy(), 3, (4 * W, 4 * H), (W, H), encoding='subpixel',
                                   joint_weights=jw.cpu().numpy())
    err = np.abs(ts.cpu().numpy().astype(np.float64) - want).max()
    print('%s: max |subpixel - float64| %.3g' % (shape, err))
    assert err <= 1e-6
    assert torch.equal(ws, wq)                                            # the weights are the quantised call's
    assert np.array_equal(ws.cpu().numpy().view(np.int32), wwant.reshape(B, J).view(np.int32))
    assert torch.equal(ts > 0, tq > 0) and not torch.equal(ts, tq)        # one window, other values


@pytest.mark.parametrize('H,W', [(96, 72), (64, 48)])
def test_dark_round_trip_on_the_device(dev, H, W):
    """generate_heatmaps(encoding='subpixel') -> dark_get_final_preds returns the joint to within 1e-3 heatmap px (1.7e-4
    measured on the restatement); the quantised targets of the same joints are off by more than 0.4 px (0.498)."""
    B, J = 4, 17
    joints, c = tr.dark_round_trip_joints(1000 + H, B, J, H, W)
    jt = torch.from_numpy(joints).to(dev)
    vis = torch.ones(B, J, device=dev)
    center = np.tile(np.array([[W / 2, H / 2]], np.float32), (B, 1))
    scale = np.tile(np.array([[W / 200, H / 200]], np.float32), (B, 1))
    assert np.float32(np.float32(W / 200) * np.float32(200)) / np.float32(W) == 1
    worst = {}
    for enc in ('subpixel', 'quantised'):
        hm, _ = FL.generate_heatmaps(jt, vis, 3, (4 * W, 4 * H), (W, H), encoding=enc)
        preds, _ = FL.dark_get_final_preds(hm, center, scale, blur_kernel=11)
        worst[enc] = np.abs(preds.cpu().numpy().astype(np.float64) - c).max()
    print('DARK round trip on the device %dx%d: %s' % (H, W, worst))
    assert worst['subpixel'] < 1e-3
    assert worst['quantised'] > 0.4


# ---------------------------------------------------------------------------------------------- OHKM

OHKM_CASES = [(1, 17, 8), (5, 17, 8), (2, 15, 8), (3, 5, 5), (2, 17, 1), (2, 70, 8)]
L_OHKM = 24 * 18


def _int_operands(B, J, k, seed):
    """integer pred / gt in [-4, 4], w in {0, 1} (~80 % ones), with the planted samples: the last sample of B >= 2 is all
    zero; of B >= 3, b = 0 has two non-zero rows (fewer than k for k >= 3) and b = 1 ties exactly at the k-th place; the
    others are as drawn"""
    rng = np.random.RandomState(seed)
    pred = rng.randint(-4, 5, (B, J, L_OHKM)).astype(np.float32)
    gt = rng.randint(-4, 5, (B, J, L_OHKM)).astype(np.float32)
    w = (rng.uniform(size=(B, J)) < 0.8).astype(np.float32)
    if B >= 3:
        w[0] = 0
        w[0, [J - 1, J // 2]] = 1                     # two non-zero rows: the zeros are taken by lowest index
    if B >= 2:
        pred[B - 1] = gt[B - 1]                       # an all-zero sample
    if B >= 3:
        w[1] = 1
        order = tr.ohkm_order(((pred[1] - gt[1]) ** 2).sum(1))
        a, b = order[k - 1], order[k] if k < J else order[k - 2]
        pred[1, b], gt[1, b] = pred[1, a], gt[1, a]   # row b repeats the k-th row
    return pred, gt, w


def want_few(row, k, J):
    """the sample with two non-zero rows: those two and the k - 2 zero rows of lowest index are selected"""
    sel = tr.ohkm_select(row[None], k)[0]
    zeros = [j for j in range(J) if row[j] == 0][:k - 2]
    return sorted(np.flatnonzero(sel)) == sorted(zeros + [J // 2, J - 1])


def _ohkm(pred, gt, w, k, scale, dev):
    B, J, L = pred.shape
    p, g = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
    wd = None if w is None else torch.from_numpy(w).to(dev)
    sb, sel = _guarded(B * J, dev)
    lb, loss = _guarded(1, dev)
    wsb, ws = _guarded(B * J, dev)
    rc = lib().cdll.fami_ohkm_fwd_f32(p.data_ptr(), g.data_ptr(), None if wd is None else wd.data_ptr(), loss.data_ptr(),
                                      sel.data_ptr(), B, J, L, k, float(scale), ws.data_ptr(), _stream(dev))
    torch.cuda.synchronize(dev)
    assert _intact(sb, B * J) and _intact(lb, 1) and _intact(wsb, B * J)
    return rc, sel.reshape(B, J).cpu().numpy().copy(), loss.cpu().numpy().copy(), (sb, lb, wsb)


@pytest.mark.parametrize('B,J,k', OHKM_CASES)
def test_ohkm_kernel_is_exact_on_integer_operands(dev, B, J, k):
    pred, gt, w = _int_operands(B, J, k, 7 * B + J + k)
    rows = ((w[:, :, None].astype(np.float64) * (pred.astype(np.float64) - gt)) ** 2).sum(2)
    assert rows.max() <= 64 * L_OHKM < 2 ** 24
    if B >= 3:
        assert (rows[0] > 0).sum() == 2 < k and want_few(rows[0], k, J)
    if B >= 2:
        assert (rows[B - 1] == 0).all()
    if B >= 3:
        o = tr.ohkm_order(rows[1])
        kk = k if k < J else k - 1
        assert rows[1][o[kk - 1]] == rows[1][o[kk]] > 0                # an exact tie at the k-th place
    want_sel = tr.ohkm_select(rows, k)
    scale = 1.0 / (B * L_OHKM * k)
    rc, sel_w, loss, _ = _ohkm(pred, gt, w, k, scale, dev)
    assert rc == 0
    assert np.array_equal(sel_w, np.where(want_sel, w, 0).astype(np.float32))
    want = np.float32(np.float64(rows[want_sel].sum()) * scale)
    assert loss.view(np.int32)[0] == want.view(np.int32), (loss, want)
    rc2, sel_w2, loss2, _ = _ohkm(pred, gt, w, k, scale, dev)                   # run to run
    assert rc2 == 0 and np.array_equal(sel_w2.view(np.int32), sel_w.view(np.int32)) and loss2.view(np.int32)[0] == loss.view(np.int32)[0]
    # without weights the selected weights are ones
    rows1 = ((pred.astype(np.float64) - gt) ** 2).sum(2)
    rc, sel1, loss1, _ = _ohkm(pred, gt, None, k, scale, dev)
    assert rc == 0 and np.array_equal(sel1, tr.ohkm_select(rows1, k).astype(np.float32))
    assert loss1.view(np.int32)[0] == np.float32(np.float64(rows1[sel1 > 0].sum()) * scale).view(np.int32)


@pytest.mark.parametrize('B,J', [(5, 17), (2, 70), (3, 5)])
def test_ohkm_with_every_joint_is_the_plain_loss(dev, B, J):
    pred, gt, w = _int_operands(B, J, J, 11)
    scale = 1.0 / (B * L_OHKM * J)
    rc, sel_w, loss, _ = _ohkm(pred, gt, w, J, scale, dev)
    assert rc == 0 and np.array_equal(sel_w, w)
    p, g, wd = (torch.from_numpy(a).to(dev) for a in (pred, gt, w))
    out, ws = torch.zeros(1, device=dev), torch.zeros(B * J, device=dev)
    lib().call('fami_wmse_fwd_f32', p.data_ptr(), g.data_ptr(), wd.data_ptr(), out.data_ptr(), B * J, L_OHKM, scale,
               ws.data_ptr(), _stream(dev))
    assert out.cpu().numpy().view(np.int32)[0] == loss.view(np.int32)[0]


def test_ohkm_nan_row_is_selected_first(dev):
    B, J, k = 2, 17, 3
    pred, gt, w = _int_operands(B, J, 1, 5)
    w[:] = 1
    pred[0, 11, 7] = np.nan
    rc, sel_w, loss, _ = _ohkm(pred, gt, w, k, 1.0, dev)
    assert rc == 0 and sel_w[0, 11] == 1 and sel_w[0].sum() == k and sel_w[1].sum() == k
    assert np.isnan(loss[0])
    rows = ((pred.astype(np.float64) - gt) ** 2).sum(2)
    assert np.array_equal(sel_w > 0, tr.ohkm_select(rows, k))


@pytest.mark.parametrize('k', [0, 18, -1])
def test_ohkm_bad_k_returns_minus_one_and_writes_nothing(dev, k):
    pred, gt, w = _int_operands(2, 17, 8, 3)
    rc, _, _, (sb, lb, wsb) = _ohkm(pred, gt, w, k, 1.0, dev)
    assert rc == -1
    for buf in (sb, lb, wsb):
        assert bool((buf == SENT).all())
    assert b'fami_ohkm_fwd_f32' in lib().cdll.fami_last_error()


@pytest.mark.parametrize('B,J,k', [(2, 17, 8), (3, 5, 5), (2, 70, 8)])
@pytest.mark.parametrize('use_w', [True, False], ids=['w', 'now'])
def test_ohkm_module_forward_and_backward_against_torch(dev, B, J, k, use_w):
    gen = torch.Generator().manual_seed(B + J + k)
    pred = torch.randn(B, J, 24, 18, generator=gen)
    gt = torch.rand(B, J, 24, 18, generator=gen)
    w = (torch.rand(B, J, 1, generator=gen) < 0.8).float() * 1.5
    p64 = pred.double().requires_grad_(True)
    want = tr.hrnet_ohkm_torch(p64, gt.double(), w.double(), k, use_target_weight=use_w)
    want.backward()
    pd = pred.to(dev).requires_grad_(True)
    got = FL.JointOHKMMSELoss(topk=k, use_target_weight=use_w)(pd, gt.to(dev), w.to(dev))
    (3.0 * got).backward()
    e_v = abs(got.item() - want.item()) / abs(want.item())
    e_g = ((pd.grad.cpu().double() / 3.0 - p64.grad).abs().max() / p64.grad.abs().max()).item()
    print('OHKM module (%d, %d, %d): value relerr %.3g, gradient relerr %.3g' % (B, J, k, e_v, e_g))
    assert e_v <= 1e-6 and e_g <= 1e-6
    if k == J:
        plain = FL.JointMSELoss(use_target_weight=use_w)(pred.to(dev), gt.to(dev), w.to(dev))
        assert plain.item() == got.item()
