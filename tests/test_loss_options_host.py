"""The supervision options without a GPU: the restatements of tests/_target_ref.py against the reference-generated
fixture tests/golden/g16_joint_weights.npz (tools/gen_target_golden.py), against oracle.ops and against a torch.topk
transcription of the HRNet OHKM loss; the argument checks that must raise before any device work; Trainer.from_cfg; and
the DARK round trip that says why the sub-pixel encoding exists.

Round-trip bounds (k = 11, sigma 3, 68 maps of 96x72 and 68 of 64x48, centres at least 10 px from every border, float64
and its fp32 emulation): a map encoded at the real-valued centre decodes to within 1.7e-4 heatmap px of it -- asserted
at 1e-3, the sixfold margin covers another expf -- while the quantised map of the same joints is off by up to 0.498 px,
asserted to exceed 0.4: the second assertion shows that the first one bites."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _dark_ref as dr  # noqa: E402
import _target_ref as tr  # noqa: E402

import fami_pose_amd as fp  # noqa: E402
from fami_pose_amd import loss as FL  # noqa: E402
from fami_pose_amd.data import FLIP_PAIRS, JOINTS_WEIGHT  # noqa: E402
from oracle import ops as oops  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g16_joint_weights.npz')


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


def test_joints_weight_is_the_posetrack_vector(gold):
    assert isinstance(JOINTS_WEIGHT, tuple) and len(JOINTS_WEIGHT) == 17
    assert np.array_equal(np.array(JOINTS_WEIGHT, np.float32), gold['joints_weight'])
    for a, b in FLIP_PAIRS:                          # a left / right pair carries one weight
        assert JOINTS_WEIGHT[a] == JOINTS_WEIGHT[b]
    assert sorted(set(JOINTS_WEIGHT)) == [1.0, 1.2, 1.5]


def test_restatement_with_weights_equals_the_reference_fixture(gold):
    for sfx in ('', '_big'):
        t, w = tr.gauss_targets(gold['joints' + sfx], gold['joints_vis' + sfx][..., 0], int(gold['sigma']),
                                gold['image_size' + sfx], gold['heatmap_size' + sfx], joint_weights=JOINTS_WEIGHT)
        assert t.dtype == np.float32 and t.shape == gold['target' + sfx].shape
        assert np.array_equal(_bits(t), _bits(gold['target' + sfx]))
        assert np.array_equal(_bits(w), _bits(gold['weight' + sfx]))
    w = gold['weight'][..., 0]
    names = list(gold['names'])
    assert (w[names.index('borders')] == 0).sum() == 5 and (w[names.index('vis0')][[0, 7, 9]] == 0).all()


def test_restatement_without_weights_equals_oracle_ops(gold):
    for sfx in ('', '_big'):
        joints, vis = gold['joints' + sfx], gold['joints_vis' + sfx]
        t, w = tr.gauss_targets(joints, vis[..., 0], 3, gold['image_size' + sfx], gold['heatmap_size' + sfx])
        for n in range(joints.shape[0]):
            t0, w0 = oops.generate_heatmaps(joints[n], vis[n], 3, gold['image_size' + sfx], gold['heatmap_size' + sfx], 17)
            assert np.array_equal(_bits(t[n]), _bits(t0)) and np.array_equal(_bits(w[n]), _bits(w0))
        # the multiplied weights are these times the vector; the maps do not change (the > 0.5 test is on the unmultiplied weight)
        assert np.array_equal(_bits(t), _bits(gold['target' + sfx]))
        assert np.array_equal(_bits(w * np.array(JOINTS_WEIGHT, np.float32).reshape(1, 17, 1)), _bits(gold['weight' + sfx]))


def test_subpixel_restatement_shares_window_and_weights_and_integer_joints(gold):
    joints, vis = gold['joints'], gold['joints_vis'][..., 0]
    q, wq = tr.gauss_targets(joints, vis, 3, gold['image_size'], gold['heatmap_size'])
    s, ws = tr.gauss_targets(joints, vis, 3, gold['image_size'], gold['heatmap_size'], encoding='subpixel')
    assert np.array_equal(wq, ws)
    assert np.array_equal(q > 0, s > 0)                       # one window; exp never underflows inside it
    k = list(gold['names']).index('centre')                   # integer positions: equal to fp32 rounding
    assert np.abs(s[k] - q[k]).max() < 1e-7
    k = list(gold['names']).index('half')                     # two equal maxima, the first is the lower pixel
    cx = joints[k, :, 0].astype(np.float64) / 4
    assert (cx % 1 == 0.5).all()
    am_s = s[k].reshape(17, -1).argmax(1) % 18
    am_q = q[k].reshape(17, -1).argmax(1) % 18
    assert np.array_equal(am_s, np.floor(cx)) and np.array_equal(am_q, np.floor(cx) + 1)


CASES = [(1, 17, 8), (5, 17, 8), (2, 15, 8), (3, 5, 5), (2, 17, 1), (2, 70, 8)]


@pytest.mark.parametrize('B,J,k', CASES)
@pytest.mark.parametrize('use_w', [True, False], ids=['w', 'now'])
def test_ohkm_restatement_equals_the_topk_transcription(B, J, k, use_w):
    gen = torch.Generator().manual_seed(100 * B + J + k)
    pred = torch.randn(B, J, 6, 5, generator=gen, dtype=torch.float64).requires_grad_(True)
    gt = torch.rand(B, J, 6, 5, generator=gen, dtype=torch.float64)
    w = (torch.rand(B, J, 1, generator=gen, dtype=torch.float64) < 0.8).double() * 1.5
    want = tr.hrnet_ohkm_torch(pred, gt, w, k, use_target_weight=use_w)
    want.backward()
    value, sel, grad = tr.ohkm_ref(pred.detach().numpy(), gt.numpy(), w.numpy() if use_w else None, k)
    assert value == pytest.approx(want.item(), rel=1e-12)
    assert np.abs(grad - pred.grad.numpy()).max() <= 1e-12 * np.abs(grad).max()
    assert (sel.sum(1) == k).all()


def test_ohkm_order_ties_and_nan():
    assert tr.ohkm_order([1.0, 3.0, 3.0, 0.0, 0.0]) == [1, 2, 0, 3, 4]
    assert tr.ohkm_order([1.0, float('nan'), 5.0, float('nan')]) == [1, 3, 2, 0]
    sel = tr.ohkm_select(np.array([[2.0, 0.0, 0.0, 0.0], [1.0, 1.0, 1.0, 1.0]]), 2)
    assert sel.tolist() == [[True, True, False, False], [True, True, False, False]]
    # topk = J is JointMSELoss: (1/J) sum_j mean_{b,p}
    rng = np.random.RandomState(0)
    p, g, w = rng.randn(3, 5, 4, 3), rng.rand(3, 5, 4, 3), rng.rand(3, 5)
    v, sel, _ = tr.ohkm_ref(p, g, w, 5)
    assert sel.all() and v == pytest.approx(((w[:, :, None, None] * (p - g)) ** 2).mean(), rel=1e-12)


def _no_device(monkeypatch):
    """any library call or device test from here on fails the test"""
    def boom(*a, **k):
        raise AssertionError('device work before the argument check')
    monkeypatch.setattr(FL, 'lib', boom)
    monkeypatch.setattr(FL, '_need_cuda', boom)


def test_generate_heatmaps_argument_checks_come_before_device_work(monkeypatch):
    _no_device(monkeypatch)
    joints, vis = torch.zeros(2, 17, 2), torch.ones(2, 17)
    for kw in (dict(encoding='dark'), dict(encoding=None), dict(encoding='Subpixel'), dict(joint_weights=[1.0] * 16),
               dict(joint_weights=torch.ones(18)), dict(joint_weights=()), dict(encoding='subpixel', joint_weights=(1.0,))):
        with pytest.raises(ValueError):
            FL.generate_heatmaps(joints, vis, 3, (72, 96), (18, 24), **kw)
    with pytest.raises(AssertionError):               # valid arguments do reach the device test
        FL.generate_heatmaps(joints, vis, 3, (72, 96), (18, 24), encoding='subpixel', joint_weights=JOINTS_WEIGHT)


def test_ohkm_loss_argument_checks(monkeypatch):
    _no_device(monkeypatch)
    for bad in (0, -1, True, False, 2.0, None, '8'):
        with pytest.raises(ValueError):
            FL.JointOHKMMSELoss(topk=bad)
    m = FL.JointOHKMMSELoss()
    assert m.topk == 8 and m.use_target_weight
    assert '0.5' in FL.JointOHKMMSELoss.__doc__ and 'mse_weight' in FL.JointOHKMMSELoss.__doc__
    with pytest.raises(AssertionError):
        m(torch.zeros(2, 17, 4, 3), torch.zeros(2, 17, 4, 3), torch.ones(2, 17, 1))


@pytest.fixture(scope='module')
def model():
    return fp.build_model(fp.default_cfg(48, image_size=(96, 128), num_sup=2), 'train')


def test_trainer_argument_checks_come_before_the_device(model):
    """the model is on the CPU: a Trainer that got past its argument checks raises RuntimeError (HIP path only)"""
    from fami_pose_amd.train import Trainer
    for bad in (dict(ohkm_topk=0), dict(ohkm_topk=18), dict(ohkm_topk=True), dict(ohkm_topk=8.0),
                dict(target_encoding='subpixel'), dict(joint_weights=JOINTS_WEIGHT),
                dict(target_encoding='subpixel', targets_from_joints=False),
                dict(target_encoding='dark', targets_from_joints=True),
                dict(joint_weights=JOINTS_WEIGHT[:16], targets_from_joints=True)):
        with pytest.raises(ValueError):
            Trainer(model, **bad)
    for good in (dict(), dict(ohkm_topk=8), dict(ohkm_topk=17), dict(ohkm_topk=1),
                 dict(target_encoding='subpixel', joint_weights=JOINTS_WEIGHT, ohkm_topk=8, targets_from_joints=True)):
        with pytest.raises(RuntimeError, match='HIP path only'):
            Trainer(model, **good)


def test_from_cfg_follows_the_cfg_key(model, monkeypatch):
    from fami_pose_amd.train import Trainer
    seen = []
    monkeypatch.setattr(Trainer, '__init__', lambda self, model, **kw: seen.append(kw))
    cfg = fp.default_cfg(48, image_size=(96, 128), num_sup=2)
    assert 'USE_DIFFERENT_JOINTS_WEIGHT' not in cfg['LOSS']
    Trainer.from_cfg(cfg, model, targets_from_joints=True)
    assert 'joint_weights' not in seen[-1]
    cfg['LOSS']['USE_DIFFERENT_JOINTS_WEIGHT'] = False
    Trainer.from_cfg(cfg, model, targets_from_joints=True)
    assert 'joint_weights' not in seen[-1]
    cfg['LOSS']['USE_DIFFERENT_JOINTS_WEIGHT'] = True
    Trainer.from_cfg(cfg, model, targets_from_joints=True)
    assert seen[-1]['joint_weights'] == JOINTS_WEIGHT and seen[-1]['targets_from_joints'] is True
    Trainer.from_cfg(cfg, model, targets_from_joints=True, joint_weights=(2.0,) * 17)      # the keyword wins
    assert seen[-1]['joint_weights'] == (2.0,) * 17
    assert 'target_encoding' not in seen[-1] and 'ohkm_topk' not in seen[-1]                # no key in the reference
    cfg['MODEL']['NUM_JOINTS'] = 15
    with pytest.raises(ValueError, match='joint_weights='):
        Trainer.from_cfg(cfg, model, targets_from_joints=True)
    Trainer.from_cfg(cfg, model, targets_from_joints=True, joint_weights=(1.0,) * 15)
    assert seen[-1]['joint_weights'] == (1.0,) * 15


@pytest.mark.parametrize('H,W', [(96, 72), (64, 48)])
def test_dark_round_trip_of_the_restatement(H, W):
    B, J = 4, 17
    joints, c = tr.dark_round_trip_joints(1000 + H, B, J, H, W)
    vis = np.ones((B, J), np.float32)
    center = np.tile(np.array([[W / 2, H / 2]], np.float32), (B, 1))
    scale = np.tile(np.array([[W / 200, H / 200]], np.float32), (B, 1))
    assert np.float32(np.float32(W / 200) * np.float32(200)) / np.float32(W) == 1      # the transform is the identity
    worst = {}
    for enc in ('subpixel', 'quantised'):
        hm, _ = tr.gauss_targets(joints, vis, 3, (4 * W, 4 * H), (W, H), encoding=enc)
        for f32 in (False, True):
            got = dr.dark_ref(hm.astype(np.float32), center, scale, 11, fp32=f32)
            assert got['moved'].all()
            worst[enc, f32] = np.abs(got['coords'].astype(np.float64) - c).max()
    print('DARK round trip %dx%d: worst |decoded - joint| in heatmap px %s' % (H, W, worst))
    assert worst['subpixel', False] < 1e-3 and worst['subpixel', True] < 1e-3
    assert worst['quantised', False] > 0.4 and worst['quantised', True] > 0.4
