"""The integral (soft-argmax) coordinate term without a GPU: the float64 restatement of tests/_integral_ref.py against torch
autograd, the conditions of the exact GPU cases on the reference alone, every refusal before device work, the config keys, and
what the decode can and cannot recover from a sub-pixel target map."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _integral_ref as ir  # noqa: E402

import fami_pose_amd as fp  # noqa: E402
from fami_pose_amd import evaluate as ev  # noqa: E402
from fami_pose_amd import loss as FL  # noqa: E402
from fami_pose_amd.train import Trainer  # noqa: E402


@pytest.mark.parametrize('shape', [(3, 16, 8), (2, 24, 18), (1, 1, 33)])
def test_restated_gradient_is_float64_autograd(shape):
    R, H, W = shape
    h = ir.general_maps(R, H, W, 7)
    txy, w = ir.general_targets(h, 20.0, 7)
    v, ga = ir.loss_autograd(h, 20.0, txy, w, 0.5)
    e_v = abs(ir.loss(h, 20.0, txy, w, 0.5).item() - v.item())
    e_g = (ir.grad(h, 20.0, txy, w, 0.5) - ga).abs().max().item()
    print('R %d %dx%d: loss differs by %.3g, gradient by %.3g' % (R, H, W, e_v, e_g))
    assert e_v <= 1e-12 and e_g <= 1e-12
    # ... and the soft-argmax alone, against autograd of a random linear form of the coordinates
    gc = torch.randn(R, 2, generator=torch.Generator().manual_seed(3)).double()
    a = ir.logits(h, 20.0).double().requires_grad_(True)
    p = torch.softmax(a, 1)
    x, y = ir.grids(H, W, ir.F64)
    (gc[:, 0] * (p * x).sum(1) + gc[:, 1] * (p * y).sum(1)).sum().backward()
    assert (ir.softargmax_grad(h, 20.0, gc) - (a.grad * 20.0).reshape(R, H, W)).abs().max().item() <= 1e-12


@pytest.mark.parametrize('case', ir.EX_CASES, ids=lambda c: 'K%d-R%d' % c)
def test_exact_cases_are_determined_on_the_reference(case):
    """exact_case asserts its own conditions; here additionally: the plain fp32 evaluation, which sums in another order and
    normalises before it sums, gives the same coordinates, loss rows and gradient -- the results do not depend on the order"""
    c = ir.exact_case(*case)
    px, py = ir.forward_plain32(c['h'], ir.EX_BETA)
    assert torch.equal(px.double(), c['cx']) and torch.equal(py.double(), c['cy'])
    assert torch.equal(ir.rows(px, py, c['txy'], c['w'], ir.EX_H, ir.EX_W).double(), c['rows'])
    assert torch.equal(ir.grad(c['h'], ir.EX_BETA, c['txy'], c['w'], c['gscale'], ir.F32).double(), c['grads'][0, 0])
    assert torch.equal(ir.grad(c['h'].flip(0), ir.EX_BETA, c['txy'].flip(0), c['w'].flip(0), c['gscale'], e32=True).flip(0), c['grads'][0, 0])


def test_flat_and_dominant_maps_on_the_reference():
    flat = torch.full((1, ir.EX_H, ir.EX_W), 0.375)
    cx, cy = ir.forward(flat, ir.EX_BETA)[:2]
    assert cx.item() == (ir.EX_W - 1) / 2 and cy.item() == (ir.EX_H - 1) / 2
    # a maximum that leads by more than 104 / beta: every other expf underflows to 0 in fp32 (the smallest subnormal is
    # exp(-103.28), half of it exp(-103.97))
    assert np.exp(np.float32(-104.0)) == 0.0 and np.exp(np.float32(-103.0)) > 0.0


@pytest.mark.parametrize('beta', [0.0, -1.0, float('inf'), float('nan'), 1e39, None, 'x', True])
def test_bad_beta_is_refused_before_device_work(beta):
    hm = torch.zeros(1, 1, 4, 4)          # a HOST tensor: reaching the device path would raise RuntimeError instead
    with pytest.raises(ValueError):
        FL.check_integral_options(1.0, beta)
    with pytest.raises(ValueError):
        FL.soft_argmax(hm, beta)
    with pytest.raises(ValueError):
        FL.IntegralL1Loss(beta=beta)
    with pytest.raises(ValueError):
        FL.integral_get_final_preds(hm, np.zeros((1, 2)), np.ones((1, 2)), beta)
    with pytest.raises(ValueError):
        ev._decoder('integral', 11, beta)
    with pytest.raises(ValueError):
        ev.predict(None, hm, hm, None, None, decode='integral', integral_beta=beta)
    with pytest.raises(ValueError):
        ev.evaluate_loop(None, [], 0, decode='integral', integral_beta=beta)


@pytest.mark.parametrize('weight', [0.0, -0.5, float('inf'), float('nan'), 'x', True])
def test_bad_weight_is_refused(weight):
    with pytest.raises(ValueError):
        FL.check_integral_options(weight, 20.0)


def test_good_options_and_the_other_decodes_ignore_beta():
    assert FL.check_integral_options(2, 20) == (2.0, 20.0)
    assert FL.check_integral_options(np.float32(0.5), np.float64(8)) == (0.5, 8.0)
    assert ev._decoder('standard', 11, -1.0) is FL.get_final_preds
    assert callable(ev._decoder('dark', 11, float('nan'))) and callable(ev._decoder('integral', 4, 20.0))
    with pytest.raises(ValueError, match='integral'):
        ev._decoder('argmax', 11)
    with pytest.raises(ValueError):
        ev.predict(None, None, None, None, None, decode='soft')


class _NoDevice(torch.nn.Module):
    """a model whose parameters live on the host: a Trainer that got past its argument checks raises RuntimeError"""
    num_joints = 17

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))


def test_trainer_refuses_before_device_work():
    with pytest.raises(ValueError, match='targets_from_joints'):
        Trainer(_NoDevice(), integral_l1_weight=1.0, targets_from_joints=False)
    for kw in (dict(integral_l1_weight=-1.0), dict(integral_l1_weight=0.0), dict(integral_l1_weight=1.0, integral_beta=0.0),
               dict(integral_l1_weight=1.0, integral_beta=float('nan'))):
        with pytest.raises(ValueError):
            Trainer(_NoDevice(), targets_from_joints=True, **kw)
    with pytest.raises(RuntimeError, match='GPU'):          # good options reach the device check
        Trainer(_NoDevice(), integral_l1_weight=0.5, targets_from_joints=True)
    with pytest.raises(RuntimeError, match='GPU'):          # ... and without the term beta is not looked at
        Trainer(_NoDevice(), integral_beta=-3.0)


def test_from_cfg_maps_the_two_keys(monkeypatch):
    cfg = fp.default_cfg(48)
    assert cfg['LOSS']['INTEGRAL_L1'] == {'USE': False, 'WEIGHT': 1.0}
    seen = []
    monkeypatch.setattr(Trainer, '__init__', lambda self, model, **kw: seen.append(kw))
    Trainer.from_cfg(cfg, None)
    assert 'integral_l1_weight' not in seen[-1]
    cfg['LOSS']['INTEGRAL_L1'] = {'USE': True, 'WEIGHT': 0.25}
    Trainer.from_cfg(cfg, None)
    assert seen[-1]['integral_l1_weight'] == 0.25
    Trainer.from_cfg(cfg, None, integral_l1_weight=None, integral_beta=8.0)          # keyword arguments win
    assert seen[-1]['integral_l1_weight'] is None and seen[-1]['integral_beta'] == 8.0
    cfg['LOSS']['INTEGRAL_L1'] = {'USE': True}
    Trainer.from_cfg(cfg, None)
    assert seen[-1]['integral_l1_weight'] == 1.0
    del cfg['LOSS']['INTEGRAL_L1']          # a configuration from before the key
    Trainer.from_cfg(cfg, None)
    assert 'integral_l1_weight' not in seen[-1]


def test_subpixel_target_decodes_back_to_its_joint():
    """A property of the definition, on the reference alone.  A sigma-3 sub-pixel target map on 96 x 72 (the window of +-9 px
    around the rounded centre) whose centre lies at least 12 px from every border decodes at beta = 20 to its joint within
    2e-3 px: the worst error over these 200 seeded draws is 1.45e-3 px, what the window's cut at +-9 px (asymmetric about a
    centre that is not an integer) leaves.  NEAR A BORDER THIS DOES NOT HOLD: the map cuts the Gaussian's tail on one side and the
    expectation is pulled inward, by up to 0.29 px for a joint within 2 px of it -- the integral decode is biased there,
    where the DARK decode is not."""
    H, W = 96, 72
    g = torch.Generator().manual_seed(20181)
    c = 12.0 + torch.rand(200, 2, generator=g).double() * torch.tensor([W - 1 - 24.0, H - 1 - 24.0], dtype=torch.float64)
    maps = torch.from_numpy(np.stack([ir.subpixel_map(H, W, x.item(), y.item()) for x, y in c]))
    cx, cy = ir.forward(maps, 20.0)[:2]
    worst = max((cx - c[:, 0]).abs().max().item(), (cy - c[:, 1]).abs().max().item())
    print('worst decode error over 200 interior joints: %.3g px' % worst)
    assert worst <= 2e-3
    edge = torch.from_numpy(np.stack([ir.subpixel_map(H, W, 30.3, y) for y in (0.0, 0.4, 1.0, 2.0)]))
    bias = (ir.forward(edge, 20.0)[1] - torch.tensor([0.0, 0.4, 1.0, 2.0], dtype=torch.float64)).abs().max().item()
    print('worst bias for a joint within 2 px of the border: %.3g px' % bias)
    assert 0.1 < bias < 0.3
