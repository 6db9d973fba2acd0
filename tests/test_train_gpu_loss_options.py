"""Trainer(target_encoding=, joint_weights=, ohkm_topk=): the options of the supervision on the MI355X, eager launches and
hipGraph replay.  Each option is checked against a PLAIN Trainer (targets_from_joints=False) that is fed what the option
must have produced -- targets and weights from loss.generate_heatmaps, the OHKM selection folded into the weights -- so
that the only thing under test is the three launches between the forward and the backward pass.

Sizes and helpers are those of tests/test_train_gpu_clip.py (W48, S = 2, 128x96, B = 2).  Every Trainer here runs
model.set_deterministic(True): gradients are then equal bit for bit from Trainer to Trainer, which is what the bitwise
assertions rest on; the 1e-6 relative bounds are for two scales that are equal in exact arithmetic and rounded
differently (mse_weight * 17 / 8 / (B L 17) against mse_weight / (B L 8)) and for fp32 against float64 row sums."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _target_ref as tref  # noqa: E402

from fami_pose_amd import loss as FL  # noqa: E402
from fami_pose_amd.data import JOINTS_WEIGHT  # noqa: E402
from test_train_gpu_clip import H, W, _batch, _relerr, _trainer  # noqa: E402

pytestmark = pytest.mark.gpu
NEW = ('fami_gauss_target_ex_f32', 'fami_ohkm_fwd_f32')
GRAPH = pytest.mark.parametrize('use_graph', [False, True], ids=['eager', 'graph'])
HM = (W // 4, H // 4)

_default = {}


def _default_step(dev, use_graph):
    """one step of the default Trainer on _batch(dev): gradient arena, loss parts and PCK rows (computed once per mode)"""
    if use_graph not in _default:
        tr = _trainer(dev, use_graph, deterministic=True)
        tr.step(*_batch(dev))
        torch.cuda.synchronize(dev)
        _default[use_graph] = (tr.grad.detach().clone(), tr.loss_parts.clone(), tr.acc.clone())
    return _default[use_graph]


def _plain(dev, use_graph, **kw):
    from fami_pose_amd.train import Trainer
    from test_train_gpu_clip import _model
    model = _model().to(dev)
    model.set_deterministic(True)
    return Trainer(model, use_graph=use_graph, targets_from_joints=False, **kw)


def test_default_trainer_calls_none_of_the_new_entry_points(dev, monkeypatch):
    from fami_pose_amd._lib import lib
    tr = _trainer(dev, False)
    assert tr.ohkm_topk is None and not tr.subpixel and tr.joint_weights is None and tr.ohkm_selection() is None
    names = []
    L = lib()
    call, call_routed = L.call, L.call_routed
    monkeypatch.setattr(L, 'call', lambda name, *a: (names.append(name), call(name, *a))[1])
    monkeypatch.setattr(L, 'call_routed', lambda route, name, *a: (names.append(name), call_routed(route, name, *a))[1])
    tr.step(*_batch(dev))
    torch.cuda.synchronize(dev)
    assert not set(names) & set(NEW)
    assert [n for n in names if n in ('fami_gauss_target_f32', 'fami_wmse_fwd_f32', 'fami_wmse_bwd_f32')] == \
        ['fami_gauss_target_f32', 'fami_wmse_fwd_f32', 'fami_wmse_bwd_f32']
    # ... and a Trainer with every option calls both, in the same three places
    names.clear()
    tr = _trainer(dev, False, target_encoding='subpixel', joint_weights=JOINTS_WEIGHT, ohkm_topk=8)
    tr.step(*_batch(dev))
    torch.cuda.synchronize(dev)
    assert [n for n in names if n in NEW + ('fami_gauss_target_f32', 'fami_wmse_fwd_f32', 'fami_wmse_bwd_f32')] == \
        ['fami_gauss_target_ex_f32', 'fami_ohkm_fwd_f32', 'fami_wmse_bwd_f32']


@GRAPH
def test_ohkm_with_every_joint_is_the_default_step(dev, use_graph):
    grad, parts, acc = _default_step(dev, use_graph)
    tr = _trainer(dev, use_graph, deterministic=True, ohkm_topk=17)
    tr.step(*_batch(dev))
    assert torch.equal(tr.grad, grad)
    e = abs(tr.loss_parts[0].item() - parts[0].item()) / abs(parts[0].item())
    print('ohkm_topk=17: loss relerr %.3g' % e)
    assert e <= 1e-6
    assert torch.equal(tr.loss_parts[1:], parts[1:]) and torch.equal(tr.acc, acc)
    bt = _batch(dev)
    assert torch.equal(tr.ohkm_selection(), FL.generate_heatmaps(bt[2], bt[3], 3, (W, H), HM)[1].reshape(2, 17) != 0)


@GRAPH
def test_ohkm_topk_8_is_a_plain_step_on_the_selected_weights(dev, use_graph):
    kf, sup, joints, vis = _batch(dev)
    vis = vis.clone()
    vis[1] = 0
    vis[1, [0, 3, 7, 10, 16]] = 1                         # five visible joints: fewer than k
    a = _trainer(dev, use_graph, deterministic=True, ohkm_topk=8, mse_weight=0.75)
    final = a.step(kf, sup, joints, vis)[0]
    sel = a.ohkm_selection()
    assert sel.dtype == torch.bool and sel.shape == (2, 17) and sel.is_cuda
    t, w = FL.generate_heatmaps(joints, vis, 3, (W, H), HM)
    # the selection: torch.topk of the row losses computed on the host from the returned final_hm
    rows = ((w.cpu().double().reshape(2, 17, 1, 1) * (final.detach().cpu().double() - t.cpu().double())) ** 2).mean((2, 3))
    want = torch.zeros(2, 17, dtype=torch.bool)
    for b in range(2):
        want[b, torch.topk(rows[b], 8).indices] = True
    want &= rows > 0                                      # weight-0 joints that fill the k places read False
    assert torch.equal(sel.cpu(), want)
    assert sel[0].sum().item() == 8 and torch.equal(sel[1].cpu(), w.reshape(2, 17)[1].cpu() != 0) and sel[1].sum().item() == 5
    assert np.array_equal(sel.cpu().numpy(), tref.ohkm_select(rows.numpy(), 8) & (rows.numpy() > 0))
    b = _plain(dev, use_graph, mse_weight=0.75 * 17 / 8)
    b.step(kf, sup, t, w * sel.reshape(2, 17, 1).float())
    e_l = abs(a.loss_parts[0].item() - b.loss_parts[0].item()) / abs(b.loss_parts[0].item())
    e_g = _relerr(a.grad, b.grad)
    print('ohkm_topk=8: loss relerr %.3g, gradient arena relerr %.3g' % (e_l, e_g))
    assert e_l <= 1e-6 and e_g <= 1e-6
    # the value: mse_weight (1/B) sum_b (1/k) sum_selected mean_p
    assert a.loss_parts[0].item() == pytest.approx(0.75 * rows[want].sum().item() / (2 * 8), rel=1e-5)


@GRAPH
def test_joint_weights_equal_a_plain_step_on_multiplied_weights(dev, use_graph):
    bt = _batch(dev)
    a = _trainer(dev, use_graph, deterministic=True, joint_weights=JOINTS_WEIGHT)
    a.step(*bt)
    t, w = FL.generate_heatmaps(bt[2], bt[3], 3, (W, H), HM, joint_weights=JOINTS_WEIGHT)
    assert set(w.unique().tolist()) <= {0.0, 1.0, float(np.float32(1.2)), 1.5} and (w == 1.5).any()
    b = _plain(dev, use_graph)
    b.step(bt[0], bt[1], t, w)
    assert torch.equal(a.grad, b.grad) and torch.equal(a.loss_parts, b.loss_parts) and torch.equal(a.acc, b.acc)
    assert not torch.equal(a.grad, _default_step(dev, use_graph)[0])


@GRAPH
def test_subpixel_encoding_equals_a_plain_step_on_subpixel_targets(dev, use_graph):
    """PCK takes the argmax of the target map.  No joint of this batch sits at exactly half a heatmap pixel (asserted), so
    the sub-pixel map's maximum is the quantised map's and the PCK rows are the quantised Trainer's; AT .5 the sub-pixel
    map has two equal maxima and its first is the lower pixel -- nothing is asserted across that."""
    bt = _batch(dev)
    c = bt[2].cpu().double() / 4
    assert ((c % 1) != 0.5).all()
    a = _trainer(dev, use_graph, deterministic=True, target_encoding='subpixel')
    a.step(*bt)
    t, w = FL.generate_heatmaps(bt[2], bt[3], 3, (W, H), HM, encoding='subpixel')
    b = _plain(dev, use_graph)
    b.step(bt[0], bt[1], t, w)
    assert torch.equal(a.grad, b.grad) and torch.equal(a.loss_parts, b.loss_parts) and torch.equal(a.acc, b.acc)
    grad, parts, acc = _default_step(dev, use_graph)
    assert torch.equal(a.acc, acc)
    assert not torch.equal(a.grad, grad)


def _all_options_run(dev, use_graph):
    tr = _trainer(dev, use_graph, deterministic=True, mode='f16', target_encoding='subpixel', joint_weights=JOINTS_WEIGHT,
                  ohkm_topk=8, accum_steps=2, max_grad_norm=1.0, loss_scale='dynamic', scaler=dict(init_scale=1024.0))
    start = tr.flat.detach().clone()
    sels = []
    for k in range(4):
        tr.step(*_batch(dev, 9 + k))
        sels.append(tr.ohkm_selection().clone())
    torch.cuda.synchronize(dev)
    return tr, start, sels


@GRAPH
def test_all_options_with_accumulation_clipping_and_dynamic_scale(dev, use_graph):
    a, start, sels = _all_options_run(dev, use_graph)
    assert a.window_position == 0 and a.opt.state[0].item() + a.skipped_steps() == 2.0 and a.opt.state[0].item() >= 1.0
    assert not torch.equal(a.flat, start) and torch.isfinite(a.flat).all()
    assert all(s.sum().item() <= 16 for s in sels) and sels[0].sum().item() > 0
    if use_graph:
        assert len(a._cache) == 1
    flat, grad, parts = a.flat.detach().clone(), a.grad.detach().clone(), a.loss_parts.clone()
    del a
    b, _, sels_b = _all_options_run(dev, use_graph)
    assert torch.equal(b.flat, flat) and torch.equal(b.grad, grad) and torch.equal(b.loss_parts, parts)
    assert all(torch.equal(x, y) for x, y in zip(sels, sels_b))
