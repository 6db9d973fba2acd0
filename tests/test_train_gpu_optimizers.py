"""The Trainer with TRAIN.OPTIMIZER 'sgd' and with two learning-rate groups (TRAIN.LR_SECOND_GROUP) on the MI355X
(posetimation/optimizer/optimizer.py:16-76, scheduler.py:14-27, engine/defaults/trainer.py:63-77,
engine/defaults/checkpoints.py:45-107): the step equals torch.optim.SGD / a list of torch.optim.Adam applied to the
Trainer's own gradients, eagerly, under hipGraph replay and with the early in-backward update; an LR schedule per group
keeps the captured plan; save -> resume -> continue is bitwise the uninterrupted run."""
import pytest
import torch

import fami_pose_amd as fp
from oracle import model as om

pytestmark = pytest.mark.gpu

S, H, W, B = 2, 128, 96, 2
HRNET = [(('hrnet',), 1e-5)]


def _model(seed=5):
    orc = om.realistic_init_(om.AlignmentOracle(om.make_cfg(48), True, S, (H, W)), seed)
    model = fp.build_model(fp.default_cfg(48, image_size=(W, H), num_sup=S), 'train')
    model.load_state_dict(orc.state_dict())
    return model


def _batch(dev, seed=9):
    gen = torch.Generator().manual_seed(seed)
    kf, sup = torch.randn(B, 3, H, W, generator=gen), torch.randn(B, 3 * S, H, W, generator=gen)
    joints = torch.rand(B, 17, 2, generator=gen) * torch.tensor([W, H], dtype=torch.float32)
    vis = (torch.rand(B, 17, generator=gen) < 0.8).float()
    return tuple(t.to(dev) for t in (kf, sup, joints, vis))


def _relerr(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


def _trainer(dev, use_graph, deterministic=False, **kw):
    from fami_pose_amd.train import Trainer
    model = _model().to(dev)
    if deterministic:
        model.set_deterministic(True)
    return Trainer(model, use_graph=use_graph, targets_from_joints=True, **kw)


@pytest.mark.parametrize('use_graph', [False, True])
def test_sgd_trainer_matches_torch_sgd_on_its_own_gradients(dev, use_graph):
    """Two steps (the momentum buffer's first-step rule, then the running rule) with the early in-backward split on"""
    kw = dict(optimizer='sgd', lr=0.01, momentum=0.9, weight_decay=1e-4, nesterov=use_graph)
    tr = _trainer(dev, use_graph, **kw)
    assert tr._adam_split is not None and tr.optimizers == [tr.opt]
    ref = torch.nn.Parameter(tr.flat.detach().cpu().clone())
    opt = torch.optim.SGD([ref], lr=0.01, momentum=0.9, weight_decay=1e-4, nesterov=use_graph)
    bt = _batch(dev)
    for k in range(2):
        tr.step(*bt)
        ref.grad = tr.grad.detach().cpu().clone()
        assert ref.grad.abs().max() > 0
        opt.step()
    torch.cuda.synchronize(dev)
    assert _relerr(tr.flat.cpu(), ref.data) < 1e-6
    assert _relerr(tr.opt.buf.cpu(), opt.state[ref]['momentum_buffer']) < 1e-6
    if use_graph:
        assert len(tr._cache) == 1


def test_two_adam_groups_match_two_torch_adams(dev):
    """hrnet.* at 1e-5, the rest at 1e-3, three captured steps: each group equals its own torch.optim.Adam on the
    Trainer's gradients, and the backbone moves by its own rate only (Adam's first update is ~lr per element)."""
    tr = _trainer(dev, True, lr=1e-3, lr_groups=HRNET)
    assert tr._adam_split is not None and len(tr.optimizers) == 2
    (blo, bhi), = tr.optimizers[0].runs
    (hlo, hhi), = tr.optimizers[1].runs
    flat0 = tr.flat.detach().cpu().clone()
    refs = [torch.nn.Parameter(flat0[blo:bhi].clone()), torch.nn.Parameter(flat0[hlo:hhi].clone())]
    opts = [torch.optim.Adam([refs[0]], lr=1e-3), torch.optim.Adam([refs[1]], lr=1e-5)]
    bt = _batch(dev)
    for k in range(3):
        before = tr.flat.detach().cpu().clone()
        tr.step(*bt)
        g = tr.grad.detach().cpu()
        refs[0].grad, refs[1].grad = g[blo:bhi].clone(), g[hlo:hhi].clone()
        for o in opts:
            o.step()
        if k == 0:
            d = (tr.flat.detach().cpu() - before).abs()
            assert d[blo:bhi].max().item() == pytest.approx(1e-3, rel=1e-3)
            assert d[hlo:hhi].max().item() == pytest.approx(1e-5, rel=0.05)      # (fp32 rounding of the weights)
    out = tr.flat.detach().cpu()
    assert _relerr(out[blo:bhi], refs[0].data) < 1e-6 and _relerr(out[hlo:hhi], refs[1].data) < 1e-6
    assert [o.state[0].item() for o in tr.optimizers] == [3.0, 3.0] and len(tr._cache) == 1


def test_lr_schedule_per_group_drives_the_captured_plan(dev):
    """build_lr_scheduler on two groups: a list of two MultiStepLR (scheduler.py:14-27); each group decays its own
    device-resident rate and the captured plan keeps replaying"""
    from fami_pose_amd.train import build_lr_scheduler
    tr = _trainer(dev, True, lr=1e-3, lr_groups=[(('hrnet',), 1e-4)])
    cfg = fp.default_cfg(48)
    cfg['TRAIN'].update(LR_STEP=[1, 2], LR_FACTOR=0.1)
    scheds = build_lr_scheduler(cfg, tr)
    assert isinstance(scheds, list) and len(scheds) == 2
    bt = _batch(dev)
    (blo, bhi), = tr.optimizers[0].runs
    (hlo, hhi), = tr.optimizers[1].runs
    deltas = []
    for epoch in range(3):
        before = tr.flat.detach().clone()
        tr.step(*bt)
        d = (tr.flat.detach() - before).abs()
        deltas.append((d[blo:bhi].max().item(), d[hlo:hhi].max().item()))
        for s in scheds:
            s.step()
    # Adam's update is ~lr in magnitude for its first steps
    assert deltas[0][0] == pytest.approx(1e-3, rel=0.05) and deltas[0][1] == pytest.approx(1e-4, rel=0.05)
    assert deltas[1][0] == pytest.approx(1e-4, rel=0.35) and deltas[1][1] == pytest.approx(1e-5, rel=0.35)
    assert deltas[2][0] == pytest.approx(1e-5, rel=0.5) and deltas[2][1] == pytest.approx(1e-6, rel=0.5)
    assert tr.optimizers[0].state[1].item() == pytest.approx(1e-5, rel=1e-5)
    assert tr.optimizers[1].state[1].item() == pytest.approx(1e-6, rel=1e-5)
    assert len(tr._cache) == 1
    plan0 = list(tr._cache.values())[0][0]
    tr.optimizers[1].set_hyper(betas=(0.8, 0.99))
    tr.step(*bt)
    assert list(tr._cache.values())[0][0] is not plan0          # a group's kernel arguments changed: re-captured


def _run(dev, steps, batches, kw, resume_from=None, save_at=None, tmp=None):
    from fami_pose_amd import checkpoint as ck
    tr = _trainer(dev, True, deterministic=True, **kw)
    start = 0
    if resume_from is not None:
        _, _, start = ck.resume(tr.model, tr, resume_from)
    for k in range(start, steps):
        tr.step(*batches[k])
        if save_at is not None and k + 1 == save_at:
            ck.save_checkpoint(k, tmp, tr.model, tr)
    return tr


@pytest.mark.parametrize('kw', [dict(optimizer='sgd', lr=0.01, momentum=0.9, weight_decay=1e-4),
                                dict(lr=1e-3, lr_groups=HRNET)], ids=['sgd', 'two_groups'])
def test_resume_continues_bitwise(dev, tmp_path, kw):
    """train 2 steps, save, resume into a FRESH model + Trainer, take step 3: parameters, optimizer arenas, rates and
    BatchNorm buffers equal the uninterrupted 3-step run bit for bit"""
    from fami_pose_amd import checkpoint as ck
    batches = [_batch(dev, 9 + k) for k in range(3)]
    full = _run(dev, 3, batches, kw)
    folder = str(tmp_path / 'ckpt')
    _run(dev, 2, batches, kw, save_at=2, tmp=folder)
    saved = torch.load(ck.get_latest_checkpoint(folder), map_location='cpu')['optimizer']
    assert len(saved) == len(full.optimizers)
    res = _run(dev, 3, batches, kw, resume_from=ck.get_latest_checkpoint(folder))
    assert torch.equal(res.flat, full.flat)
    for a, b in zip(res.optimizers, full.optimizers):
        for x, y in zip(a.tensors()[:-1], b.tensors()[:-1]):          # moment arenas / momentum buffer
            assert torch.equal(x, y)
        assert torch.equal(a.state[1], b.state[1])
        if a.kind == 'adam':
            assert torch.equal(a.state, b.state)
    for (n1, b1), (n2, b2) in zip(res.model.named_buffers(), full.model.named_buffers()):
        assert n1 == n2 and torch.equal(b1, b2), n1
