"""Trainer(ema_decay=d): the device-resident exponential moving average of the weights on the MI355X.  The recurrence
(float64 on host copies of the parameter arena taken after every step), eager launches and hipGraph replay, Adam and SGD;
skipped fp16 steps leave the average alone; one update per accumulation window; clipping with learning-rate groups; the
data-parallel plans with one rank over RCCL; ema_weights() puts the average into the model and takes it out bit for bit;
save -> resume continues bit for bit; a default Trainer launches none of it.

Sizes and helpers are those of tests/test_train_gpu_clip.py.  The bound on the recurrence: one update is within
3 * 2^-24 * max(|param|, |ema|) of its float64 value (tests/test_ema_gpu.py), the errors of earlier updates are carried
forward with weights <= 1, so after at most four updates the average is within 4 * 3 * 2^-24 * max|param| of the float64
recurrence."""
import os
import subprocess
import sys

import pytest
import torch

import fami_pose_amd as fp
from test_train_gpu_clip import S, H, W, HRNET, _batch, _model, _trainer

pytestmark = pytest.mark.gpu
NEW = ('fami_ema_prep_f32', 'fami_ema_update_f32', 'fami_swap_f32')
ADAM, SGD = dict(lr=1e-3), dict(optimizer='sgd', lr=0.01, momentum=0.9, weight_decay=1e-4)


class _Recurrence:
    """ema_k = ema_{k-1} + w (p_k - ema_{k-1}) in float64 on the host, from the construction-time parameters; w is the
    fp32 weight the device used, read back from ema_state"""

    def __init__(self, tr):
        self.ref = tr.flat.detach().cpu().double()
        self.peak = self.ref.abs().max().item()
        self.k = 0

    def update(self, tr):
        p = tr.flat.detach().cpu().double()
        w = float(tr.ema_state[2].item())
        self.ref = self.ref + w * (p - self.ref)
        self.peak = max(self.peak, p.abs().max().item())
        self.k += 1

    def check(self, tr, what=''):
        err = (tr.ema.detach().cpu().double() - self.ref).abs().max().item()
        bound = 4 * 3 * 2.0 ** -24 * self.peak
        print('%s update %d: |ema - float64 recurrence| %.3g, bound %.3g' % (what, self.k, err, bound))
        assert self.k <= 4 and err <= bound, (what, self.k, err, bound)


@pytest.mark.parametrize('use_graph', [False, True], ids=['eager', 'graph'])
@pytest.mark.parametrize('kind', ['adam', 'sgd'])
def test_average_follows_the_recurrence(dev, use_graph, kind):
    tr = _trainer(dev, use_graph, ema_decay=0.5, **(ADAM if kind == 'adam' else SGD))
    assert tr.ema is not None and tr.ema.shape == tr.flat.shape and tr.ema.data_ptr() != tr.flat.data_ptr()
    assert torch.equal(tr.ema, tr.flat) and tr.ema_updates() == 0 and tr.ema_decay_value() == 0.5
    rec = _Recurrence(tr)
    for k in range(4):
        before = tr.flat.detach().clone()
        tr.step(*_batch(dev, 9 + k))
        assert tr.ema_updates() == k + 1          # graph mode: the capture's warm-up steps were rolled back
        assert not torch.equal(tr.flat, before)
        rec.update(tr)
        rec.check(tr, '%s %s' % (kind, 'graph' if use_graph else 'eager'))
        assert not torch.equal(tr.ema, tr.flat)
    assert tr.opt.state[0].item() == 4.0 and tr.ema_decay_value() == 0.5
    if use_graph:
        assert len(tr._cache) == 1


def test_skipped_steps_leave_the_average_alone(dev):
    """fp16 with a dynamic scale starting at 2^40 (tests/test_train_gpu_clip.py derives why it overflows): every skipped
    step leaves `ema` and its update count untouched; the first applied step moves it"""
    tr = _trainer(dev, True, mode='f16', loss_scale='dynamic', scaler=dict(init_scale=2.0 ** 40), ema_decay=0.5)
    bt = _batch(dev)
    start = tr.ema.detach().clone()
    skipped = 0
    for _ in range(42):
        tr.step(*bt)
        if tr.skipped_steps() == skipped:
            break
        skipped = tr.skipped_steps()
        assert torch.equal(tr.ema.view(torch.int32), start.view(torch.int32)) and tr.ema_updates() == 0
        assert torch.equal(tr.flat, start)
    else:
        pytest.fail('no step was applied within 42 steps')
    print('%d skipped steps before the first applied one' % skipped)
    assert skipped >= 1 and tr.ema_updates() == 1 and tr.opt.state[0].item() == 1.0
    assert not torch.equal(tr.ema, start) and torch.equal(tr.ema, start + tr.ema_state[2] * (tr.flat - start))
    assert len(tr._cache) == 1


@pytest.mark.parametrize('use_graph', [False, True], ids=['eager', 'graph'])
def test_one_update_per_accumulation_window(dev, use_graph):
    tr = _trainer(dev, use_graph, lr=1e-3, accum_steps=3, ema_decay=0.5)
    start = tr.ema.detach().clone()
    for k in range(2):
        tr.step(*_batch(dev, 9 + k))
        assert torch.equal(tr.ema.view(torch.int32), start.view(torch.int32)) and tr.ema_updates() == 0
    tr.step(*_batch(dev, 11))
    assert tr.ema_updates() == 1 and tr.opt.state[0].item() == 1.0 and not torch.equal(tr.flat, start)
    assert torch.equal(tr.ema, start + tr.ema_state[2] * (tr.flat - start)) and not torch.equal(tr.ema, start)
    tr.step(*_batch(dev, 12))
    assert tr.ema_updates() == 1
    if use_graph:
        assert len(tr._cache) == 1


def test_clipping_and_learning_rate_groups_together(dev):
    tr = _trainer(dev, True, lr=1e-3, max_grad_norm=1.0, lr_groups=HRNET, ema_decay=0.5)
    assert len(tr.optimizers) == 2
    rec = _Recurrence(tr)
    for k in range(3):
        tr.step(*_batch(dev, 9 + k))
        assert tr.ema_updates() == k + 1
        rec.update(tr)
        rec.check(tr, 'clip + groups')
    assert tr.clip_coef() < 1.0 and tr.skipped_steps() == 0 and len(tr._cache) == 1


def test_data_parallel_plans_single_rank(dev):
    """The 'serial' and 'overlap' plans (and the accumulating serial tail) with ONE rank over RCCL, in a child process
    (tests/_ddp_single_rank_ema.py; tests/test_model_gpu.py::test_ddp_path_single_rank_rccl says why a child)."""
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT='29523')
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), '_ddp_single_rank_ema.py')],
                       env=env, capture_output=True, text=True, timeout=900)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'DDP_EMA_SINGLE_RANK_OK' in r.stdout


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
def test_ema_weights_context(dev, mode):
    kw = dict(deterministic=True, mode=mode, lr=1e-3, ema_decay=0.5)
    tr, twin = _trainer(dev, True, **kw), _trainer(dev, True, **kw)
    for k in range(2):
        tr.step(*_batch(dev, 9 + k))
        twin.step(*_batch(dev, 9 + k))
    assert torch.equal(tr.flat, twin.flat) and torch.equal(tr.ema, twin.ema)
    flat, ema = tr.flat.detach().clone(), tr.ema.detach().clone()
    assert not torch.equal(flat, ema)
    entry = tr.ema_state_dict()
    kf, sup = _batch(dev, 30)[:2]
    # the second model: built fresh, given the averaged parameters over the live buffers
    other = fp.build_model(fp.default_cfg(48, image_size=(W, H), num_sup=S), 'train')
    other.load_state_dict({**{k: v.detach().cpu() for k, v in tr.model.state_dict().items()}, **entry['params']}, strict=True)
    other = other.to(dev).set_compute_dtype(mode).set_deterministic(True)
    # the same launch plan as tr.model, incl. the arena layout: adjacent predictor weights run as ONE convolution, which sums in
    # another order than the two convolutions of a model whose parameters were allocated one by one (the bitwise comparison of
    # tests/test_train_gpu.py::test_frozen_weight_image_is_not_reused_after_training lays its fresh model out the same way)
    from fami_pose_amd.train import Trainer
    Trainer(other, use_graph=False, targets_from_joints=True)
    other.eval()
    with torch.no_grad():
        want = other(kf, sup)
    tr.model.eval()
    with torch.no_grad():
        raw = tr.model(kf, sup)
    with tr.ema_weights() as inside:
        assert inside is tr
        sd = tr.model.state_dict()
        names = [k for k, p in tr.model.named_parameters() if p.requires_grad]
        assert names == list(entry['params'])
        for (p, off, n), k in zip(tr.table, names):
            assert torch.equal(sd[k].reshape(-1), ema[off:off + n]), k
        assert torch.equal(tr.flat, ema) and torch.equal(tr.ema, flat)
        with torch.no_grad():
            got = tr.model(kf, sup)
        with pytest.raises(RuntimeError):
            tr.step(*_batch(dev, 11))
        with pytest.raises(RuntimeError):
            with tr.ema_weights():
                pass
        with pytest.raises(RuntimeError):
            tr.ema_state_dict()
    tr.model.train()
    assert torch.equal(tr.flat.view(torch.int32), flat.view(torch.int32))
    assert torch.equal(tr.ema.view(torch.int32), ema.view(torch.int32))
    for g, w, r in zip(got[:2], want[:2], raw[:2]):
        print('%s: |inside - fresh model| %.3g, |inside - raw weights| %.3g' % (mode, (g - w).abs().max().item(), (g - r).abs().max().item()))
        assert torch.equal(g, w) and not torch.equal(g, r)
    tr.step(*_batch(dev, 11))
    twin.step(*_batch(dev, 11))
    assert torch.equal(tr.flat, twin.flat) and torch.equal(tr.ema, twin.ema) and tr.ema_updates() == 3
    assert len(tr._cache) == 1


def test_save_checkpoint_inside_the_context_is_refused(dev, tmp_path):
    from fami_pose_amd import checkpoint as ck
    tr = _trainer(dev, False, ema_decay=0.9)
    with tr.ema_weights():
        with pytest.raises(RuntimeError):
            ck.save_checkpoint(0, str(tmp_path), tr.model, tr)
    assert not list(tmp_path.iterdir())
    plain = _trainer(dev, False)
    with pytest.raises(ValueError):
        with plain.ema_weights():
            pass


def test_resume_in_the_middle_of_a_run_continues_bitwise(dev, tmp_path):
    """save after two steps, resume into a FRESH graph-mode Trainer: two more steps leave parameters, average and state
    vector bitwise those of the run that went on without interruption"""
    from fami_pose_amd import checkpoint as ck
    bts = [_batch(dev, 9 + k) for k in range(4)]
    kw = dict(deterministic=True, lr=1e-3, ema_decay=0.999, ema_warmup=True)
    full = _trainer(dev, True, **kw)
    for bt in bts[:2]:
        full.step(*bt)
    path = ck.save_checkpoint(0, str(tmp_path), full.model, full)
    at_save = (full.flat.detach().clone(), full.ema.detach().clone(), full.ema_state.detach().clone())
    saved = torch.load(path, map_location='cpu')
    assert sorted(saved) == ['begin_epoch', 'ema', 'optimizer', 'state_dict']
    assert saved['ema']['updates'] == 2 and saved['ema']['decay'] == 0.999 and saved['ema']['warmup'] is True
    for bt in bts[2:]:
        full.step(*bt)
    res = _trainer(dev, True, **kw)
    ck.resume(res.model, res, path)
    assert torch.equal(res.flat, at_save[0]) and torch.equal(res.ema, at_save[1]) and torch.equal(res.ema_state, at_save[2])
    assert res.ema_updates() == 2 and not torch.equal(res.ema, res.flat)
    for bt in bts[2:]:
        res.step(*bt)
    assert torch.equal(res.flat, full.flat) and torch.equal(res.ema, full.ema) and torch.equal(res.ema_state, full.ema_state)
    assert res.ema_updates() == 4 and res.ema_decay_value() == pytest.approx(5.0 / 14.0, rel=1e-6)


def test_resume_without_the_entry_and_without_an_average(dev, tmp_path):
    from fami_pose_amd import checkpoint as ck
    av = _trainer(dev, False, lr=1e-3, ema_decay=0.9)
    plain = _trainer(dev, False, lr=1e-3)
    av.step(*_batch(dev, 9))
    plain.step(*_batch(dev, 10))
    assert av.ema_updates() == 1 and not torch.equal(av.ema, av.flat) and not torch.equal(av.flat, plain.flat)
    with_entry = ck.save_checkpoint(0, str(tmp_path / 'a'), av.model, av)
    without = ck.save_checkpoint(0, str(tmp_path / 'b'), plain.model, plain)
    assert sorted(torch.load(without, map_location='cpu')) == ['begin_epoch', 'optimizer', 'state_dict']
    was = av.flat.detach().clone()
    # a file without the entry: the average restarts from the loaded weights
    ck.resume(av.model, av, without)
    assert torch.equal(av.flat, plain.flat) and torch.equal(av.ema, av.flat) and av.ema_updates() == 0
    # ... and a Trainer without an average ignores the entry
    ck.resume(plain.model, plain, with_entry)
    assert torch.equal(plain.flat, was) and plain.ema is None


def test_set_ema_decay_recaptures_and_reset_ema(dev):
    tr = _trainer(dev, True, lr=1e-3, ema_decay=0.5)
    bt = _batch(dev)
    tr.step(*bt)
    plan = list(tr._cache.values())[0][0]
    tr.set_ema_decay(0.5)
    tr.step(*bt)
    assert list(tr._cache.values())[0][0] is plan           # unchanged: no re-capture
    tr.set_ema_decay(0.75)
    before = tr.ema.detach().clone()
    tr.step(*bt)
    assert list(tr._cache.values())[0][0] is not plan and len(tr._cache) == 1
    assert tr.ema_updates() == 3 and tr.ema_decay_value() == 0.75 and tr.ema_state[2].item() == 0.25
    assert torch.equal(tr.ema, before + tr.ema_state[2] * (tr.flat - before))
    tr.reset_ema()
    assert torch.equal(tr.ema, tr.flat) and tr.ema_updates() == 0
    for bad in (0.0, 1.0, 'x'):
        with pytest.raises(ValueError):
            tr.set_ema_decay(bad)


@pytest.mark.parametrize('mode', ['f32', 'f16'])
def test_default_trainer_launches_none_of_it(dev, mode, monkeypatch, tmp_path):
    from fami_pose_amd import checkpoint as ck
    from fami_pose_amd._lib import lib
    tr = _trainer(dev, False, mode=mode)
    assert tr.ema_decay is None and tr.ema is None and tr.ema_state is None
    assert tr.ema_updates() is None and tr.ema_decay_value() is None
    names = []
    L = lib()
    call, call_routed = L.call, L.call_routed
    monkeypatch.setattr(L, 'call', lambda name, *a: (names.append(name), call(name, *a))[1])
    monkeypatch.setattr(L, 'call_routed', lambda route, name, *a: (names.append(name), call_routed(route, name, *a))[1])
    tr.step(*_batch(dev))
    torch.cuda.synchronize(dev)
    assert len(names) > 100 and 'fami_adam_f32' in names and not set(names) & set(NEW)
    path = ck.save_checkpoint(0, str(tmp_path), tr.model, tr)
    assert sorted(torch.load(path, map_location='cpu')) == ['begin_epoch', 'optimizer', 'state_dict']
    # ... and an averaging one launches prep and update exactly once per step, directly behind the optimizer
    names.clear()
    av = _trainer(dev, False, mode=mode, ema_decay=0.999)
    av.step(*_batch(dev))
    assert names.count('fami_ema_prep_f32') == 1 and names.count('fami_ema_update_f32') == 1 and 'fami_swap_f32' not in names
    assert names[-2:] == ['fami_ema_prep_f32', 'fami_ema_update_f32']
    assert max(i for i, n in enumerate(names) if n == 'fami_adam_f32') < names.index('fami_ema_prep_f32')


def test_argument_checks(dev):
    from fami_pose_amd.train import Trainer
    model = _model().to(dev)
    for bad in (0, 1, 0.0, 1.0, -0.1, '0.5', True):
        with pytest.raises(ValueError):
            Trainer(model, use_graph=False, ema_decay=bad)
    with pytest.raises(ValueError):
        Trainer(model, use_graph=False, ema_warmup=True)
    tr = Trainer.from_cfg(fp.default_cfg(48, image_size=(W, H), num_sup=S), model, use_graph=False, ema_decay=0.999,
                          ema_warmup=True)
    assert tr.ema_decay == 0.999 and tr.ema_warmup is True and tr.ema is not None and torch.equal(tr.ema, tr.flat)
