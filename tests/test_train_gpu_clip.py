"""The Trainer with global-norm gradient clipping (max_grad_norm) and a dynamic fp16 loss scale (loss_scale='dynamic') on
the MI355X.  The oracle is torch on the CPU: torch.nn.utils.clip_grad_norm_ + torch.optim.Adam / SGD applied to the
Trainer's own gradients, and torch.amp.GradScaler's update rule.  Eager launches and hipGraph replay; threshold and
scale move without a re-capture; save -> resume continues bit for bit; a default Trainer launches none of it."""
import math

import pytest
import torch

import fami_pose_amd as fp
from oracle import model as om

pytestmark = pytest.mark.gpu

S, H, W, B = 2, 128, 96, 2
HRNET = [(('hrnet',), 1e-5)]
NEW = ('fami_sumsq_f32', 'fami_unscale_check_sumsq_f32', 'fami_clip_coef_f32', 'fami_adam_scaled_f32',
       'fami_sgd_scaled_f32', 'fami_loss_scale_update_f32')


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


def _trainer(dev, use_graph, deterministic=False, mode=None, **kw):
    from fami_pose_amd.train import Trainer
    model = _model().to(dev)
    if mode is not None:
        model.set_compute_dtype(mode)
    if deterministic:
        model.set_deterministic(True)
    return Trainer(model, use_graph=use_graph, targets_from_joints=True, **kw)


class _TorchTwin:
    """The torch side: one nn.Parameter per trainable parameter of the Trainer, as views of one host copy of its arena --
    clip_grad_norm_ then sees what it sees in a torch training loop (a norm per parameter tensor, then the norm of the
    norms).  Handed the 64.7 M-element arena as ONE tensor its fp32 reduction is off by 0.4 % (measured: 2.03027 against
    the float64 2.03855), which is not the oracle."""

    def __init__(self, tr):
        self.flat = tr.flat.detach().cpu().clone()
        self.spans = [(o, n) for _, o, n in tr.table]
        self.params = [torch.nn.Parameter(self.flat[o:o + n]) for o, n in self.spans]
        assert self.params[0].data_ptr() == self.flat[self.spans[0][0]:].data_ptr()

    def inside(self, lo, hi):
        return [p for p, (o, n) in zip(self.params, self.spans) if lo <= o and o + n <= hi]

    def clip(self, grad, max_norm):
        g = grad.detach().cpu()
        for p, (o, n) in zip(self.params, self.spans):
            p.grad = g[o:o + n].clone()
        return torch.nn.utils.clip_grad_norm_(self.params, max_norm).item()


def _norm_bound(t):
    """(k + 3) 2^-24 with k the longest fp32 addition chain of the norm kernel over t (tests/test_clip_gpu.py derives it)"""
    from fami_pose_amd._lib import lib
    n = t.numel()
    head = min(n, ((16 - t.data_ptr() % 16) % 16) // 4)
    chunk = -(-((n - head) // 4) // lib().cdll.fami_sumsq_parts())
    return (-(-chunk // 256) + 11 + 3) * 2.0 ** -24


@pytest.mark.parametrize('use_graph', [False, True], ids=['eager', 'graph'])
@pytest.mark.parametrize('kind', ['adam', 'sgd'])
def test_clipped_trainer_matches_clip_grad_norm_on_its_own_gradients(dev, use_graph, kind):
    """Step 1 runs with a threshold far above the norm (coef == 1) and measures the norm; the threshold then drops to a
    tenth of it (the same batch every step: Adam shrinks the norm sevenfold in three steps), so steps 2-4 clip.  After
    every step grad_norm() is the float64 norm of the gradient arena within the derived bound, and the parameters equal
    clip_grad_norm_ + the torch optimizer on copies of trainer.grad."""
    kw = dict(lr=1e-3) if kind == 'adam' else dict(optimizer='sgd', lr=0.01, momentum=0.9, weight_decay=1e-4)
    tr = _trainer(dev, use_graph, max_grad_norm=1e9, **kw)
    assert tr._adam_split is None and tr.overflow is not None and tr.opt.gmul is not None
    twin = _TorchTwin(tr)
    opt = (torch.optim.Adam(twin.params, lr=1e-3) if kind == 'adam' else
           torch.optim.SGD(twin.params, lr=0.01, momentum=0.9, weight_decay=1e-4))
    bt = _batch(dev)
    max_norm, coefs = 1e9, []
    for k in range(4):
        tr.step(*bt)
        g = tr.grad.detach().cpu()
        want = g.double().norm().item()
        got = tr.grad_norm()
        err = abs(got - want) / want
        print('step %d: grad_norm %.9g  float64 %.9g  relative error %.3g  bound %.3g  coef %.6g' %
              (k, got, want, err, _norm_bound(tr.grad), tr.clip_coef()))
        assert err <= _norm_bound(tr.grad)
        coefs.append(tr.clip_coef())
        assert coefs[-1] == pytest.approx(min(1.0, max_norm / (got + 1e-6)), rel=1e-6)
        total = twin.clip(tr.grad, max_norm)
        print('        torch total_norm %.9g (relative to float64 %.3g)' % (total, abs(total - want) / want))
        opt.step()
        if k == 0:
            max_norm = 0.1 * got
            tr.set_max_grad_norm(max_norm)
    assert coefs[0] == 1.0 and min(coefs[1:]) < 1.0          # clipping was active
    e = _relerr(tr.flat.cpu(), twin.flat)
    print('parameters relerr %.3g' % e)
    assert e < 1e-6
    assert tr.skipped_steps() == 0
    if use_graph:
        assert len(tr._cache) == 1


def test_threshold_changes_need_no_recapture(dev):
    tr = _trainer(dev, True, max_grad_norm=1e9)
    bt = _batch(dev)
    tr.step(*bt)
    assert tr.clip_coef() == 1.0
    plan0, graphs0 = list(tr._cache.values())[0][0], tr.plan_summary()['graphs']
    norm = tr.grad_norm()
    for frac in (0.5, 0.125, 4.0):
        tr.set_max_grad_norm(frac * norm)
        tr.step(*bt)
        want = min(1.0, frac * norm / (tr.grad_norm() + 1e-6))
        assert tr.clip_coef() == pytest.approx(want, rel=1e-6)
        assert (tr.clip_coef() < 1.0) == (want < 1.0)
    assert len(tr._cache) == 1 and list(tr._cache.values())[0][0] is plan0 and tr.plan_summary()['graphs'] == graphs0
    with pytest.raises(ValueError):
        tr.set_max_grad_norm(0.0)


def test_two_learning_rate_groups_share_one_coefficient(dev):
    """one clip_grad_norm_ over all parameters, then each group's own torch.optim.Adam"""
    tr = _trainer(dev, True, lr=1e-3, lr_groups=HRNET, max_grad_norm=1e9)
    assert len(tr.optimizers) == 2 and all(o.gmul is not None and o.gmul.data_ptr() == tr.opt.gmul.data_ptr() for o in tr.optimizers)
    (blo, bhi), = tr.optimizers[0].runs
    (hlo, hhi), = tr.optimizers[1].runs
    twin = _TorchTwin(tr)
    groups = [twin.inside(blo, bhi), twin.inside(hlo, hhi)]
    assert len(groups[0]) + len(groups[1]) == len(twin.params) and groups[0] and groups[1]
    opts = [torch.optim.Adam(groups[0], lr=1e-3), torch.optim.Adam(groups[1], lr=1e-5)]
    bt = _batch(dev)
    max_norm = 1e9
    for k in range(3):
        tr.step(*bt)
        want = tr.grad.detach().cpu().double().norm().item()
        assert abs(tr.grad_norm() - want) / want <= _norm_bound(tr.grad)          # ONE norm over both groups
        twin.clip(tr.grad, max_norm)
        for o in opts:
            o.step()
        if k == 0:
            max_norm = 0.1 * tr.grad_norm()
            tr.set_max_grad_norm(max_norm)
        else:
            assert tr.clip_coef() < 1.0
    out = tr.flat.detach().cpu()
    e = (_relerr(out[blo:bhi], twin.flat[blo:bhi]), _relerr(out[hlo:hhi], twin.flat[hlo:hhi]))
    print('two groups relerr %.3g %.3g' % e)
    assert e[0] < 1e-6 and e[1] < 1e-6
    assert [o.state[0].item() for o in tr.optimizers] == [3.0, 3.0] and len(tr._cache) == 1


def test_dynamic_scale_equals_static_at_a_fixed_power_of_two(dev):
    """fp16, deterministic model: a dynamic scale pinned at 8192 (growth_interval 10^9) against the static 8192 from the same
    start -- with a power-of-two scale the device product gdev[0] * scale rounds like the host product and 1 / scale is
    exact, so the parameter arenas are equal bit for bit"""
    bts = [_batch(dev, 9 + k) for k in range(3)]
    a = _trainer(dev, True, deterministic=True, mode='f16', loss_scale=8192.0)
    b = _trainer(dev, True, deterministic=True, mode='f16', loss_scale='dynamic',
                 scaler=dict(init_scale=8192.0, growth_interval=10 ** 9))
    assert b.dynamic_scale and b.loss_scale == 8192.0 and not a.dynamic_scale
    assert torch.equal(a.flat, b.flat)
    for bt in bts:
        a.step(*bt)
        b.step(*bt)
        assert torch.equal(a.grad, b.grad)
        assert torch.equal(a.flat, b.flat)
    assert torch.equal(a.opt.m, b.opt.m) and torch.equal(a.opt.v, b.opt.v)
    assert a.skipped_steps() == b.skipped_steps() == 0 and b.loss_scale_value() == 8192.0
    assert b.scaler_state[2].item() == 3.0


def test_dynamic_scale_backs_off_and_recovers(dev):
    """fp16, graph mode, init_scale 2^40: the MSE seed is scale * 2 w^2 (pred - gt) * mse_weight / (B L J) with
    B L J = 2 * 768 * 17 = 26112, i.e. 2^40 * 7.7e-5 * error = 8.4e7 * error -- beyond fp16's 65504 for every heatmap
    error above 8e-4 (the Gaussian targets peak at 1), so the first steps overflow.  Only float VALUES overflow.
    While steps are skipped the parameters do not move and the scale halves; the scale reaches 1 after 40 halvings, so
    stepping resumes within log2(init_scale) + 1 = 41 steps; skipped_steps() counts the halvings; one captured plan
    throughout; growth_interval = 4 clean steps later the scale doubles.  (Measured on the MI355X: 18 halvings, the first
    step that runs does so at 2^22.)"""
    init = 2.0 ** 40
    tr = _trainer(dev, True, mode='f16', loss_scale='dynamic', scaler=dict(init_scale=init, growth_interval=4))
    assert tr.loss_scale == init and tr.dynamic_scale and tr.loss_scale_value() == init
    bt = _batch(dev)
    before = tr.flat.detach().clone()
    halvings, scale = 0, init
    for k in range(int(math.log2(init)) + 1):
        tr.step(*bt)
        now = tr.loss_scale_value()
        if tr.skipped_steps() == halvings:          # this step ran
            assert now == scale and not torch.equal(tr.flat, before)
            break
        halvings += 1
        assert tr.skipped_steps() == halvings and now == scale / 2 and torch.equal(tr.flat, before)
        scale = now
    else:
        pytest.fail('no step ran within log2(init_scale) + 1 steps')
    print('first overflow-free scale 2^%d after %d halvings' % (int(math.log2(scale)), halvings))
    assert halvings >= 1 and tr.skipped_steps() == halvings and torch.isfinite(tr.flat).all()
    assert tr.opt.state[0].item() == 1.0 and tr.scaler_state[2].item() == 1.0
    # three more clean steps complete the growth interval
    for k in range(3):
        assert tr.loss_scale_value() == scale
        tr.step(*bt)
    if tr.skipped_steps() == halvings:
        assert tr.loss_scale_value() == 2 * scale and tr.scaler_state[2].item() == 0.0
        assert tr.opt.state[0].item() == 4.0
    else:
        pytest.fail('a step at the scale that had just worked overflowed: %d skipped' % tr.skipped_steps())
    assert len(tr._cache) == 1 and tr.plan_summary()['graphs'] == 1


def _run(dev, steps, batches, kw, resume_from=None, save_at=None, tmp=None):
    from fami_pose_amd import checkpoint as ck
    tr = _trainer(dev, True, deterministic=True, mode='f16', **kw)
    start = 0
    if resume_from is not None:
        _, _, start = ck.resume(tr.model, tr, resume_from)
    for k in range(start, steps):
        tr.step(*batches[k])
        if save_at is not None and k + 1 == save_at:
            ck.save_checkpoint(k, tmp, tr.model, tr)
    return tr


def test_resume_restores_the_loss_scaler_and_continues_bitwise(dev, tmp_path):
    """init_scale 2^40 with a back-off of 2^-8 reaches a working scale in a few skipped steps; save after step 5 (past the
    back-offs, growth tracker under way), resume into a FRESH dynamic Trainer, continue: bitwise the uninterrupted run"""
    from fami_pose_amd import checkpoint as ck
    kw = dict(lr=1e-3, loss_scale='dynamic', max_grad_norm=1.0,
              scaler=dict(init_scale=2.0 ** 40, backoff_factor=2.0 ** -8, growth_interval=3))
    batches = [_batch(dev, 9 + k) for k in range(7)]
    full = _run(dev, 7, batches, kw)
    assert full.skipped_steps() >= 1 and full.opt.state[0].item() >= 2.0
    folder = str(tmp_path / 'ckpt')
    part = _run(dev, 5, batches, kw, save_at=5, tmp=folder)
    saved = torch.load(ck.get_latest_checkpoint(folder), map_location='cpu')
    assert sorted(saved) == ['begin_epoch', 'loss_scaler', 'optimizer', 'state_dict']
    assert sorted(saved['loss_scaler']) == sorted(torch.amp.GradScaler('cpu').state_dict())
    assert saved['loss_scaler']['scale'] == part.loss_scale_value() < 2.0 ** 40
    assert saved['loss_scaler']['_growth_tracker'] == int(part.scaler_state[2].item())
    res = _run(dev, 7, batches, kw, resume_from=ck.get_latest_checkpoint(folder))
    assert torch.equal(res.scaler_state, full.scaler_state)
    assert torch.equal(res.flat, full.flat)
    assert torch.equal(res.opt.m, full.opt.m) and torch.equal(res.opt.v, full.opt.v) and torch.equal(res.opt.state, full.opt.state)
    # a checkpoint without the entry loads into a dynamic Trainer and leaves its initial scale
    del saved['loss_scaler']
    plain = str(tmp_path / 'plain' / 'epoch_4_state.pth')
    import os
    os.makedirs(os.path.dirname(plain))
    torch.save(saved, plain)
    ck.resume(res.model, res, plain)
    assert torch.equal(res.scaler_state, full.scaler_state)
    # ... and a static Trainer writes exactly the three keys
    st = _trainer(dev, False, mode='f16', max_grad_norm=1.0)
    out = ck.save_checkpoint(0, str(tmp_path / 'static'), st.model, st)
    assert sorted(torch.load(out, map_location='cpu')) == ['begin_epoch', 'optimizer', 'state_dict']


@pytest.mark.parametrize('mode', ['f32', 'bf16', 'f16'])
def test_default_trainer_launches_none_of_it(dev, mode, monkeypatch):
    from fami_pose_amd._lib import lib
    tr = _trainer(dev, False, mode=mode)
    assert tr.max_grad_norm is None and not tr.dynamic_scale and tr.clip is None and tr.scaler_state is None
    assert all(o.gmul is None for o in tr.optimizers)
    if mode == 'f16':
        assert tr.loss_scale == 8192.0 and tr.overflow is not None
    else:
        assert tr.loss_scale == 1.0 and tr.overflow is None and tr._adam_split is not None
    names = []
    L = lib()
    call, call_routed = L.call, L.call_routed
    monkeypatch.setattr(L, 'call', lambda name, *a: (names.append(name), call(name, *a))[1])
    monkeypatch.setattr(L, 'call_routed', lambda route, name, *a: (names.append(name), call_routed(route, name, *a))[1])
    tr.step(*_batch(dev))
    torch.cuda.synchronize(dev)
    assert len(names) > 100 and ('fami_adam_f32' in names)
    assert not set(names) & set(NEW)
    assert ('fami_unscale_check_f32' in names) == (mode == 'f16')
    assert tr.grad_norm() is None and tr.clip_coef() is None and tr.loss_scale_value() == tr.loss_scale


def test_argument_checks(dev):
    from fami_pose_amd.train import Trainer
    model = _model().to(dev)
    for bad in (dict(max_grad_norm=0.0), dict(max_grad_norm=-1.0), dict(scaler=dict(init_scale=4.0)),
                dict(loss_scale=8192.0, scaler=dict(init_scale=4.0)), dict(loss_scale='auto'),
                dict(loss_scale='dynamic', scaler=dict(scale=4.0))):
        with pytest.raises(ValueError):
            Trainer(model, use_graph=False, **bad)
    tr = Trainer.from_cfg(fp.default_cfg(48, image_size=(W, H), num_sup=S), model, use_graph=False, max_grad_norm=2.0,
                          loss_scale='dynamic')
    assert tr.max_grad_norm == 2.0 and tr.dynamic_scale and tr.loss_scale == 65536.0
    assert tr.scaler_cfg == {'init_scale': 65536.0, 'growth_factor': 2.0, 'backoff_factor': 0.5, 'growth_interval': 2000}


def test_data_parallel_plans_clip_and_scale_single_rank(dev):
    """Clipping and the dynamic scale on the data-parallel plans (overlap, serial, eager hooks) with ONE rank over RCCL, in a
    child process (tests/_ddp_single_rank_clip.py; tests/test_model_gpu.py::test_ddp_path_single_rank_rccl says why)."""
    import os
    import subprocess
    import sys
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT='29519')
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), '_ddp_single_rank_clip.py')],
                       env=env, capture_output=True, text=True, timeout=900)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'DDP_CLIP_SINGLE_RANK_OK' in r.stdout
