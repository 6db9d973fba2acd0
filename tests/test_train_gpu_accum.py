"""Trainer(accum_steps=N): gradient accumulation over micro-batches on the MI355X.  The exact rule (the window's gradient is
((g1 + g2) + g3) * fl(1/3) bit for bit, nothing but the accumulation arena moves before the last call), the CPU oracle (a
torch loop that backpropagates loss_k / N and takes one Adam step), hipGraph replay without a capture per window position,
clipping and the dynamic fp16 scale once per window, window control, save -> resume inside a window, the data-parallel
plans with one rank over RCCL and with two ranks sharing the GPU, and default trainers that launch none of it.

Sizes and helpers are those of tests/test_train_gpu_clip.py.  'Deterministic' is model.set_deterministic(True): gradients are
then equal bit for bit from run to run and from Trainer to Trainer, which is what the bitwise assertions rest on."""
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import fami_pose_amd as fp
from oracle import model as om, ops as oops
from test_train_gpu_clip import S, H, W, B, _TorchTwin, _batch, _model, _norm_bound, _relerr, _trainer

pytestmark = pytest.mark.gpu
NAME = 'fami_accum_unscale_check_sumsq_f32'


def _batch_of(dev, seed, b):
    gen = torch.Generator().manual_seed(seed)
    kf, sup = torch.randn(b, 3, H, W, generator=gen), torch.randn(b, 3 * S, H, W, generator=gen)
    joints = torch.rand(b, 17, 2, generator=gen) * torch.tensor([W, H], dtype=torch.float32)
    vis = (torch.rand(b, 17, generator=gen) < 0.8).float()
    return tuple(t.to(dev) for t in (kf, sup, joints, vis))


def _gradient(tr, bt):
    """the gradient of one batch at tr's parameters: a direct _forward_backward call is a pure gradient computation"""
    kf, sup, joints, vis = bt
    tr._forward_backward(kf, sup, joints.float().contiguous(), vis.reshape(vis.shape[0], -1).float().contiguous())
    return tr.grad.detach().clone()


@pytest.mark.parametrize('use_graph', [False, True], ids=['eager', 'graph'])
@pytest.mark.parametrize('kind', ['adam', 'sgd'])
def test_exact_accumulation_rule(dev, use_graph, kind):
    kw = dict(lr=1e-3) if kind == 'adam' else dict(optimizer='sgd', lr=0.01, momentum=0.9, weight_decay=1e-4)
    bts = [_batch(dev, 9 + k) for k in range(3)]
    tr = _trainer(dev, use_graph, deterministic=True, accum_steps=3, **kw)
    assert tr.accum_steps == 3 and tr.accum is not None and tr.accum.shape == tr.grad.shape and tr._adam_split is None
    ref = _trainer(dev, False, deterministic=True, **kw)
    assert torch.equal(ref.flat, tr.flat)
    gs = [_gradient(ref, bt) for bt in bts]
    assert not torch.equal(gs[0], gs[1]) and not torch.equal(gs[1], gs[2])
    twin = _TorchTwin(tr)
    opt = (torch.optim.Adam(twin.params, lr=1e-3) if kind == 'adam' else
           torch.optim.SGD(twin.params, lr=0.01, momentum=0.9, weight_decay=1e-4))
    start = tr.flat.detach().clone()
    for k, bt in enumerate(bts):
        assert tr.window_position == k
        tr.step(*bt)
        if k < 2:
            assert torch.equal(tr.flat, start) and tr.opt.state[0].item() == 0.0
            assert torch.equal(tr.accum, gs[0] if k == 0 else gs[0] + gs[1])
    assert tr.window_position == 0 and tr.opt.state[0].item() == 1.0
    want = ((gs[0] + gs[1]) + gs[2]) * torch.tensor(1.0 / 3.0, dtype=torch.float32, device=dev)
    assert torch.equal(tr.grad, want)
    twin.clip(want, 1e30)              # (sets the twin's .grad; a coefficient clamped to 1.0 multiplies exactly)
    opt.step()
    e = _relerr(tr.flat.cpu(), twin.flat)
    print('%s parameters relerr %.3g' % (kind, e))
    assert e < 1e-6 and not torch.equal(tr.flat, start)
    if use_graph:
        assert len(tr._cache) == 1


def test_window_matches_the_cpu_oracle(dev):
    """N = 2, two different batches; the oracle backpropagates loss_k / 2, lets .grad accumulate and takes one Adam step"""
    from fami_pose_amd.train import Trainer
    orc = om.realistic_init_(om.AlignmentOracle(om.make_cfg(48), True, S, (H, W)), 5)
    model = fp.build_model(fp.default_cfg(48, image_size=(W, H), num_sup=S), 'train')
    model.load_state_dict(orc.state_dict())
    opt = torch.optim.Adam(orc.parameters(), lr=1e-3)
    p0 = orc.agg_final_layer.weight.data.clone()
    host = []
    for k in range(2):
        gen = torch.Generator().manual_seed(9 + k)
        kf, sup = torch.randn(B, 3, H, W, generator=gen), torch.randn(B, 3 * S, H, W, generator=gen)
        joints = torch.rand(B, 17, 2, generator=gen) * torch.tensor([W, H], dtype=torch.float32)
        vis = (torch.rand(B, 17, generator=gen) < 0.8).float()
        host.append((kf, sup, joints, vis))
    opt.zero_grad()
    losses = []
    for kf, sup, joints, vis in host:
        tg, tw = np.zeros((B, 17, H // 4, W // 4), np.float32), np.zeros((B, 17, 1), np.float32)
        for b in range(B):
            j3 = np.concatenate([joints[b].numpy(), np.zeros((17, 1), np.float32)], 1)
            v3 = np.repeat(vis[b].numpy()[:, None], 3, 1)
            tg[b], tw[b] = oops.generate_heatmaps(j3, v3, 3, np.array([W, H]), np.array([W // 4, H // 4]), 17)
        f0, k0, mi0 = orc(kf, sup)
        loss = oops.total_loss(f0, torch.from_numpy(tg), torch.from_numpy(tw), mi0)
        (loss / 2).backward()
        losses.append(loss.item())
    g_ref = orc.agg_final_layer.weight.grad.clone()
    opt.step()

    tr = Trainer(model.to(dev), lr=1e-3, use_graph=False, targets_from_joints=True, accum_steps=2)
    for k, bt in enumerate(host):
        tr.step(*(t.to(dev) for t in bt))
        assert tr.loss_value() == pytest.approx(losses[k], rel=1e-4)          # 'of the last call'
    print('window loss %.7g, oracle %.7g' % (tr.window_loss_value(), sum(losses) / 2))
    assert tr.window_loss_value() == pytest.approx(sum(losses) / 2, rel=1e-4)
    g1 = tr.views[id(model.agg_final_layer.weight)].cpu()
    e_g = ((g1 - g_ref).abs().max() / g_ref.abs().max()).item()
    p1 = model.agg_final_layer.weight.data.cpu()
    big = g_ref.abs() > 1e-3 * g_ref.abs().max()
    e_p = ((p1 - orc.agg_final_layer.weight.data)[big]).abs().max().item()
    e_rm = (orc.hrnet.bn1.running_mean - model.hrnet.bn1.running_mean.cpu()).abs().max().item()
    print('gradient relerr %.3g  parameter delta %.3g  running_mean %.3g' % (e_g, e_p, e_rm))
    assert e_g < 1e-3 and e_p < 1e-5 and e_rm < 1e-5
    assert not torch.equal(p1, p0)


def test_same_batch_twice_is_the_one_step_update(dev):
    """N = 2 on one batch: g + g and the multiplication by 1/2 are exact, so gradient and parameter arenas are those of a
    default Trainer after one step on that batch, bit for bit"""
    bt = _batch(dev)
    one = _trainer(dev, True, deterministic=True, lr=1e-3)
    one.step(*bt)
    two = _trainer(dev, True, deterministic=True, lr=1e-3, accum_steps=2)
    two.step(*bt)
    two.step(*bt)
    assert torch.equal(two.grad, one.grad) and torch.equal(two.flat, one.flat)
    assert torch.equal(two.opt.m, one.opt.m) and torch.equal(two.opt.v, one.opt.v)
    assert two.window_loss_value() == pytest.approx(one.loss_value(), rel=1e-6)


def test_graph_mode_never_captures_for_a_window_position(dev):
    """three windows of N = 2 over two batch shapes; B = 1 is first seen at window position 1"""
    seq = [_batch_of(dev, 20, 2), _batch_of(dev, 21, 1), _batch_of(dev, 22, 2), _batch_of(dev, 23, 2),
           _batch_of(dev, 24, 1), _batch_of(dev, 25, 2)]
    g = _trainer(dev, True, deterministic=True, lr=1e-3, accum_steps=2)
    e = _trainer(dev, False, deterministic=True, lr=1e-3, accum_steps=2)
    plans, tail = {}, None
    for k, bt in enumerate(seq):
        if k == 3:                       # inside the second window: acts at that window's update, no re-capture
            g.opt.set_lr(3e-4)
            e.opt.set_lr(3e-4)
        g.step(*bt)
        e.step(*bt)
        assert g.window_position == e.window_position == (k + 1) % 2
        assert len(g._cache) == (1 if k == 0 else 2)
        for key, entry in g._cache.items():
            assert plans.setdefault(key, entry[0]) is entry[0]
        tail = tail or g._tail[0]
        assert g._tail[0] is tail
        assert torch.equal(g.grad, e.grad) and torch.equal(g.accum, e.accum), k
        assert torch.equal(g.flat, e.flat), k
        assert torch.equal(g.model.hrnet.bn1.running_mean, e.model.hrnet.bn1.running_mean)
    assert g.opt.state[0].item() == 3.0 and g.opt.state[1].item() == pytest.approx(3e-4)
    assert g.plan_summary()['graphs'] == 1 and g.window_loss_value() == pytest.approx(e.window_loss_value(), rel=1e-6)


def test_clipping_once_per_window(dev):
    tr = _trainer(dev, True, lr=1e-3, max_grad_norm=1e9, accum_steps=2)
    twin = _TorchTwin(tr)
    opt = torch.optim.Adam(twin.params, lr=1e-3)
    bts = [_batch(dev, 9), _batch(dev, 10)]
    max_norm, coefs = 1e9, []
    for w in range(3):
        before = tr.clip.detach().clone()
        tr.step(*bts[0])
        assert torch.equal(tr.clip, before)                  # no coefficient on a non-closing call
        tr.step(*bts[1])
        want = tr.grad.detach().cpu().double().norm().item()         # grad: the window's mean gradient, before clipping
        got = tr.grad_norm()
        err = abs(got - want) / want
        print('window %d: grad_norm %.9g  float64 %.9g  relative error %.3g  bound %.3g  coef %.6g' %
              (w, got, want, err, _norm_bound(tr.grad), tr.clip_coef()))
        assert err <= _norm_bound(tr.grad)
        coefs.append(tr.clip_coef())
        assert coefs[-1] == pytest.approx(min(1.0, max_norm / (got + 1e-6)), rel=1e-6)
        twin.clip(tr.grad, max_norm)
        opt.step()
        if w == 0:
            max_norm = 0.1 * got
            tr.set_max_grad_norm(max_norm)
    assert coefs[0] == 1.0 and min(coefs[1:]) < 1.0          # clipping was active
    e = _relerr(tr.flat.cpu(), twin.flat)
    print('parameters relerr %.3g' % e)
    assert e < 1e-6 and tr.skipped_steps() == 0 and tr.opt.state[0].item() == 3.0 and len(tr._cache) == 1


def test_dynamic_scale_moves_once_per_window(dev):
    """fp16, init_scale 2^40 (tests/test_train_gpu_clip.py derives why it overflows), N = 2: a window whose sum holds inf / NaN
    is skipped and counted ONCE and the scale backs off once; windows until one is applied: skipped windows == halvings"""
    init = 2.0 ** 40
    tr = _trainer(dev, True, mode='f16', loss_scale='dynamic', scaler=dict(init_scale=init, growth_interval=1000), accum_steps=2)
    bts = [_batch(dev, 9), _batch(dev, 10)]
    before = tr.flat.detach().clone()
    tr.step(*bts[0])
    assert tr.loss_scale_value() == init and tr.skipped_steps() == 0          # nothing moves inside a window
    tr.step(*bts[1])
    assert tr.skipped_steps() == 1 and tr.loss_scale_value() == init * 0.5 and torch.equal(tr.flat, before)
    halvings, scale = 1, init * 0.5
    for w in range(int(math.log2(init)) + 1):
        tr.step(*bts[0])
        tr.step(*bts[1])
        if tr.skipped_steps() == halvings:
            assert tr.loss_scale_value() == scale and not torch.equal(tr.flat, before)
            break
        halvings += 1
        assert tr.skipped_steps() == halvings and tr.loss_scale_value() == scale / 2 and torch.equal(tr.flat, before)
        scale /= 2
    else:
        pytest.fail('no window was applied within log2(init_scale) + 1 windows')
    print('first applied window at scale 2^%d after %d halvings' % (int(math.log2(scale)), halvings))
    assert tr.opt.state[0].item() == 1.0 and tr.scaler_state[2].item() == 1.0 and torch.isfinite(tr.flat).all()
    assert len(tr._cache) == 1


def test_dynamic_scale_equals_static_at_a_fixed_power_of_two_with_accumulation(dev):
    bts = [_batch(dev, 9 + k) for k in range(4)]
    a = _trainer(dev, True, deterministic=True, mode='f16', loss_scale=8192.0, accum_steps=2)
    b = _trainer(dev, True, deterministic=True, mode='f16', loss_scale='dynamic', accum_steps=2,
                 scaler=dict(init_scale=8192.0, growth_interval=10 ** 9))
    for bt in bts:
        a.step(*bt)
        b.step(*bt)
        assert torch.equal(a.grad, b.grad) and torch.equal(a.flat, b.flat)
    assert a.skipped_steps() == b.skipped_steps() == 0 and a.opt.state[0].item() == 2.0
    assert b.scaler_state[2].item() == 2.0                   # the growth tracker counts windows


def test_reset_window_and_window_position(dev):
    bts = [_batch(dev, 9 + k) for k in range(3)]
    a = _trainer(dev, False, deterministic=True, lr=1e-3, accum_steps=2)
    assert a.window_position == 0 and a.window_loss_value() is not None
    a.step(*bts[0])
    assert a.window_position == 1
    a.reset_window()
    assert a.window_position == 0
    a.step(*bts[1])
    assert a.window_position == 1
    a.step(*bts[2])
    assert a.window_position == 0
    b = _trainer(dev, False, deterministic=True, lr=1e-3, accum_steps=2)
    b.step(*bts[1])
    b.step(*bts[2])
    assert torch.equal(a.grad, b.grad) and torch.equal(a.flat, b.flat) and a.opt.state[0].item() == 1.0
    assert a.window_loss_value() == b.window_loss_value()


@pytest.mark.parametrize('steps', [None, 1])
def test_default_trainers_launch_none_of_it(dev, steps, monkeypatch):
    from fami_pose_amd._lib import lib
    tr = _trainer(dev, False, accum_steps=steps)
    assert tr.accum_steps == 1 and tr.accum is None and tr._window_loss is None and tr._adam_split is not None
    assert tr.window_loss_value() is None
    names = []
    L = lib()
    call, call_routed = L.call, L.call_routed
    monkeypatch.setattr(L, 'call', lambda name, *a: (names.append(name), call(name, *a))[1])
    monkeypatch.setattr(L, 'call_routed', lambda route, name, *a: (names.append(name), call_routed(route, name, *a))[1])
    tr.step(*_batch(dev))
    torch.cuda.synchronize(dev)
    assert len(names) > 100 and 'fami_adam_f32' in names and NAME not in names
    assert tr.opt.state[0].item() == 1.0 and tr.window_position == 0
    # ... and an accumulating one launches it exactly once per window
    names.clear()
    acc = _trainer(dev, False, accum_steps=2)
    acc.step(*_batch(dev))
    assert NAME not in names and 'fami_adam_f32' not in names
    acc.step(*_batch(dev))
    assert names.count(NAME) == 1 and names.count('fami_adam_f32') == 1


def test_argument_checks(dev):
    from fami_pose_amd.train import Trainer
    model = _model().to(dev)
    for bad in (0, -1, 2.5, True, '2'):
        with pytest.raises(ValueError):
            Trainer(model, use_graph=False, accum_steps=bad)
    tr = Trainer.from_cfg(fp.default_cfg(48, image_size=(W, H), num_sup=S), model, use_graph=False, accum_steps=4)
    assert tr.accum_steps == 4 and tr.accum is not None


def test_resume_inside_a_window_continues_bitwise(dev, tmp_path):
    """save at position 1, resume into a FRESH graph-mode Trainer (whose first call therefore captures at position 1): this
    window's update and the next one's are those of the uninterrupted run"""
    from fami_pose_amd import checkpoint as ck
    bts = [_batch(dev, 9 + k) for k in range(4)]
    kw = dict(deterministic=True, lr=1e-3, max_grad_norm=1.0, accum_steps=2)
    full = _trainer(dev, True, **kw)
    after = []
    for k, bt in enumerate(bts):
        full.step(*bt)
        if k % 2 == 1:
            after.append((full.flat.detach().clone(), full.window_loss_value(), full.grad_norm()))
    part = _trainer(dev, True, **kw)
    part.step(*bts[0])
    path = ck.save_checkpoint(0, str(tmp_path), part.model, part)
    saved = torch.load(path, map_location='cpu')
    assert sorted(saved) == ['begin_epoch', 'grad_accum', 'optimizer', 'state_dict']
    assert saved['grad_accum']['steps'] == 2 and saved['grad_accum']['position'] == 1
    assert torch.equal(saved['grad_accum']['arena'], part.accum.cpu())
    res = _trainer(dev, True, **kw)
    ck.resume(res.model, res, path)
    assert res.window_position == 1 and torch.equal(res.accum, part.accum)
    res.step(*bts[1])
    assert torch.equal(res.flat, after[0][0]) and res.window_loss_value() == after[0][1] and res.grad_norm() == after[0][2]
    res.step(*bts[2])
    res.step(*bts[3])
    assert torch.equal(res.flat, after[1][0]) and res.window_loss_value() == after[1][1] and res.grad_norm() == after[1][2]
    assert torch.equal(res.opt.m, full.opt.m) and torch.equal(res.opt.v, full.opt.v)
    with pytest.raises(ValueError):
        other = _trainer(dev, False, accum_steps=3)
        ck.resume(other.model, other, path)
    # without accumulation: today's keys
    plain = _trainer(dev, False)
    out = ck.save_checkpoint(1, str(tmp_path / 'plain'), plain.model, plain)
    assert sorted(torch.load(out, map_location='cpu')) == ['begin_epoch', 'optimizer', 'state_dict']


def test_data_parallel_plans_accumulate_single_rank(dev):
    """The three data-parallel plans with ONE rank over RCCL, in a child process (tests/_ddp_single_rank_accum.py;
    tests/test_model_gpu.py::test_ddp_path_single_rank_rccl says why a child)."""
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT='29521')
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), '_ddp_single_rank_accum.py')],
                       env=env, capture_output=True, text=True, timeout=900)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'DDP_ACCUM_SINGLE_RANK_OK' in r.stdout


# ---- two ranks sharing the one GPU (gloo), the pattern of tests/test_ddp_gpu.py
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    try:
        os.environ['MASTER_ADDR'] = '127.0.0.1'
        os.environ['MASTER_PORT'] = str(port)
        os.environ.setdefault('HIP_FORCE_DEV_KERNARG', '1')
        os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
        os.environ.pop('FAMI_DDP_ALGO', None)
        import torch.distributed as dist
        from fami_pose_amd.train import Trainer
        dev = torch.device('cuda:0')
        dist.init_process_group('gloo', rank=rank, world_size=world)
        h, w = 96, 64

        def gather(t):
            out = [torch.empty_like(t.cpu()) for _ in range(world)]
            dist.all_gather(out, t.cpu().contiguous())
            return out

        sd = om.realistic_init_(om.AlignmentOracle(om.make_cfg(48), True, S, (h, w)), 5).state_dict()

        def model():
            m = fp.build_model(fp.default_cfg(48, image_size=(w, h), num_sup=S), 'train')
            m.load_state_dict(sd)
            return m.to(dev).set_deterministic(True)

        def batch(seed):
            gen = torch.Generator().manual_seed(seed)
            kf, sup = torch.randn(B, 3, h, w, generator=gen).to(dev), torch.randn(B, 3 * S, h, w, generator=gen).to(dev)
            joints = (torch.rand(B, 17, 2, generator=gen) * torch.tensor([w, h], dtype=torch.float32)).to(dev)
            return kf, sup, joints, (torch.rand(B, 17, generator=gen) < 0.8).float().to(dev)
        shard = [batch(100 + 10 * k + rank) for k in range(2)]          # this rank's two micro-batches

        # the window mean of a single-process accumulating trainer on this rank's shard
        tr_a = Trainer(model(), use_graph=False, targets_from_joints=True, data_parallel=False, accum_steps=2)
        assert not tr_a.ddp
        for bt in shard:
            tr_a.step(*bt)
        both = gather(tr_a.grad)
        mean = (both[0] + both[1]) * 0.5
        assert not torch.equal(both[0], both[1])

        # two ranks, eager: no exchange before the last micro-batch, then every bucket once
        tr_b = Trainer(model(), use_graph=False, targets_from_joints=True, bucket_mb=8, accum_steps=2)
        assert tr_b.ddp and tr_b.world == world
        calls, inner = [], tr_b.reducer.allreduce
        tr_b.reducer.allreduce = lambda lo, hi: (calls.append((lo, hi)), inner(lo, hi))[1]
        start = tr_b.flat.detach().clone()
        tr_b.step(*shard[0])
        assert calls == [] and torch.equal(tr_b.flat, start)
        tr_b.step(*shard[1])
        assert sorted(calls) == sorted(tr_b.reducer.ranges())
        assert torch.equal(tr_b.grad.cpu(), mean), 'exchanged gradients are not the mean over ranks of the window means'
        ps = gather(tr_b.flat)
        assert torch.equal(ps[0], ps[1]) and not torch.equal(tr_b.flat, start)
        # the overlap graph plan takes the same serial tail
        os.environ['FAMI_DDP_PLAN'] = 'overlap'
        tr_c = Trainer(model(), use_graph=True, targets_from_joints=True, bucket_mb=8, accum_steps=2)
        for bt in shard:
            tr_c.step(*bt)
        assert torch.equal(tr_c.grad.cpu(), mean) and torch.equal(tr_c.flat, tr_b.flat)
        torch.cuda.synchronize()
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, 'ok'))
    except Exception as e:       # noqa: BLE001 -- reported to the parent
        import traceback
        q.put((rank, 'FAILED: %s\n%s' % (e, traceback.format_exc())))


def test_two_ranks_on_one_gpu_exchange_the_window_mean(dev):
    """each rank's exchanged gradient is the mean over ranks of the per-rank window means of single-process trainers on the
    shards -- bitwise, as tests/test_ddp_gpu.py holds the non-accumulating exchange (a two-term sum is order independent and
    the factors are powers of two)"""
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    for _ in procs:
        r, msg = q.get(timeout=900)
        res[r] = msg
    for p in procs:
        p.join(60)
    assert res == {0: 'ok', 1: 'ok'}, res
