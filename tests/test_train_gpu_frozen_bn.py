"""Trainer(frozen_bn=...) on the GPU: a step with frozen BatchNorm statistics against the CPU oracle with the same BatchNorms
in eval mode (the reduced model and input size of test_model_gpu.py::test_model_vs_oracle), the launch content of such a
step, graph replay against eager launches, and the bf16 mode."""
import copy
import warnings

import numpy as np
import pytest
import torch

import fami_pose_amd as fp
from oracle import model as om, ops as oops

pytestmark = pytest.mark.gpu
warnings.filterwarnings('ignore')
HM_TOL = 1e-3
S, H, W, B = 2, 192, 128, 2           # test_model_vs_oracle's first case
LR = 1e-3


def _argmax(hm):
    return hm.reshape(hm.shape[0], hm.shape[1], -1).argmax(2).cpu().numpy()


def _pair(seed=5):
    orc = om.realistic_init_(om.AlignmentOracle(om.make_cfg(48), True, S, (H, W)), seed)
    gen = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():                 # statistics a pretrained model would carry: away from (0, 1), so using them shows
        for m in orc.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=gen) * 0.05)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=gen) * 0.5 + 0.75)
    model = fp.build_model(fp.default_cfg(48, image_size=(W, H), num_sup=S), 'train')
    model.load_state_dict(orc.state_dict())
    return model, orc


def _batch():
    # The argmax of a heatmap is only defined up to the error of the arithmetic: where the reference's two largest values of a map
    # are closer than its own fp32 evaluation is to its fp64 one, "the same argmax" is a coin toss between two correct
    # implementations (seed 52, test_model_vs_oracle's, has such a map with the backbone frozen: top two 3.6e-7 apart where the
    # fp32 oracle is 1.2e-4 from fp64 behind the head's train-mode BatchNorms).  The batch is the first seed from 52 up for which,
    # in both scopes and for every map of both outputs, the fp32 oracle's top-two margin exceeds 4x its distance from the fp64
    # oracle on that output (52: no, 53: no, 54: yes) -- a property of the reference alone, asserted in _oracle.
    gen = torch.Generator().manual_seed(54)
    kf, sup = torch.randn(B, 3, H, W, generator=gen), torch.randn(B, 3 * S, H, W, generator=gen)
    tgt = torch.rand(B, 17, H // 4, W // 4, generator=gen)
    w = (torch.rand(B, 17, 1, generator=gen) < 0.8).float()
    return kf, sup, tgt, w


def _freeze_oracle(orc, prefix):
    names = []
    for n, m in orc.named_modules():
        if isinstance(m, torch.nn.BatchNorm2d) and n.startswith(prefix):
            m.eval()
            names.append(n)
    return names


_ORACLE = {}


def _oracle(scope):
    """One oracle evaluation per scope for the whole module (fp32 step with torch.optim.Adam, and the fp64 gradients that
    arbitrate): computed once, never modified afterwards."""
    if scope not in _ORACLE:
        torch.set_num_threads(min(16, torch.get_num_threads()))
        _, orc = _pair()
        frozen = _freeze_oracle(orc, '' if scope == 'all' else 'hrnet.')
        kf, sup, tgt, w = _batch()
        start = {k: v.clone() for k, v in orc.state_dict().items()}
        orc64 = copy.deepcopy(orc).double()
        opt = torch.optim.Adam(orc.parameters(), lr=LR)
        opt.zero_grad()
        f0, k0, mi0 = orc(kf, sup)
        l0 = oops.total_loss(f0, tgt, w, mi0)
        l0.backward()
        grads = {k: p.grad.clone() for k, p in orc.named_parameters() if p.grad is not None}
        opt.step()
        after = {k: p.detach().clone() for k, p in orc.named_parameters()}
        f64, k64, mi64 = orc64(kf.double(), sup.double())
        for fp32, fp64 in ((f0, f64), (k0, k64)):
            top = fp32.detach().reshape(B * 17, -1).topk(2, dim=1).values
            assert (top[:, 0] - top[:, 1]).min().item() > 4 * (fp32.detach().double() - fp64.detach()).abs().max().item()
        oops.total_loss(f64, tgt.double(), w.double(), mi64).backward()
        g64 = {k: p.grad.clone() for k, p in orc64.named_parameters() if p.grad is not None}
        _ORACLE[scope] = dict(frozen=frozen, start=start, f0=f0.detach(), k0=k0.detach(), l0=l0.item(), grads=grads, after=after,
                              g64=g64, f64=f64.detach(), buffers={k: v.clone() for k, v in orc.state_dict().items()
                                                                 if 'running' in k or 'num_batches' in k})
    return _ORACLE[scope]


def _check_step_against_oracle(dev, scope):
    from fami_pose_amd.train import Trainer
    o = _oracle(scope)
    model, _ = _pair()
    model = model.to(dev)
    tr = Trainer(model, lr=LR, use_graph=False, frozen_bn=scope)
    assert tr.frozen_bn_names() == o['frozen'] and len(o['frozen']) > 100
    kf, sup, tgt, w = _batch()
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    outs = tr.step(kf.to(dev), sup.to(dev), tgt.to(dev), w.to(dev))
    f1, k1 = outs[0].detach().cpu(), outs[1].detach().cpu()
    e_f, e_k = (f1 - o['f0']).abs().max().item(), (k1 - o['k0']).abs().max().item()
    print('frozen_bn=%s: |final_hm - oracle| %.3e |kf_hm - oracle| %.3e loss %.8f vs %.8f' % (scope, e_f, e_k, tr.loss_value(), o['l0']))
    assert e_f < HM_TOL and e_k < HM_TOL
    assert np.array_equal(_argmax(f1), _argmax(o['f0'])) and np.array_equal(_argmax(k1), _argmax(o['k0']))
    assert tr.loss_value() == pytest.approx(o['l0'], rel=1e-4)
    # gradients: the acceptance rule of test_model_vs_oracle (fp64 arbitrates)
    mine = dict(model.named_parameters())
    bad, e_cpus, e_hips = [], [], []
    for name, g64 in o['g64'].items():
        s64 = g64.abs().max().item()
        if s64 < 1e-9:
            continue
        e_cpu = (o['grads'][name].double() - g64).abs().max().item() / s64
        e_hip = (tr.views[id(mine[name])].cpu().double() - g64).abs().max().item() / s64
        e_cpus.append(e_cpu)
        e_hips.append(e_hip)
        if e_hip > max(0.25, 2 * e_cpu):
            bad.append((name, e_hip, e_cpu))
    print('frozen_bn=%s gradients vs fp64: HIP median %.3e p90 %.3e max %.3e | CPU fp32 median %.3e p90 %.3e max %.3e' %
          (scope, np.median(e_hips), np.percentile(e_hips, 90), max(e_hips), np.median(e_cpus), np.percentile(e_cpus, 90), max(e_cpus)))
    assert len(e_hips) > 900 and not bad, bad[:20]
    assert np.median(e_hips) <= 3 * np.median(e_cpus) + 1e-4, (np.median(e_hips), np.median(e_cpus))
    assert np.percentile(e_hips, 90) <= 3 * np.percentile(e_cpus, 90) + 1e-4
    # Adam's first step is lr * g / (|g| + eps), i.e. lr * sign(g) wherever |g| >> eps = 1e-8.
    # (a) test_trainer_step_matches_oracle_adam's own comparison: the output layer's weight, where its gradient is above 1e-3 of
    #     its maximum.
    # (b) every parameter, where the sign of the gradient is DETERMINED: the rule asserted above lets a correct fp32 gradient be
    #     max(0.25, 2 e_cpu) * max|g64| away from the fp64 one (behind train-mode BatchNorms the fp32 oracle itself is 1e-2 of the
    #     maximum off, so a smaller element can have either sign in two correct implementations and the updates then differ by
    #     2 lr); above that bound the oracle's sign and any accepted gradient's sign are the fp64 sign.  |g| > 1e3 * eps as well:
    #     the update's sensitivity to a relative gradient error d is lr * eps * d / |g|, invisible at 1e-5 from there up.
    g = o['grads']['agg_final_layer.weight']
    big = g.abs() > 1e-3 * g.abs().max()
    head = (mine['agg_final_layer.weight'].detach().cpu() - o['after']['agg_final_layer.weight'])[big].abs().max().item()
    worst, compared = 0.0, 0
    for name, p in mine.items():
        if name not in o['g64']:
            continue
        g, g64 = o['grads'][name], o['g64'][name]
        s64 = g64.abs().max().item()
        e_cpu = (g.double() - g64).abs().max().item() / max(s64, 1e-30)
        sure = (g.abs() > max(0.25, 2 * e_cpu) * s64) & (g.abs() > 1e-5)
        if sure.any():
            compared += 1
            worst = max(worst, (p.detach().cpu() - o['after'][name])[sure].abs().max().item())
    print('frozen_bn=%s: largest Adam update difference: output layer %.3e, %d parameters %.3e' % (scope, head, compared, worst))
    assert head < 1e-5
    assert compared >= 0.5 * len(o['g64']) and worst < 1e-5
    return tr, model, sd0, (kf, sup, tgt, w)


def test_step_all_frozen_matches_oracle_in_eval(dev):
    tr, model, sd0, batch = _check_step_against_oracle(dev, 'all')
    tr.step(*[t.to(dev) for t in batch])
    torch.cuda.synchronize(dev)
    n = 0
    for k, v in model.state_dict().items():
        if 'running_' in k or 'num_batches_tracked' in k:
            assert torch.equal(v, sd0[k]), k
            n += 1
    assert n > 300


def test_step_backbone_frozen(dev):
    tr, model, sd0, batch = _check_step_against_oracle(dev, 'backbone')
    o = _oracle('backbone')
    moved = 0
    for k, v in model.state_dict().items():
        if 'running_' in k or 'num_batches_tracked' in k:
            if k.startswith('hrnet.'):
                assert torch.equal(v, sd0[k]), k
            else:
                assert not torch.equal(v, sd0[k]), k
                moved += 1
                if 'running_' in k:
                    assert (v.cpu() - o['buffers'][k]).abs().max().item() < 1e-5, k
                else:
                    assert int(v) == int(o['buffers'][k]), k
    assert moved > 10


TRAIN_ONLY = ('fami_bn_stats_', 'fami_bn_train_fwd', 'fami_bn_apply_slots_', 'fami_bn_bwd_', 'fami_bn_bwd2_',
              'fami_bn_bwd_apply_slots_', 'fami_bn_finalize_slots_f32', 'fami_bn_running_update', 'fami_conv2d_fwd_stats_',
              'fami_conv2d_dgrad_bnstats_')


def _small():
    s, h, w, b = 2, 128, 96, 2            # test_trainer_step_matches_oracle_adam's size: these tests need no CPU reference
    gen = torch.Generator().manual_seed(9)
    kf, sup = torch.randn(b, 3, h, w, generator=gen), torch.randn(b, 3 * s, h, w, generator=gen)
    tgt = torch.rand(b, 17, h // 4, w // 4, generator=gen)
    wt = (torch.rand(b, 17, 1, generator=gen) < 0.8).float()
    orc = om.realistic_init_(om.AlignmentOracle(om.make_cfg(48), True, s, (h, w)), 5)
    model = fp.build_model(fp.default_cfg(48, image_size=(w, h), num_sup=s), 'train')
    model.load_state_dict(orc.state_dict())
    return model, (kf, sup, tgt, wt)


@pytest.mark.parametrize('mode', [None, 'bf16'])
def test_launch_content_all_frozen(dev, mode):
    """No train-mode BatchNorm kernel, no statistics epilogue, and exactly one fami_bn_eval_bwd_* per BatchNorm call whose input
    or parameters need a gradient (every BatchNorm call of this model: all have trainable gamma / beta)."""
    from fami_pose_amd.train import Trainer
    from fami_pose_amd._lib import lib
    model, batch = _small()
    model = model.to(dev)
    if mode:
        model.set_compute_dtype(mode)
    tr = Trainer(model, lr=LR, use_graph=False, frozen_bn='all')
    L, log = lib(), []
    call, call_routed = L.call, L.call_routed
    L.call = lambda name, *a: (log.append(name), call(name, *a))[1]
    L.call_routed = lambda route, name, *a: (log.append(name), call_routed(route, name, *a))[1]
    try:
        tr.step(*[t.to(dev) for t in batch])
    finally:
        del L.call, L.call_routed
    torch.cuda.synchronize(dev)
    assert not sorted({n for n in log if n.startswith(TRAIN_ONLY)})
    fwd = sum(n == 'fami_bn_eval_stats_f32' for n in log)           # one per BatchNorm call of the forward pass
    bwd = sum(n.startswith('fami_bn_eval_bwd_') for n in log)
    nbn = sum(isinstance(m, torch.nn.BatchNorm2d) for m in model.modules())
    assert fwd >= nbn and bwd == fwd, (fwd, bwd, nbn)
    assert tr.last_nfused == {'fwd': 0, 'bwd': 0, 'xbn': 0}


def test_graph_replay_is_bitwise_eager_and_refreezing_recaptures(dev):
    from fami_pose_amd.train import Trainer, freeze_batchnorm
    res = {}
    for use_graph in (False, True):
        model, batch = _small()
        model = model.to(dev)
        model.set_deterministic(True)       # (the DCN input-gradient scatter is the one order-dependent sum of the step)
        tr = Trainer(model, lr=LR, use_graph=use_graph, frozen_bn='all')
        batch = [t.to(dev) for t in batch]
        outs = []
        for _ in range(2):
            o = tr.step(*batch)
            outs.append((o[0].clone(), tr.loss_parts.clone(), tr.flat.clone()))
        res[use_graph] = outs
        if use_graph:
            ncap = len(tr._cache)
            key = next(iter(tr._cache))
            plan = tr._cache[key][0]
            assert freeze_batchnorm(model, 'backbone')
            o = tr.step(*batch)
            assert tr._cache[key][0] is not plan and len(tr._cache) == ncap           # re-captured, not replayed
            third_b = (o[0].clone(), tr.flat.clone(), {k: v.clone() for k, v in model.state_dict().items() if 'running_mean' in k})
        else:
            freeze_batchnorm(model, 'backbone')
            o = tr.step(*batch)
            third_a = (o[0].clone(), tr.flat.clone(), {k: v.clone() for k, v in model.state_dict().items() if 'running_mean' in k})
    for a, b in zip(res[False], res[True]):
        for u, v in zip(a, b):
            assert torch.equal(u, v)
    # the third step ran with the head's BatchNorms on batch statistics again: its heatmaps differ from a frozen step's and are
    # the eager run's, bit for bit; the head's running statistics moved
    assert torch.equal(third_a[0], third_b[0]) and torch.equal(third_a[1], third_b[1])
    assert not torch.equal(third_b[0], res[True][1][0])
    head = [k for k in third_b[2] if not k.startswith('hrnet.')]
    assert head and all(torch.equal(third_a[2][k], third_b[2][k]) for k in third_b[2])
    model0, _ = _small()
    sd = model0.state_dict()
    assert all(not torch.equal(third_b[2][k].cpu(), sd[k]) for k in head)
    assert all(torch.equal(third_b[2][k].cpu(), sd[k]) for k in third_b[2] if k.startswith('hrnet.'))


def _half_emulation(orc, dtype):
    """test_model_gpu.py's: the oracle with every conv operand / conv output / BN output rounded to the 16-bit storage type"""
    emu = copy.deepcopy(orc)
    rb = lambda t: t.to(dtype).float()
    with torch.no_grad():
        for m in emu.modules():
            if isinstance(m, torch.nn.Conv2d):
                m.weight.copy_(rb(m.weight))
    for n, m in emu.named_modules():
        if isinstance(m, torch.nn.Conv2d):
            m.register_forward_pre_hook(lambda mod, inp: tuple(rb(i) for i in inp))
            if not n.endswith('final_layer'):
                m.register_forward_hook(lambda mod, inp, out: rb(out))
        elif isinstance(m, torch.nn.BatchNorm2d):
            m.register_forward_hook(lambda mod, inp, out: rb(out))
    return emu


def test_bf16_step_all_frozen(dev):
    """test_half_mode_vs_oracle's band against the oracle with eval-mode BatchNorm: the HIP path no further from the fp32 oracle
    than 1.5x a plain bf16 emulation of the same graph (relative RMS per output) plus 1e-2, the loss within 10 %."""
    from fami_pose_amd.train import Trainer
    o = _oracle('all')
    _, orc = _pair()
    _freeze_oracle(orc, '')
    kf, sup, tgt, w = _batch()
    emu = _half_emulation(orc, torch.bfloat16)
    with torch.no_grad():
        fe, ke, _ = emu(kf, sup)
    model, _ = _pair()
    model = model.to(dev).set_compute_dtype('bf16')
    tr = Trainer(model, lr=LR, use_graph=False, frozen_bn='all')
    sd0 = {k: v.clone() for k, v in model.state_dict().items() if 'running_' in k}
    outs = tr.step(kf.to(dev), sup.to(dev), tgt.to(dev), w.to(dev))
    rms = lambda a, b: ((a - b).norm() / b.norm()).item()
    for hip, emul, ref in ((outs[0], fe, o['f0']), (outs[1], ke, o['k0'])):
        e_hip, e_emu = rms(hip.detach().cpu().float(), ref), rms(emul, ref)
        print('bf16 frozen_bn=all: HIP rel RMS %.4f, CPU bf16 emulation %.4f' % (e_hip, e_emu))
        assert e_hip <= 1.5 * e_emu + 1e-2, (e_hip, e_emu)
    assert tr.loss_value() == pytest.approx(o['l0'], rel=0.1)
    assert torch.isfinite(tr.grad).all() and tr.grad.abs().max().item() > 0
    for k, v in model.state_dict().items():
        if 'running_' in k:
            assert torch.equal(v, sd0[k]), k
