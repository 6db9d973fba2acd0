"""fami_sgd_f32 / FlatSGD against torch.optim.SGD (posetimation/optimizer/optimizer.py:58-64) on the MI355X: every valid
momentum / nesterov / dampening / weight-decay combination over a length with a scalar tail, sub-ranges with unaligned
bounds (the Trainer's in-backward split), arenas of different alignment, and the checked step of the fp16 overflow
guard."""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

N = 1003


def relerr(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


_COMBOS = [(m, nv, d, wd) for m in (0.0, 0.9) for nv in (False, True) for d in (0.0, 0.1) for wd in (0.0, 1e-4)
           if not (nv and (m == 0.0 or d != 0.0))]


@pytest.mark.parametrize('momentum,nesterov,dampening,wd', _COMBOS)
def test_sgd_matches_torch(dev, momentum, nesterov, dampening, wd):
    from fami_pose_amd.train import FlatSGD
    torch.manual_seed(11)
    p = torch.randn(N)
    ref = nn.Parameter(p.clone())
    opt = torch.optim.SGD([ref], lr=0.05, momentum=momentum, dampening=dampening, weight_decay=wd, nesterov=nesterov)
    flat = p.clone().to(dev)
    o = FlatSGD(flat, lr=0.05, momentum=momentum, dampening=dampening, weight_decay=wd, nesterov=nesterov)
    assert (o.buf is None) == (momentum == 0.0)
    for it in range(10):
        g = torch.randn(N)
        ref.grad = g.clone()
        opt.step()
        o.grad.copy_(g.to(dev))
        o.step()
    assert relerr(flat, ref.data) < 1e-6
    if momentum:
        assert relerr(o.buf, opt.state[ref]['momentum_buffer']) < 1e-6


@pytest.mark.parametrize('lo,hi', [(5, 998), (1, 2), (3, 1003), (0, 7)])
def test_sgd_sub_range_with_unaligned_bounds(dev, lo, hi):
    """prep once, then apply(lo, hi): only arena[lo:hi] moves, exactly like torch's SGD on that slice"""
    from fami_pose_amd.train import FlatSGD
    torch.manual_seed(12)
    p = torch.randn(N)
    ref = nn.Parameter(p[lo:hi].clone())
    opt = torch.optim.SGD([ref], lr=0.05, momentum=0.9, weight_decay=1e-4, nesterov=True)
    flat = p.clone().to(dev)
    o = FlatSGD(flat, lr=0.05, momentum=0.9, weight_decay=1e-4, nesterov=True)
    for it in range(10):
        g = torch.randn(N)
        ref.grad = g[lo:hi].clone()
        opt.step()
        o.grad.copy_(g.to(dev))
        o.prep()
        o.apply(lo, hi)
    out = flat.cpu()
    assert relerr(out[lo:hi], ref.data) < 1e-6
    assert torch.equal(out[:lo], p[:lo]) and torch.equal(out[hi:], p[hi:])
    assert not o.buf[:lo].any() and not o.buf[hi:].any()


def test_sgd_arenas_of_different_alignment(dev):
    """p, g and buf at different 16-byte phases: every element takes the kernel's scalar path"""
    from fami_pose_amd._lib import lib
    torch.manual_seed(13)
    p = torch.randn(N)
    ref = nn.Parameter(p.clone())
    opt = torch.optim.SGD([ref], lr=0.05, momentum=0.9, dampening=0.1, weight_decay=1e-4)
    pa, ga, ba = (torch.zeros(N + 4, device=dev) for _ in range(3))
    pa[1:1 + N].copy_(p.to(dev))
    state = torch.tensor([0.0, 0.05, 1.0], device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    for it in range(10):
        g = torch.randn(N)
        ref.grad = g.clone()
        opt.step()
        ga[2:2 + N].copy_(g.to(dev))
        lib().call('fami_sgd_prep_f32', state.data_ptr(), st)
        lib().call('fami_sgd_f32', pa[1:].data_ptr(), ga[2:].data_ptr(), ba[3:].data_ptr(), N, state.data_ptr(), 0.9,
                   0.1, 1e-4, 0, st)
    assert relerr(pa[1:1 + N], ref.data) < 1e-6
    assert pa[0].item() == 0 and not pa[1 + N:].any() and not ba[:3].any() and ba[3 + N:].numel() == 1 and ba[3 + N].item() == 0


def test_sgd_skips_a_step_with_nonfinite_gradients(dev):
    """The checked step of the static loss scale (fp16): a step whose gradients hold inf / NaN leaves parameters, the
    momentum buffer and the step count untouched, clears the flag and counts the skip in flag[1]; the run then equals
    torch's SGD that never saw the bad steps -- the very first step skipped included (the buffer's first-step rule
    waits for the first step that runs)."""
    from fami_pose_amd._lib import lib
    from fami_pose_amd.train import FlatSGD
    torch.manual_seed(14)
    p = torch.randn(N)
    ref = nn.Parameter(p.clone())
    opt = torch.optim.SGD([ref], lr=0.05, momentum=0.9, weight_decay=1e-4)
    flat = p.clone().to(dev)
    o = FlatSGD(flat, lr=0.05, momentum=0.9, weight_decay=1e-4)
    flag = torch.zeros(2, dtype=torch.int32, device=dev)      # {raised, skipped steps}
    st = torch.cuda.current_stream(dev).cuda_stream
    scale = 8192.0
    for it in range(6):
        g = torch.randn(N)
        bad = it in (0, 4)
        gd = (g * scale).to(dev)
        if bad:
            gd[(17, 1002)[it == 4]] = float('inf') if it == 0 else float('nan')
        else:
            ref.grad = g.clone()
            opt.step()
        o.grad.copy_(gd)
        before = (flat.clone(), o.buf.clone(), o.state[0].item())
        lib().call('fami_unscale_check_f32', o.grad.data_ptr(), o.grad.numel(), 1.0 / scale, flag.data_ptr(), st)
        assert flag[0].item() == (1 if bad else 0)
        o.step(flag)
        assert flag[0].item() == 0
        if bad:
            assert torch.equal(flat, before[0]) and torch.equal(o.buf, before[1]) and o.state[0].item() == before[2]
    assert o.state[0].item() == 4.0 and flag[1].item() == 2
    assert relerr(flat, ref.data) < 1e-6
