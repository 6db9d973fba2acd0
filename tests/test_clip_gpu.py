"""Global-norm gradient clipping at kernel level on the MI355X: fami_sumsq_f32 / fami_unscale_check_sumsq_f32 /
fami_clip_coef_f32 against the float64 norm of the same data, and FlatAdam / FlatSGD with a device gradient multiplier
against torch.nn.utils.clip_grad_norm_ followed by torch.optim.Adam / SGD.

The error bound of the norm is derived, not tuned.  The kernel adds non-negative fp32 squares; k is its longest chain
of fp32 additions (csrc/optim.hip, sumsq_kernel): per lane ceil(ceil(n4 / parts) / 256) vectors (n4 = 16-byte vectors
of the aligned body, parts = fami_sumsq_parts() workgroups of 256 lanes), the four vector components pairwise (2), the
scalar head / tail element (1), wave_sum (6), the four waves through LDS pairwise (2); the partials are then summed in
double.  The sum of squares is off by at most (k + 1) 2^-24 relative (one rounding per square, k additions); the
square root halves that and rounds once: (k + 3) 2^-24 on the norm is the simpler, conservative bound asserted.
At the W48 arena length (64 655 204 elements) n4 = 16 163 801, each workgroup owns 7893 vectors, a lane adds 31 of
them: k = 31 + 11 = 42 and the bound is 45 * 2^-24 = 2.7e-6."""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

N = 1003
W48 = 64655204
BLOCK = 256
_COMBOS = [(m, nv, d, wd) for m in (0.0, 0.9) for nv in (False, True) for d in (0.0, 0.1) for wd in (0.0, 1e-4)
           if not (nv and (m == 0.0 or d != 0.0))]


def relerr(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def _st(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _parts():
    from fami_pose_amd._lib import lib
    return lib().cdll.fami_sumsq_parts()


def chain_length(t):
    """k of the module docstring for the device tensor t (its alignment decides head and body)"""
    parts, n = _parts(), t.numel()
    head = min(n, ((16 - t.data_ptr() % 16) % 16) // 4)
    n4 = (n - head) // 4
    chunk = -(-n4 // parts)
    return -(-chunk // BLOCK) + 2 + 1 + 6 + 2


def bound(t):
    return (chain_length(t) + 3) * 2.0 ** -24


def device_norm(t, dev, max_norm=1.0):
    """-> (total_norm, coef, partials, flag) of fami_sumsq_f32 + fami_clip_coef_f32 over the device tensor t"""
    from fami_pose_amd._lib import lib
    parts = torch.full((_parts(),), float('nan'), device=dev)        # every slot must be written
    clip = torch.zeros(2, device=dev)
    mx = torch.tensor([max_norm], device=dev)
    flag = torch.zeros(2, dtype=torch.int32, device=dev)
    lib().call('fami_sumsq_f32', t.data_ptr(), t.numel(), parts.data_ptr(), _st(dev))
    lib().call('fami_clip_coef_f32', parts.data_ptr(), parts.numel(), mx.data_ptr(), clip.data_ptr(), flag.data_ptr(), _st(dev))
    return clip[0].item(), clip[1].item(), parts, flag


def _check_norm(t, dev, max_norm=1.0):
    ref = t.detach().cpu().double().norm().item()
    norm, coef, parts, flag = device_norm(t, dev, max_norm)
    err = abs(norm - ref) / ref
    print('n %d  k %d  norm %.9g  float64 %.9g  relative error %.3g  bound %.3g' %
          (t.numel(), chain_length(t), norm, ref, err, bound(t)))
    assert err <= bound(t)
    assert flag[0].item() == 0 and torch.isfinite(parts).all()
    want = torch.tensor(max_norm, dtype=torch.float32) / (torch.tensor(norm, dtype=torch.float32) + 1e-6)
    assert coef == pytest.approx(min(1.0, want.item()), rel=2.0 ** -22)      # clip_grad_norm_'s rule, in fp32
    return norm


@pytest.mark.parametrize('n', [1, 3, 1003, 4098, 1 << 20])
def test_norm_matches_float64(dev, n):
    """lengths 1 and 3 (scalar path only), 1003 and 4098 (tails of 3 and 2 behind the 16-byte body), 2^20"""
    torch.manual_seed(21)
    _check_norm(torch.randn(n).to(dev), dev, max_norm=0.5)


@pytest.mark.parametrize('lo,hi', [(5, 998), (1, 2), (3, 1003), (0, 7)])
def test_norm_of_sub_range_with_unaligned_bounds(dev, lo, hi):
    torch.manual_seed(22)
    _check_norm(torch.randn(N).to(dev)[lo:hi], dev)


def test_norm_of_the_w48_arena_length(dev):
    """64 655 204 elements: k = 42, bound 2.7e-6; a design with k > 1024 here is rejected"""
    g = torch.empty(W48, device=dev).normal_(generator=torch.Generator(device=dev).manual_seed(23)).mul_(1e-3)
    assert chain_length(g) == 42 and chain_length(g) <= 1024
    _check_norm(g, dev, max_norm=1.0)


def test_norm_is_bitwise_reproducible(dev):
    """the same arena twice, and a fresh allocation at the same alignment: equal partials and norm bit for bit"""
    torch.manual_seed(24)
    h = torch.randn(3 * (1 << 20) + 5)
    a = h.to(dev)
    n1, _, p1, _ = device_norm(a, dev)
    n2, _, p2, _ = device_norm(a, dev)
    b = h.to(dev)
    assert b.data_ptr() != a.data_ptr() and b.data_ptr() % 16 == a.data_ptr() % 16
    n3, _, p3, _ = device_norm(b, dev)
    assert torch.equal(p1, p2) and torch.equal(p1, p3) and n1 == n2 == n3
    small = torch.randn(40).to(dev)
    _, _, ps, _ = device_norm(small, dev)
    assert ps[0].item() > 0 and not ps[10:].any()       # unused slots are written as 0


@pytest.mark.parametrize('n,off', [(1003, 0), (1003, 1), (1 << 20, 0), (5, 3)])
def test_fused_unscale_pass(dev, n, off):
    """fami_unscale_check_sumsq_f32 leaves the arena fami_unscale_check_f32 leaves (same f, fdev NULL), its norm obeys the
    bound against the unscaled data, and fdev = [2^-13] with f = 1 is the static pass with f = 2^-13 bit for bit"""
    from fami_pose_amd._lib import lib
    torch.manual_seed(25)
    h = torch.randn(n) * 8192.0
    f = 1.0 / 8192.0
    flag = torch.zeros(2, dtype=torch.int32, device=dev)
    base = torch.zeros(n + 4, device=dev)

    def arena():
        a = base.clone()[off:off + n]
        a.copy_(h.to(dev))
        return a
    a = arena()
    if off == 0:            # (the existing pass takes 16-byte aligned arenas only)
        lib().call('fami_unscale_check_f32', a.data_ptr(), n, f, flag.data_ptr(), _st(dev))
    else:
        a.mul_(f)
    parts = torch.full((_parts(),), float('nan'), device=dev)
    b = arena()
    lib().call('fami_unscale_check_sumsq_f32', b.data_ptr(), n, f, None, flag.data_ptr(), parts.data_ptr(), _st(dev))
    assert torch.equal(a, b) and flag[0].item() == 0
    clip = torch.zeros(2, device=dev)
    mx = torch.ones(1, device=dev)
    lib().call('fami_clip_coef_f32', parts.data_ptr(), parts.numel(), mx.data_ptr(), clip.data_ptr(), flag.data_ptr(), _st(dev))
    ref = b.cpu().double().norm().item()
    err = abs(clip[0].item() - ref) / ref
    print('fused n %d off %d: relative error %.3g  bound %.3g' % (n, off, err, bound(b)))
    assert err <= bound(b) and flag[0].item() == 0
    # device factor
    c = arena()
    fdev = torch.tensor([2.0 ** -13], device=dev)
    lib().call('fami_unscale_check_sumsq_f32', c.data_ptr(), n, 1.0, fdev.data_ptr(), flag.data_ptr(), None, _st(dev))
    assert torch.equal(a, c) and flag[0].item() == 0


@pytest.mark.parametrize('bad', [float('inf'), float('nan')])
def test_fused_pass_raises_the_flag(dev, bad):
    from fami_pose_amd._lib import lib
    torch.manual_seed(26)
    g = torch.randn(N).to(dev)
    g[1002 if bad != bad else 17] = bad
    flag = torch.zeros(2, dtype=torch.int32, device=dev)
    parts = torch.zeros(_parts(), device=dev)
    lib().call('fami_unscale_check_sumsq_f32', g.data_ptr(), N, 0.5, None, flag.data_ptr(), parts.data_ptr(), _st(dev))
    assert flag[0].item() == 1
    # ... and the coefficient kernel raises it for a non-finite norm on its own (torch's clip_grad_norm_ would not)
    flag.zero_()
    clip = torch.zeros(2, device=dev)
    mx = torch.ones(1, device=dev)
    lib().call('fami_clip_coef_f32', parts.data_ptr(), parts.numel(), mx.data_ptr(), clip.data_ptr(), flag.data_ptr(), _st(dev))
    assert flag[0].item() == 1 and clip[1].item() == 0.0 and not torch.isfinite(clip[0])


def _clipped_run(dev, make_ref, make_flat, steps=10, max_norm=20.0):
    """ten steps; gradient scales alternate so that some steps clip and some do not -> (flat optimizer, coefficients)"""
    from fami_pose_amd._lib import lib
    torch.manual_seed(27)
    p = torch.randn(N)
    ref = nn.Parameter(p.clone())
    opt = make_ref(ref)
    flat = p.clone().to(dev)
    o = make_flat(flat)
    clip = torch.zeros(2, device=dev)
    mx = torch.tensor([max_norm], device=dev)
    flag = torch.zeros(2, dtype=torch.int32, device=dev)
    parts = torch.zeros(_parts(), device=dev)
    o.set_grad_multiplier(clip[1:2])
    coefs = []
    for it in range(steps):
        g = torch.randn(N) * (3.0 if it % 3 == 0 else 0.2)        # norms ~95 and ~6.3 around max_norm 20
        ref.grad = g.clone()
        nn.utils.clip_grad_norm_([ref], max_norm)
        opt.step()
        o.grad.copy_(g.to(dev))
        lib().call('fami_sumsq_f32', o.grad.data_ptr(), N, parts.data_ptr(), _st(dev))
        lib().call('fami_clip_coef_f32', parts.data_ptr(), parts.numel(), mx.data_ptr(), clip.data_ptr(), flag.data_ptr(), _st(dev))
        o.step(flag)
        assert torch.equal(o.grad.cpu(), g)               # the gradient arena is not rewritten
        coefs.append(clip[1].item())
    assert flag[1].item() == 0
    return o, opt, ref, flat, coefs


def test_scaled_adam_matches_clip_grad_norm_then_torch_adam(dev):
    from fami_pose_amd.train import FlatAdam
    o, opt, ref, flat, coefs = _clipped_run(dev, lambda r: torch.optim.Adam([r], lr=0.01),
                                            lambda f: FlatAdam(f, lr=0.01))
    assert min(coefs) < 1.0 and max(coefs) == 1.0
    e = relerr(flat, ref.data)
    print('scaled adam relerr %.3g' % e)
    assert e < 1e-6
    assert relerr(o.m, opt.state[ref]['exp_avg']) < 1e-6
    # the kernel's (1 - beta2) is fp32 arithmetic, 1.f - 0.999f = 0.00100004673, where torch's is 0.001 in double: every
    # increment of the second moment is 4.7e-5 larger, with or without a gradient multiplier
    assert relerr(o.v, opt.state[ref]['exp_avg_sq']) < 5e-5


@pytest.mark.parametrize('momentum,nesterov,dampening,wd', _COMBOS)
def test_scaled_sgd_matches_clip_grad_norm_then_torch_sgd(dev, momentum, nesterov, dampening, wd):
    from fami_pose_amd.train import FlatSGD
    kw = dict(lr=0.05, momentum=momentum, dampening=dampening, weight_decay=wd, nesterov=nesterov)
    o, opt, ref, flat, coefs = _clipped_run(dev, lambda r: torch.optim.SGD([r], **kw), lambda f: FlatSGD(f, **kw))
    assert min(coefs) < 1.0 and max(coefs) == 1.0
    e = relerr(flat, ref.data)
    print('scaled sgd %s relerr %.3g' % (kw, e))
    assert e < 1e-6
    if momentum:
        assert relerr(o.buf, opt.state[ref]['momentum_buffer']) < 1e-6


@pytest.mark.parametrize('kind', ['adam', 'sgd', 'sgd_nesterov_wd'])
def test_multiplier_of_one_is_bitwise_the_plain_update(dev, kind):
    """every norm below max_norm: coef == 1.0f, and a multiplication by 1.0f is exact"""
    from fami_pose_amd._lib import lib
    from fami_pose_amd.train import FlatAdam, FlatSGD
    torch.manual_seed(28)
    p = torch.randn(N)
    make = {'adam': lambda f: FlatAdam(f, lr=0.01, weight_decay=1e-4),
            'sgd': lambda f: FlatSGD(f, lr=0.05, momentum=0.9, dampening=0.1, weight_decay=1e-4),
            'sgd_nesterov_wd': lambda f: FlatSGD(f, lr=0.05, momentum=0.9, weight_decay=1e-4, nesterov=True)}[kind]
    a, b = make(p.clone().to(dev)), make(p.clone().to(dev))
    clip = torch.zeros(2, device=dev)
    mx = torch.tensor([1e6], device=dev)
    flag = torch.zeros(2, dtype=torch.int32, device=dev)
    parts = torch.zeros(_parts(), device=dev)
    b.set_grad_multiplier(clip[1:2])
    for it in range(10):
        g = torch.randn(N).to(dev)
        a.grad.copy_(g)
        b.grad.copy_(g)
        a.step()
        lib().call('fami_sumsq_f32', b.grad.data_ptr(), N, parts.data_ptr(), _st(dev))
        lib().call('fami_clip_coef_f32', parts.data_ptr(), parts.numel(), mx.data_ptr(), clip.data_ptr(), flag.data_ptr(), _st(dev))
        assert clip[1].item() == 1.0
        b.step(flag)
    assert torch.equal(a.p, b.p)
    for x, y in zip(a.tensors(), b.tensors()):
        assert torch.equal(x, y)


@pytest.mark.parametrize('kind', ['adam', 'sgd'])
def test_nan_gradient_skips_the_clipped_step(dev, kind):
    """a NaN in the gradients makes the norm NaN: parameters and moments unchanged, step count not advanced, flag[1]
    incremented -- through fami_clip_coef_f32 alone (no unscale pass)"""
    from fami_pose_amd._lib import lib
    from fami_pose_amd.train import FlatAdam, FlatSGD
    torch.manual_seed(29)
    flat = torch.randn(N).to(dev)
    o = FlatAdam(flat, lr=0.01) if kind == 'adam' else FlatSGD(flat, lr=0.05, momentum=0.9)
    clip = torch.zeros(2, device=dev)
    mx = torch.tensor([1.0], device=dev)
    flag = torch.zeros(2, dtype=torch.int32, device=dev)
    parts = torch.zeros(_parts(), device=dev)
    o.set_grad_multiplier(clip[1:2])

    def step(g):
        o.grad.copy_(g.to(dev))
        lib().call('fami_sumsq_f32', o.grad.data_ptr(), N, parts.data_ptr(), _st(dev))
        lib().call('fami_clip_coef_f32', parts.data_ptr(), parts.numel(), mx.data_ptr(), clip.data_ptr(), flag.data_ptr(), _st(dev))
        o.step(flag)
    step(torch.randn(N))
    before = [flat.clone()] + [t.clone() for t in o.tensors()]
    g = torch.randn(N)
    g[500] = float('nan')
    step(g)
    after = [flat] + o.tensors()
    for x, y in zip(before[:-1], after[:-1]):
        assert torch.equal(x, y)
    assert o.state[0].item() == 1.0 and flag[0].item() == 0 and flag[1].item() == 1
    step(torch.randn(N))
    assert o.state[0].item() == 2.0 and not torch.equal(flat, before[0]) and torch.isfinite(flat).all()
