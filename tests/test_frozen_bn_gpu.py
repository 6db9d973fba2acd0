"""BatchNorm with FROZEN statistics at kernel level: the eval-mode forward (fami_bn_eval_stats_f32 + fami_bn_apply_*) and the
one-pass backward fami_bn_eval_bwd_* through Engine.bn / Engine.fuse_term, against torch autograd on the CPU with the
BatchNorm in eval mode.  Tolerances are the project's own for the train-mode BatchNorm kernels (test_kernels_gpu.py::
test_bn_train_fwd_bwd, test_kernels_half_gpu.py::test_bn_half), which do the same arithmetic with more terms; all are
relative to the reference's maximum."""
import contextlib
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ACT_TOL, F32_TOL = 1e-2, 2e-3          # 16-bit storage: test_kernels_half_gpu.py's bf16 pair, applied to both 16-bit types
DTYPES = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
CASES = [(48, True, True), (48, True, False), (96, False, False), (16, True, False), (384, True, True), (256, False, True),
         (1024, False, False), (4, True, False)]
SIZES = [(1, 1, 1), (3, 10, 7), (9, 48, 36)]


def _eng(dev, dt='f32', deterministic=None):
    from fami_pose_amd.engine import Engine
    return Engine(dev, dtype=DTYPES[dt], deterministic=deterministic)


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.float().permute(0, 3, 1, 2).contiguous()


def relerr(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def _bn_pair(C, dev, seed):
    """a CPU BatchNorm in eval mode with non-trivial statistics and its device copy in TRAIN mode with frozen statistics"""
    torch.manual_seed(seed)
    bn = nn.BatchNorm2d(C, momentum=0.1)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_(0, 0.2)
        bn.running_mean.normal_(0.5, 0.4)
        bn.running_var.uniform_(0.5, 3.0)
        bn.num_batches_tracked.fill_(7)
    bn.eval()
    bd = nn.BatchNorm2d(C, momentum=0.1).to(dev)
    bd.load_state_dict(bn.state_dict())
    bd.train()
    bd.frozen_stats = True
    return bn, bd


def _buffers(bd):
    return [bd.running_mean.clone(), bd.running_var.clone(), bd.num_batches_tracked.clone()]


@contextlib.contextmanager
def launches():
    """-> the list of entry-point names (with their arguments) called inside the block: lib().call / call_routed wrapped on the
    instance, the way tests/_launch_log.py does"""
    from fami_pose_amd._lib import lib
    L, log = lib(), []
    call, call_routed = L.call, L.call_routed
    L.call = lambda name, *a: (log.append((name, a)), call(name, *a))[1]
    L.call_routed = lambda route, name, *a: (log.append((name, a)), call_routed(route, name, *a))[1]
    try:
        yield log
    finally:
        del L.call, L.call_routed


def _case(dev, C, relu, res, size, dt, seed=None):
    """torch reference (fp32 operands rounded to the storage type) and the engine run -> everything the tests compare"""
    from fami_pose_amd.engine import T
    tdt = DTYPES[dt]
    rb = (lambda t: t) if dt == 'f32' else (lambda t: t.to(tdt).float())
    N, H, W = size
    bn, bd = _bn_pair(C, dev, C if seed is None else seed)
    x = rb(torch.randn(N, C, H, W) * 2 + 0.7).requires_grad_(True)
    r = rb(torch.randn(N, C, H, W)).requires_grad_(True) if res else None
    y = bn(x)
    if res:
        y = y + r
    if relu:
        y = F.relu(y)
    gy = rb(torch.randn_like(y))
    y.backward(gy)
    before = _buffers(bd)
    eng = _eng(dev, dt)
    xt = T(nhwc(x.detach()).to(dev).to(tdt), True)
    rt = T(nhwc(r.detach()).to(dev).to(tdt), True) if res else None
    yt = eng.bn(xt, bd, relu=relu, residual=rt)
    yt.grad = nhwc(gy).to(dev).to(tdt)
    with launches() as log:
        eng.backward()
    torch.cuda.synchronize(dev)
    return dict(bn=bn, bd=bd, x=x, r=r, y=y, gy=gy, eng=eng, xt=xt, rt=rt, yt=yt, before=before, log=log)


@pytest.mark.parametrize('dt', list(DTYPES))
@pytest.mark.parametrize('size', SIZES, ids=['one-row', 'ragged', 'grid-strides'])
@pytest.mark.parametrize('C,relu,res', CASES)
def test_frozen_bn_backward_vs_torch_eval(dev, C, relu, res, size, dt):
    """(1,1,1): fewer rows than one workgroup holds; (3,10,7): 210 rows, no multiple of the rows per workgroup (21 at C = 48) or
    of the unroll; (9,48,36): several grid strides.  The forward is bitwise the eval-mode forward, the statistics and the
    batch counter do not move, and the backward is torch's eval-mode BatchNorm backward."""
    from fami_pose_amd.engine import T
    c = _case(dev, C, relu, res, size, dt)
    bn, bd, eng, xt, rt, yt = c['bn'], c['bd'], c['eng'], c['xt'], c['rt'], c['yt']
    half = dt != 'f32'
    assert yt.data.dtype == DTYPES[dt]
    assert relerr(nchw(yt.data), c['y']) < (ACT_TOL if half else 1e-5)
    e_dx = relerr(nchw(xt.grad), c['x'].grad)
    e_dg = relerr(eng.param_grads[id(bd.weight)], bn.weight.grad)
    e_db = relerr(eng.param_grads[id(bd.bias)], bn.bias.grad)
    print('frozen bn %s C=%d relu=%d res=%d %s: dx %.2e dgamma %.2e dbeta %.2e' % (dt, C, relu, res, size, e_dx, e_dg, e_db))
    assert e_dx < (2 * ACT_TOL if half else 5e-5)
    assert e_dg < (5 * F32_TOL if half else 5e-5)
    assert e_db < (5 * F32_TOL if half else 5e-5)
    if res and not half:
        assert relerr(nchw(rt.grad), c['r'].grad) < 1e-6
    if res:
        assert rt.grad is not None and rt.grad.dtype == DTYPES[dt]
    for a, b in zip(c['before'], _buffers(bd)):
        assert torch.equal(a, b)
    assert eng.bn_trained == []
    names = [n for n, _ in c['log'] if n.startswith('fami_bn')]
    assert names == ['fami_bn_eval_bwd_' + dt], names
    # the forward is the eval-mode forward that exists today, bit for bit
    del bd.frozen_stats
    bd.eval()
    e2 = _eng(dev, dt)
    y2 = e2.bn(T(xt.data, False), bd, relu=relu, residual=None if rt is None else T(rt.data, False))
    assert torch.equal(y2.data, yt.data)


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_plain_eval_mode_has_the_same_backward(dev, dt):
    """model.eval() under a recording engine: the same launches and bits as train mode with frozen statistics"""
    from fami_pose_amd.engine import T
    c = _case(dev, 48, True, True, (3, 10, 7), dt)
    bd = c['bd']
    del bd.frozen_stats
    bd.eval()
    eng = _eng(dev, dt)
    xt, rt = T(c['xt'].data, True), T(c['rt'].data, True)
    yt = eng.bn(xt, bd, relu=True, residual=rt)
    yt.grad = c['yt'].grad
    eng.backward()
    assert torch.equal(xt.grad, c['xt'].grad) and torch.equal(rt.grad, c['rt'].grad)
    assert torch.equal(eng.param_grads[id(bd.weight)], c['eng'].param_grads[id(bd.weight)])
    assert torch.equal(eng.param_grads[id(bd.bias)], c['eng'].param_grads[id(bd.bias)])


@pytest.mark.parametrize('dt', list(DTYPES))
@pytest.mark.parametrize('P,C', [(210, 48), (15552, 96)])
def test_accumulate_flags(dev, dt, P, C):
    """acc_dx, acc_param, acc_dres each on and off, through the C ABI: "on" equals "off" plus what the buffer held before,
    to the tolerances of the backward itself."""
    from fami_pose_amd._lib import lib
    L, tdt, half = lib(), DTYPES[dt], dt != 'f32'
    torch.manual_seed(P + C)
    st = torch.cuda.current_stream(dev).cuda_stream
    mk = lambda *s: torch.randn(*s, device=dev)
    dy, x, y = mk(P, C).to(tdt), (mk(P, C) * 2 + 0.7).to(tdt), mk(P, C).to(tdt)
    mean, invstd, gamma = mk(C) * 0.3, torch.rand(C, device=dev) + 0.5, torch.rand(C, device=dev) + 0.5
    prior = {'dx': mk(P, C).to(tdt), 'dres': mk(P, C).to(tdt), 'dg': mk(C) * 10, 'db': mk(C) * 10}
    ws = torch.empty(L.cdll.fami_bn_workspace(C) // 4, device=dev)

    def run(acc_dx, acc_param, acc_dres):
        b = {k: v.clone() for k, v in prior.items()}
        L.call('fami_bn_eval_bwd_' + dt, dy.data_ptr(), x.data_ptr(), y.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
               gamma.data_ptr(), b['dx'].data_ptr(), b['dg'].data_ptr(), b['db'].data_ptr(), b['dres'].data_ptr(), P, C, 1,
               acc_dx, acc_param, acc_dres, ws.data_ptr(), st)
        torch.cuda.synchronize(dev)
        return b
    off = run(0, 0, 0)
    # "off" itself against the definition, in fp64 on the stored values
    dz = dy.double() * (y.double() > 0)
    ref = {'dx': dz * (gamma * invstd).double(), 'dres': dz, 'db': dz.sum(0),
           'dg': (dz * (x.double() - mean.double()) * invstd.double()).sum(0)}
    tol = {'dx': 2 * ACT_TOL if half else 5e-5, 'dres': 2 * ACT_TOL if half else 1e-6,
           'dg': 5 * F32_TOL if half else 5e-5, 'db': 5 * F32_TOL if half else 5e-5}
    for k in ref:
        assert relerr(off[k], ref[k]) < tol[k], k
    for flags in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
        on = run(*flags)
        acc = {'dx': flags[0], 'dg': flags[1], 'db': flags[1], 'dres': flags[2]}
        for k in ref:
            want = ref[k] + prior[k].double() if acc[k] else ref[k]
            assert relerr(on[k], want) < tol[k], (flags, k)
            if not acc[k]:
                assert torch.equal(on[k], off[k]), (flags, k)


@pytest.mark.parametrize('dt', list(DTYPES))
@pytest.mark.parametrize('size', [(3, 10, 7), (9, 48, 36)], ids=['ragged', 'grid-strides'])
def test_frozen_gamma_beta(dev, dt, size):
    """requires_grad = False on gamma and beta: dx is still right, and the one call gets no parameter-gradient pointers and no
    workspace -- by the entry point's contract that is the form without sums and without the finalize launch (x, mean and
    ws are then not read: the direct call below passes NULL for all three and a poisoned workspace stays poisoned)."""
    from fami_pose_amd.engine import T
    from fami_pose_amd._lib import lib
    tdt, half = DTYPES[dt], dt != 'f32'
    rb = (lambda t: t) if not half else (lambda t: t.to(tdt).float())
    N, H, W = size
    C = 48
    bn, bd = _bn_pair(C, dev, 5)
    for p in (bn.weight, bn.bias, bd.weight, bd.bias):
        p.requires_grad = False
    x = rb(torch.randn(N, C, H, W) * 2 + 0.7).requires_grad_(True)
    y = F.relu(bn(x))
    gy = rb(torch.randn_like(y))
    y.backward(gy)
    eng = _eng(dev, dt)
    xt = T(nhwc(x.detach()).to(dev).to(tdt), True)
    yt = eng.bn(xt, bd, relu=True)
    yt.grad = nhwc(gy).to(dev).to(tdt)
    with launches() as log:
        eng.backward()
    torch.cuda.synchronize(dev)
    assert relerr(nchw(xt.grad), x.grad) < (2 * ACT_TOL if half else 5e-5)
    log = [e for e in log if e[0].startswith('fami_bn')]
    assert [n for n, _ in log] == ['fami_bn_eval_bwd_' + dt]
    a = log[0][1]       # (dy, x, y, mean, invstd, gamma, dx, dgamma, dbeta, dres, P, C, relu, acc_dx, acc_param, acc_dres, ws, stream)
    assert not a[7] and not a[8] and not a[16], a
    assert id(bd.weight) not in eng.param_grads and id(bd.bias) not in eng.param_grads
    # the same call by hand with x = mean = ws = NULL: accepted, same bits
    L, P = lib(), N * H * W
    dx2 = torch.empty_like(xt.grad)
    L.call('fami_bn_eval_bwd_' + dt, a[0], None, a[2], None, a[4], a[5], dx2.data_ptr(), None, None, None, P, C, 1, 0, 0, 0,
           None, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    assert torch.equal(dx2, xt.grad)


def test_fuse_terms_frozen(dev):
    """test_kernels_gpu.py::test_fuse_sum_fwd_bwd's three-term sum (shifts 0, 1, 2) with all three BatchNorms frozen, against
    torch with those BatchNorms in eval mode, to that test's tolerances."""
    from fami_pose_amd.engine import T
    torch.manual_seed(1)
    N, C, H, W = 2, 48, 16, 12
    pairs = [_bn_pair(C, dev, 20 + k) for k in range(3)]
    bns, bd = [p[0] for p in pairs], [p[1] for p in pairs]
    torch.manual_seed(1)
    x0 = torch.randn(N, C, H, W, requires_grad=True)
    z1 = torch.randn(N, C, H // 2, W // 2, requires_grad=True)
    z2 = torch.randn(N, C, H // 4, W // 4, requires_grad=True)
    z3 = torch.randn(N, C, H, W, requires_grad=True)
    y = F.relu(x0 + F.interpolate(bns[0](z1), scale_factor=2, mode='nearest')
               + F.interpolate(bns[1](z2), scale_factor=4, mode='nearest') + bns[2](z3))
    gy = torch.randn_like(y)
    y.backward(gy)
    before = [_buffers(d) for d in bd]
    eng = _eng(dev)
    ts = [T(nhwc(t.detach()).to(dev), True) for t in (x0, z1, z2, z3)]
    yt = eng.fuse([eng.fuse_term(*t) for t in ((ts[0], None, 0), (ts[1], bd[0], 1), (ts[2], bd[1], 2), (ts[3], bd[2], 0))])
    assert relerr(nchw(yt.data), y) < 1e-5
    yt.grad = nhwc(gy).to(dev)
    with launches() as log:
        eng.backward()
    torch.cuda.synchronize(dev)
    for t, ref in zip(ts, (x0, z1, z2, z3)):
        assert relerr(nchw(t.grad), ref.grad) < 5e-5
    for d, b in zip(bd, bns):
        assert relerr(eng.param_grads[id(d.weight)], b.weight.grad) < 5e-5
        assert relerr(eng.param_grads[id(d.bias)], b.bias.grad) < 5e-5
    for d, b in zip(bd, before):
        for u, v in zip(_buffers(d), b):
            assert torch.equal(u, v)
    names = [n for n, _ in log]
    assert names.count('fami_bn_eval_bwd_f32') == 3 and names.count('fami_pool_relu_bwd_f32') == 2, names
    assert [n for n in names if n.startswith('fami_bn')] == ['fami_bn_eval_bwd_f32'] * 3, names
    assert eng.bn_trained == []


@pytest.mark.parametrize('deterministic', [False, True], ids=['default', 'deterministic'])
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_backward_is_bitwise_reproducible(dev, dt, deterministic):
    """fixed-order partial rows + a fixed-order fp64 finalize: two runs on the same inputs give the same bits, in either engine mode"""
    from fami_pose_amd.engine import T
    c = _case(dev, 48, True, True, (9, 48, 36), dt)
    bd, outs = c['bd'], []
    for _ in range(2):
        eng = _eng(dev, dt, deterministic=deterministic)
        xt, rt = T(c['xt'].data, True), T(c['rt'].data, True)
        yt = eng.bn(xt, bd, relu=True, residual=rt)
        yt.grad = c['yt'].grad
        with launches() as log:
            eng.backward()
        torch.cuda.synchronize(dev)
        assert [n for n, _ in log if n.startswith('fami_bn')] == ['fami_bn_eval_bwd_' + dt]
        outs.append((xt.grad.clone(), rt.grad.clone(), eng.param_grads[id(bd.weight)].clone(),
                     eng.param_grads[id(bd.bias)].clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    for a, b in zip(outs[0], (c['xt'].grad, c['rt'].grad, c['eng'].param_grads[id(bd.weight)], c['eng'].param_grads[id(bd.bias)])):
        assert torch.equal(a, b)        # ... and the default engine of _case gave them too: one form, no switch


TRAIN_ONLY = ('fami_bn_stats_', 'fami_bn_train_fwd', 'fami_bn_apply_slots_', 'fami_bn_bwd_', 'fami_bn_bwd2_',
              'fami_bn_bwd_apply_slots_', 'fami_bn_finalize_slots_f32', 'fami_bn_running_update', 'fami_conv2d_fwd_stats_',
              'fami_conv2d_dgrad_bnstats_')


@pytest.mark.parametrize('name', ['basic', 'neck', 'neck_ds'])
def test_blocks_with_frozen_bn_match_the_oracle_in_eval(dev, name):
    """A BasicBlock / Bottleneck (through Engine.conv_bn / conv_bn_relu_into) with frozen BatchNorms against the oracle's modules
    with .eval() on their BatchNorms, by test_blocks_golden_gpu.py's criteria at its 1e-4; none of the train-only BatchNorm
    fusions or kernels is taken."""
    from fami_pose_amd.engine import Engine, T
    from fami_pose_amd import modules as M
    from fami_pose_amd.train import freeze_batchnorm
    from oracle import model as om
    TOL = 1e-4
    make = {'basic': (lambda: om.Basic(16, 16), lambda: M.BasicBlock(16, 16)),
            'neck': (lambda: om.Neck(32, 8), lambda: M.Bottleneck(32, 8)),
            'neck_ds': (lambda: om.Neck(16, 8, 1, om._proj(16, 32)), lambda: M.Bottleneck(16, 8, 1, M._shortcut(16, 32)))}[name]
    orc = om.realistic_init_(make[0](), 100)
    gen = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for m in orc.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=gen) * 0.2)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=gen) * 1.5 + 0.5)
    inner = make[1]()
    inner.load_state_dict(orc.state_dict())
    inner = inner.to(dev).train()
    assert len(freeze_batchnorm(inner, 'all')) >= 2
    orc.train()
    for m in orc.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.eval()
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g1_blocks.npz'))
    x0 = torch.from_numpy(g[name + '.x'])
    xr = x0.clone().requires_grad_(True)
    y0 = orc(xr)
    gy = torch.randn(y0.shape, generator=gen)
    y0.backward(gy)
    before = {k: v.clone() for k, v in inner.state_dict().items()}
    eng = Engine(dev)
    xt = T(x0.permute(0, 2, 3, 1).contiguous().to(dev), True)
    with launches() as log:
        y = inner.run(eng, xt)
        y.grad = gy.permute(0, 2, 3, 1).contiguous().to(dev)
        eng.backward()
    torch.cuda.synchronize(dev)
    assert relerr(nchw(y.data), y0) < TOL
    assert relerr(nchw(xt.grad), xr.grad) < TOL
    p, ref = dict(inner.named_parameters()), dict(orc.named_parameters())
    names = sorted(ref)
    gabs = np.array([eng.param_grads[id(p[k])].double().abs().sum().item() for k in names])
    gsum = np.array([eng.param_grads[id(p[k])].double().sum().item() for k in names])
    ref_abs = np.array([ref[k].grad.double().abs().sum().item() for k in names])
    ref_sum = np.array([ref[k].grad.double().sum().item() for k in names])
    assert np.allclose(gabs, ref_abs, rtol=TOL, atol=TOL * np.abs(ref_abs).max()), (gabs, ref_abs)
    assert np.allclose(gsum, ref_sum, rtol=1e-3, atol=2e-4 * np.abs(ref_abs).max()), (gsum, ref_sum)
    for mn, m in inner.named_modules():          # gamma / beta of the frozen BatchNorms element by element
        if isinstance(m, nn.BatchNorm2d):
            for k in (mn + '.weight', mn + '.bias'):
                assert relerr(eng.param_grads[id(p[k])], ref[k].grad) < TOL, k
    for k, v in inner.state_dict().items():
        assert torch.equal(v, before[k]), k
    called = [n for n, _ in log]
    assert not [n for n in called if n.startswith(TRAIN_ONLY)], called
    nbn = sum(isinstance(m, nn.BatchNorm2d) for m in inner.modules())
    assert sum(n.startswith('fami_bn_eval_bwd_') for n in called) == nbn
    assert eng.bn_trained == [] and eng.nfused == {'fwd': 0, 'bwd': 0, 'xbn': 0}
