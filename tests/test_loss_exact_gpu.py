"""csrc/loss.hip through the C ABI, with guard zones around every output and NaN around every operand: wmse forward and backward,
argmax2d, final_preds, pck_accuracy and the Gaussian targets against exact references (tests/_stream_exact.py: integer
operands, power-of-two factors, fp32 row sums below 2^24 quarter-units; decode and PCK against oracle.ops on rows built so that
the order of the reduction decides the answer, NaN ordered as numpy orders it), and softmax_kl -- the one family with a
tolerance, which the test measures: 8 x the error of the fp32 CPU evaluation of oracle.ops.softmax_kl_rows against its fp64
self on the same operands, floor 2^-20.  Last, the reference-generated fixtures g5_mse, g6_targets and g7_decode of
tests/golden/ on the HIP path, at the tolerances tests/test_oracle.py grants the oracle."""
import os

import numpy as np
import pytest
import torch

import _stream_exact as SE

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def run(fn, cases, dev):
    fails = []
    for c in cases:
        fails += fn(c, None, SE.Run(dev))
    assert not fails, fails


def test_wmse_forward_and_backward(dev):
    run(SE.wmse, SE.WMSE_CASES, dev)


@pytest.mark.parametrize('L', SE.ARGMAX_L)
def test_argmax2d_reduction_order_and_nan(dev, L):
    run(SE.argmax2d, [L], dev)


@pytest.mark.parametrize('case', SE.FINAL_CASES, ids=['8x6', '96x72'])
def test_final_preds(dev, case):
    run(SE.final_preds, [case], dev)


def test_pck_accuracy(dev):
    run(SE.pck, SE.PCK_CASES, dev)


def test_gauss_targets_between_guards(dev):
    run(SE.gauss, SE.GAUSS_CASES, dev)


@pytest.mark.parametrize('L', SE.KL_L)
def test_softmax_kl_against_the_fp32_yardstick(dev, L):
    """Measured on the MI355X, the largest over R = 1, 3, 257 (kernel error / fp32 CPU yardstick; the gradient over the four
    backward forms, as a fraction of the row maximum).  The test prints its own figures before it asserts.
        L      value              sa                 sb                 S                  gradient
        1      0 / 0              3.1e-7 / 3.1e-7    4.1e-7 / 4.1e-7    0 / 0              0 / 0
        2      4.4e-8 / 1.2e-7    1.9e-7 / 1.9e-7    2.6e-7 / 2.6e-7    2.4e-7 / 1.7e-7    2.6e-2 / 2.9e-2
        255    9.9e-8 / 9.9e-8    2.0e-7 / 2.3e-7    1.7e-7 / 2.2e-7    1.9e-7 / 2.4e-7    4.9e-6 / 1.6e-5
        256    8.5e-8 / 8.5e-8    3.4e-7 / 2.5e-7    1.4e-7 / 2.1e-7    3.2e-7 / 2.5e-7    2.5e-6 / 5.4e-6
        257    9.0e-8 / 5.3e-8    2.0e-7 / 1.8e-7    1.2e-7 / 1.0e-7    2.4e-7 / 2.3e-7    6.8e-6 / 7.3e-6
        4095   8.4e-8 / 2.3e-7    3.2e-7 / 5.4e-7    2.3e-7 / 2.8e-7    1.3e-7 / 1.7e-7    8.9e-7 / 6.3e-6
        4096   8.0e-8 / 1.5e-7    2.2e-7 / 2.2e-7    1.7e-7 / 2.2e-7    1.8e-7 / 2.0e-7    1.1e-6 / 2.8e-6
        4097   1.2e-7 / 2.0e-7    1.8e-7 / 1.8e-7    1.5e-7 / 1.9e-7    1.9e-7 / 2.2e-7    8.7e-7 / 6.2e-6
        8192   1.4e-7 / 3.9e-7    2.2e-7 / 2.5e-7    1.3e-7 / 1.8e-7    1.8e-7 / 1.8e-7    1.0e-5 / 7.4e-5
        8193   1.2e-7 / 3.3e-7    3.0e-7 / 1.8e-7    2.1e-7 / 2.1e-7    2.5e-7 / 2.3e-7    8.5e-7 / 3.1e-6
    (L = 2 with 257 rows holds rows whose two gradient elements nearly cancel: fp32 and the kernel lose the same digits there.)"""
    fails, report = [], []
    for Rr in SE.KL_R:
        fails += SE.softmax_kl((Rr, L), None, SE.Run(dev), report)
    for line in report:
        print('softmax_kl R %3d L %5d: ' % (line['R'], line['L']) +
              '  '.join('%s %.3g (fp32 %.3g)' % (k, line[k][0], line[k][1]) for k in ('value', 'sa', 'sb', 'S', 'grad')))
    assert not fails, fails


def test_softmax_kl_underflow_regime_between_guards(dev):
    """randn * 8: softmax(Bt / T) underflows to exact zeros.  Element-wise the fp32 evaluation is itself off by the whole row
    maximum there (the gradient of a one-hot target cancels to nearly zero), so this keeps the finiteness and value check of
    tests/test_kernels_gpu.py::test_softmax_kl and adds the guard zones and accumulate = 1."""
    from oracle import ops as O
    g = SE.gen('kl underflow')
    Rr, L = 34, 108
    a = (torch.randn(Rr, L, generator=g) * 0.2).float()
    b = (torch.randn(Rr, L, generator=g) * 8.0).float()
    prior = SE.ints(g, (Rr, L), -4, 4)
    ref = O.softmax_kl_rows(a, b).item()
    R = SE.Run(dev)
    F32 = torch.float32
    ad, bd = R.op(a.double(), F32), R.op(b.double(), F32)
    value, stats, ws = R.out((1,), F32, None, 'value'), R.out((Rr, 5), F32, None, 'stats'), R.out((Rr,), F32, None, 'row values')
    R.call('fami_softmax_kl_fwd_f32', SE.ptr(ad), SE.ptr(bd), SE.ptr(value), SE.ptr(stats), Rr, L, SE.KL_T, SE.ptr(ws), R.st)
    outs = []
    for acc in (0, 1):
        d = R.out((Rr, L), F32, prior if acc else None, 'dBt(acc %d)' % acc)
        R.call('fami_softmax_kl_bwd_f32', SE.ptr(ad), SE.ptr(bd), SE.ptr(stats), SE.ptr(d), Rr, L, SE.KL_T, 1.0, None, acc, R.st)
        outs.append(d)
    fails = R.end()
    assert not fails, fails
    assert abs(value.item() - ref) < 1e-6 + 1e-4 * abs(ref)
    assert torch.isfinite(stats).all() and all(torch.isfinite(d).all() for d in outs)
    # accumulate = 1 adds the same gradient to the prior: one fp32 rounding of a sum below 8 (an ulp there is 2^-21)
    assert (outs[1].cpu().double() - prior - outs[0].cpu().double()).abs().max().item() <= 2.0 ** -21


# ------------------------------------------------------------------ the reference's own fixtures on the HIP path
@pytest.mark.parametrize('name', ['b4', 'b1'])
def test_g5_mse_on_the_device(dev, name):
    from fami_pose_amd.loss import JointMSELoss
    g = np.load(os.path.join(GOLD, 'g5_mse.npz'))
    p, t, w = (torch.from_numpy(g[name + k]).to(dev) for k in ('.pred', '.gt', '.w'))
    assert abs(JointMSELoss()(p, t, w).item() - float(g[name + '.loss'])) < 1e-6
    assert abs(JointMSELoss(True, False)(p, t, w).item() - float(g[name + '.loss_nodiv'])) < 2e-5
    assert abs(JointMSELoss(False, True)(p, t, w).item() - float(g[name + '.loss_nowt'])) < 1e-6
    pp = p.clone().requires_grad_(True)
    JointMSELoss()(pp, t, w).backward()
    want = torch.from_numpy(g[name + '.gpred']).double()
    assert ((pp.grad.cpu().double() - want).abs().max() / want.abs().max()).item() <= 1e-5


@pytest.mark.parametrize('sigma', [3, 2])
def test_g6_targets_on_the_device(dev, sigma):
    from fami_pose_amd.loss import generate_heatmaps
    g = np.load(os.path.join(GOLD, 'g6_targets.npz'))
    t, w = generate_heatmaps(torch.from_numpy(g['joints'])[None].to(dev), torch.from_numpy(g['vis'])[None].to(dev), sigma, (288, 384), (72, 96))
    t, w = t[0].cpu().numpy(), w[0].cpu().numpy()
    assert np.abs(t.astype(np.float64) - g['s%d.target' % sigma]).max() < 1e-6
    assert np.array_equal(w, g['s%d.weight' % sigma])
    assert w[4, 0] == 0 and w[5, 0] == 0 and w[11, 0] == 0.5 and t[11].max() == 0 and t[10].max() == 0


def test_g7_decode_on_the_device(dev):
    from fami_pose_amd import loss as FL
    g = np.load(os.path.join(GOLD, 'g7_decode.npz'))
    out, tgt = torch.from_numpy(g['out']).to(dev), torch.from_numpy(g['tgt']).to(dev)
    preds, maxvals = FL.get_max_preds(out)
    assert np.array_equal(preds.cpu().numpy(), g['preds']) and np.array_equal(maxvals.cpu().numpy(), g['maxvals'])
    acc, avg, cnt, pred = FL.accuracy(out, tgt)
    assert np.array_equal(acc, g['acc']) and avg == float(g['avg']) and cnt == int(g['cnt'])
    assert np.array_equal(pred, g['pred'])
    assert np.array_equal(FL.argmax_indices(out).cpu().numpy(), g['out'].reshape(3, 17, -1).argmax(2))
