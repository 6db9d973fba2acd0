"""The integral (soft-argmax) coordinate kernels on the MI355X (csrc/loss.hip: fami_softargmax_fwd_f32 / _bwd_f32,
fami_heatmap_xy_f32, fami_integral_l1_fwd_f32 / _bwd_f32, fami_softargmax_preds_f32) with loss.soft_argmax / IntegralL1Loss /
integral_get_final_preds and evaluate.predict(decode='integral') on top.

Kernel launches go through the C ABI: operands uploaded inside NaN, outputs between guard zones (tests/_stream_exact.Run).

Bounds.  The exact cases (tests/_integral_ref.exact_case) have none: every result is determined, whatever the order of the sums.
Everything else is held to the project's rule for kernels that call expf (tests/_stream_exact.softmax_kl): 8 x the error of
the plain fp32 CPU evaluation (torch.softmax(beta h), weighted sums) against the float64 restatement on the same fp32 operands,
with a floor of 2^-20 of the coordinate range (W for x, H for y; of the row maximum for the gradient).  The loss is a weighted sum of
normalised coordinate errors: its bound follows from the coordinates' (loss_bound).  The decode multiplies by the crop's image
pixels per heatmap pixel, s = 200 scale / W, and so do its bound and floor."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _integral_ref as ir  # noqa: E402
from _stream_exact import F32, F64, Run, ptr  # noqa: E402

from fami_pose_amd import evaluate as ev, loss as FL  # noqa: E402
from test_dark_gpu import CENTER, SCALE, e2e  # noqa: E402,F401  (the small evaluation model of the DARK tests)

pytestmark = pytest.mark.gpu
NAN = float('nan')


def bound(yard, floor):
    return max(ir.MARGIN * yard, floor)


def loss_bound(scale, w, bx, by, H, W, l64):
    """The loss is scale sum_r w_r (|cx - tx| / W + |cy - ty| / H): coordinates within bx, by of the float64 ones move it by at
    most scale sum_r w_r (bx / W + by / H); the fp32 row arithmetic (two subtractions, two divisions, an addition, a product)
    and the final rounding add a few units of 2^-24 of its value: 2^-21."""
    return scale * w.double().abs().sum().item() * (bx / W + by / H) + 2.0 ** -21 * abs(l64)


def axis_errors(got, want, live):
    d = (got.double() - want).abs()[live]
    return d[..., 0].max().item(), d[..., 1].max().item()


# ---------------------------------------------------------------------------------------- 1. exact cases
@pytest.mark.parametrize('case', ir.EX_CASES, ids=lambda c: 'K%d-R%d' % c)
def test_exact_cases(dev, case):
    c = ir.exact_case(*case)
    Rr, H, W = c['R'], ir.EX_H, ir.EX_W
    R = Run(dev)
    h, txy, w = R.op(c['h'].double(), F32), R.op(c['txy'], F32), R.op(c['w'], F32)
    coords, stats = R.out((Rr, 2), F32, None, 'coords'), R.out((Rr, 2), F32, None, 'stats')
    R.call('fami_softargmax_fwd_f32', ptr(h), ptr(coords), ptr(stats), Rr, H, W, ir.EX_BETA, R.st)
    R.want('coords', coords, torch.stack([c['cx'], c['cy']], 1), '(r,xy)')
    R.want('stats', stats, torch.stack([torch.zeros(Rr, dtype=F64), torch.full((Rr,), float(c['K']), dtype=F64)], 1), '(r,mZ)')
    for s, wl in zip(c['scales'], c['want_loss']):
        loss, ws = R.out((1,), F32, None, 'loss'), R.out((Rr,), F32, None, 'row values')
        R.call('fami_integral_l1_fwd_f32', ptr(coords), ptr(txy), ptr(w), ptr(loss), Rr, H, W, s, ptr(ws), R.st)
        R.want('loss at scale %r' % s, loss, wl)
        R.want('row values', ws, c['rows'])
    gdev = R.op(torch.tensor([c['g0']], dtype=F64), F32)
    for (acc, hg), wg in c['grads'].items():
        d = R.out((Rr, H, W), F32, c['prior'] if acc else None, 'dhm(acc %d)' % acc)
        R.call('fami_integral_l1_bwd_f32', ptr(h), ptr(coords), ptr(stats), ptr(txy), ptr(w), ptr(d), Rr, H, W, ir.EX_BETA,
               c['gscale'], ptr(gdev) if hg else None, acc, R.st)
        R.want('gradient acc %d gdev %d' % (acc, hg), d, wg, '(r,y,x)')
    fails = R.end()
    assert not fails, '\n'.join(fails)


def test_flat_map_and_dominant_maximum(dev):
    H, W = ir.EX_H, ir.EX_W
    g = torch.Generator().manual_seed(11)
    lead = 104.0 / 20.0 + 1.0          # beta = 20: every other logit is more than 104 below the maximum
    maps = torch.rand(5, H, W, generator=g).double() - 1.0
    peaks = [(0, 0), (W - 1, H - 1), (3, 7), (W - 1, 0), (5, 15)]
    for r, (x, y) in enumerate(peaks):
        maps[r, y, x] = lead
    assert (ir.logits(maps.float(), 20.0).max(1).values - ir.logits(maps.float().clamp(max=0.0), 20.0).max(1).values).min().item() > 104.0
    R = Run(dev)
    for name, hm, beta, want in (('flat', torch.full((2, H, W), 0.375, dtype=F64), ir.EX_BETA,
                                  torch.tensor([[(W - 1) / 2, (H - 1) / 2]] * 2, dtype=F64)),
                                 ('dominant', maps, 20.0, torch.tensor(peaks, dtype=F64))):
        n = hm.shape[0]
        coords, stats = R.out((n, 2), F32, None, name + ' coords'), R.out((n, 2), F32, None, name + ' stats')
        R.call('fami_softargmax_fwd_f32', ptr(R.op(hm, F32)), ptr(coords), ptr(stats), n, H, W, beta, R.st)
        R.want(name, coords, want, '(r,xy)')
    fails = R.end()
    assert not fails, '\n'.join(fails)


# ---------------------------------------------------------------------------------------- 2. every path, general accuracy
# (H, W, shift): the smallest sizes that cross each instance boundary (registers for L <= 4096 and <= 8192, streaming beyond),
# the two production maps, an odd W, and a view that starts 3 elements behind the 256-byte boundary
SHAPES = [(1, 1, 0), (1, 255, 0), (1, 257, 0), (64, 64, 0), (1, 4097, 0), (96, 72, 0), (1, 8193, 0), (128, 96, 0), (96, 71, 0), (96, 72, 3),
          (1, 8193, 1)]
BETA = 20.0


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d+%d' % s)
def test_paths_against_float64(dev, shape):
    H, W, shift = shape
    Rr = 3
    h = ir.general_maps(Rr, H, W, 100 + H + W)
    txy, w = ir.general_targets(h, BETA, 100 + H + W)
    cx, cy, m, Z, _ = ir.forward(h, BETA)
    px, py = ir.forward_plain32(h, BETA)
    yx, yy = (px.double() - cx).abs().max().item(), (py.double() - cy).abs().max().item()
    Z32 = torch.exp(ir.logits(h, BETA) - m[:, None]).sum(1)
    yZ = ((Z32.double() - Z).abs() / Z).max().item()
    scale = 0.5 / Rr
    l64, l32 = ir.loss(h, BETA, txy, w, scale).item(), ir.loss(h, BETA, txy, w, scale, F32).item()
    prior = torch.randint(-4, 5, (Rr, H, W), generator=torch.Generator().manual_seed(5)).double()
    gs, g0 = 8.0, 0.5

    R = Run(dev)
    hd, td, wd = R.op(h.double(), F32, shift), R.op(txy.double(), F32), R.op(w.double(), F32)
    coords, stats = R.out((Rr, 2), F32, None, 'coords'), R.out((Rr, 2), F32, None, 'stats')
    R.call('fami_softargmax_fwd_f32', ptr(hd), ptr(coords), ptr(stats), Rr, H, W, BETA, R.st)
    loss, ws = R.out((1,), F32, None, 'loss'), R.out((Rr,), F32, None, 'row values')
    R.call('fami_integral_l1_fwd_f32', ptr(coords), ptr(td), ptr(wd), ptr(loss), Rr, H, W, scale, ptr(ws), R.st)
    torch.cuda.synchronize(dev)
    c, st = coords.cpu().double(), stats.cpu()
    ex, ey = (c[:, 0] - cx).abs().max().item(), (c[:, 1] - cy).abs().max().item()
    eZ = ((st[:, 1].double() - Z).abs() / Z).max().item()
    el = abs(loss.item() - l64)
    bx, by = bound(yx, ir.FLOOR * W), bound(yy, ir.FLOOR * H)
    bl = loss_bound(scale, w, bx, by, H, W, l64)
    print('%dx%d: x %.3g px (fp32 %.3g, floor %.3g)  y %.3g px (fp32 %.3g, floor %.3g)  Z %.3g (fp32 %.3g)  loss %.3g (fp32 %.3g, bound %.3g)'
          % (H, W, ex, yx, ir.FLOOR * W, ey, yy, ir.FLOOR * H, eZ, yZ, el, abs(l32 - l64), bl))
    assert torch.equal(st[:, 0], m), 'm is the fp32 maximum of the fp32 logits'
    assert ex <= bx and ey <= by
    assert eZ <= bound(yZ, ir.FLOOR)
    assert el <= bl

    gdev = R.op(torch.tensor([g0], dtype=F64), F32)
    for acc in (0, 1):
        for hg in (0, 1):
            f = gs * (g0 if hg else 1.0)
            want = ir.grad(h, BETA, txy, w, f) + (prior if acc else 0)
            fp32 = ir.grad(h, BETA, txy, w, f, F32) + (prior.float() if acc else 0)
            rmax = want.abs().amax((1, 2), keepdim=True).clamp(min=1e-300)
            yard = ((fp32.double() - want).abs() / rmax).max().item()
            d = R.out((Rr, H, W), F32, prior if acc else None, 'dhm(acc %d)' % acc, shift)
            R.call('fami_integral_l1_bwd_f32', ptr(hd), ptr(coords), ptr(stats), ptr(td), ptr(wd), ptr(d), Rr, H, W, BETA, gs,
                   ptr(gdev) if hg else None, acc, R.st)
            torch.cuda.synchronize(dev)
            e = ((d.cpu().double() - want).abs() / rmax).max().item()
            print('    gradient acc %d gdev %d: %.3g of the row maximum (fp32 %.3g)' % (acc, hg, e, yard))
            assert e <= bound(yard, ir.FLOOR)
    # the soft-argmax alone: a random linear form of the coordinates
    gc = torch.randn(Rr, 2, generator=torch.Generator().manual_seed(6))
    want = ir.softargmax_grad(h, BETA, gc)
    rmax = want.abs().amax((1, 2), keepdim=True).clamp(min=1e-300)
    yard = ((ir.softargmax_grad(h, BETA, gc, F32).double() - want).abs() / rmax).max().item()
    d = R.out((Rr, H, W), F32, None, 'dhm(soft-argmax)')
    R.call('fami_softargmax_bwd_f32', ptr(hd), ptr(coords), ptr(stats), ptr(R.op(gc.double(), F32)), ptr(d), Rr, H, W, BETA, 0, R.st)
    torch.cuda.synchronize(dev)
    e = ((d.cpu().double() - want).abs() / rmax).max().item()
    print('    soft-argmax gradient: %.3g of the row maximum (fp32 %.3g)' % (e, yard))
    assert e <= bound(yard, ir.FLOOR)
    fails = R.end()
    assert not fails, '\n'.join(fails)


def test_two_runs_are_bitwise_equal(dev):
    h = ir.general_maps(5, 96, 72, 3).to(dev)
    a, b = FL._softargmax_fwd(h.reshape(1, 5, 96, 72), BETA), FL._softargmax_fwd(h.reshape(1, 5, 96, 72), BETA)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---------------------------------------------------------------------------------------- 3. robustness
def test_wide_logits_zero_weights_and_refusals(dev):
    H, W, Rr = 24, 18, 4
    g = torch.Generator().manual_seed(8)
    h = (torch.rand(Rr, H, W, generator=g) * 100 - 50).float()          # logits in +-1000 at beta = 20
    txy = torch.rand(Rr, 2, generator=g) * 10
    w = torch.tensor([1.0, 0.0, 0.5, 0.0])
    prior = torch.randn(Rr, H, W, generator=g).double()
    R = Run(dev)
    hd, td, wd = R.op(h.double(), F32), R.op(txy.double(), F32), R.op(w.double(), F32)
    coords, stats = R.out((Rr, 2), F32, None, 'coords'), R.out((Rr, 2), F32, None, 'stats')
    R.call('fami_softargmax_fwd_f32', ptr(hd), ptr(coords), ptr(stats), Rr, H, W, BETA, R.st)
    loss, ws = R.out((1,), F32, None, 'loss'), R.out((Rr,), F32, None, 'row values')
    R.call('fami_integral_l1_fwd_f32', ptr(coords), ptr(td), ptr(wd), ptr(loss), Rr, H, W, 0.25, ptr(ws), R.st)
    d0 = R.out((Rr, H, W), F32, None, 'dhm')
    d1 = R.out((Rr, H, W), F32, prior, 'dhm(acc)')
    for d, acc in ((d0, 0), (d1, 1)):
        R.call('fami_integral_l1_bwd_f32', ptr(hd), ptr(coords), ptr(stats), ptr(td), ptr(wd), ptr(d), Rr, H, W, BETA, 1.0, None,
               acc, R.st)
    torch.cuda.synchronize(dev)
    for t in (coords, stats, loss, ws, d0, d1):
        assert torch.isfinite(t).all()
    cx, cy = ir.forward(h, BETA)[:2]
    assert (coords.cpu().double() - torch.stack([cx, cy], 1)).abs().max().item() <= 1e-4
    assert (d0[1] == 0).all() and (d0[3] == 0).all() and (d0[0] != 0).any()          # a weight-0 row: an exact zero row
    R.want_bits('weight-0 rows under accumulate keep their bits', d1[[1, 3]], prior[[1, 3]].float())
    # refusals: -1, the entry point named, nothing written
    c2, s2, l2 = R.out((Rr, 2), F32, None, 'refused coords'), R.out((Rr, 2), F32, None, 'refused stats'), R.out((1,), F32, None, 'refused loss')
    d2, p2, m2 = R.out((Rr, H, W), F32, None, 'refused dhm'), R.out((Rr, 2), F32, None, 'refused preds'), R.out((Rr,), F32, None, 'refused maxvals')
    cs = R.op(torch.ones(Rr, 2, dtype=F64), F32)
    for beta in (0.0, -20.0, float('inf'), NAN):
        R.refused('fami_softargmax_fwd_f32', ptr(hd), ptr(c2), ptr(s2), Rr, H, W, beta, R.st)
        R.refused('fami_integral_l1_bwd_f32', ptr(hd), ptr(coords), ptr(stats), ptr(td), ptr(wd), ptr(d2), Rr, H, W, beta, 1.0, None, 0, R.st)
        R.refused('fami_softargmax_bwd_f32', ptr(hd), ptr(coords), ptr(stats), ptr(td), ptr(d2), Rr, H, W, beta, 0, R.st)
        R.refused('fami_softargmax_preds_f32', ptr(hd), ptr(cs), ptr(cs), beta, ptr(p2), ptr(m2), 1, Rr, H, W, R.st)
    for Rb, Hb, Wb in ((0, H, W), (Rr, 0, W), (Rr, H, -1)):
        R.refused('fami_softargmax_fwd_f32', ptr(hd), ptr(c2), ptr(s2), Rb, Hb, Wb, BETA, R.st)
        R.refused('fami_integral_l1_fwd_f32', ptr(coords), ptr(td), ptr(wd), ptr(l2), Rb, Hb, Wb, 1.0, ptr(ws), R.st)
        R.refused('fami_integral_l1_bwd_f32', ptr(hd), ptr(coords), ptr(stats), ptr(td), ptr(wd), ptr(d2), Rb, Hb, Wb, BETA, 1.0, None, 0, R.st)
        R.refused('fami_softargmax_preds_f32', ptr(hd), ptr(cs), ptr(cs), BETA, ptr(p2), ptr(m2), 1, Rb, Hb, Wb, R.st)
    for t, name in ((c2, 'coords'), (s2, 'stats'), (l2, 'loss'), (d2, 'dhm'), (p2, 'preds'), (m2, 'maxvals')):
        R.want_untouched('refused ' + name, t)
    fails = R.end()
    assert not fails, '\n'.join(fails)


def test_heatmap_xy_is_the_subpixel_centre(dev):
    """joint / stride as fami_gauss_target_ex_f32(subpixel = 1) forms it: in double, rounded once"""
    g = torch.Generator().manual_seed(4)
    joints = (torch.rand(3, 17, 2, generator=g) * torch.tensor([288.0, 384.0])).float()
    got = FL.heatmap_xy(joints.to(dev), (288, 384), (72, 96)).cpu()
    want = (joints.double() / torch.tensor([288.0 / 72, 384.0 / 96], dtype=F64)).float()
    assert torch.equal(got, want)
    got = FL.heatmap_xy(joints.to(dev), (100, 70), (33, 17)).cpu()          # strides that are no power of two
    want = (joints.double() / torch.tensor([100.0 / 33, 70.0 / 17], dtype=F64)).float()
    assert torch.equal(got, want)


# ---------------------------------------------------------------------------------------- 4. module and decode
@pytest.mark.parametrize('BJ', [(2, 17), (3, 5)])
@pytest.mark.parametrize('use_w', [True, False])
def test_module_forward_backward(dev, BJ, use_w):
    B, J = BJ
    H, W = 24, 18
    h = ir.general_maps(B * J, H, W, 21)
    txy, w = ir.general_targets(h, BETA, 21)
    w[1] = 0.0
    weff = w if use_w else torch.ones_like(w)
    pred = h.reshape(B, J, H, W).to(dev).requires_grad_(True)
    crit = FL.IntegralL1Loss(use_target_weight=use_w)
    val = crit(pred, txy.reshape(B, J, 2).to(dev), w.reshape(B, J, 1).to(dev))
    (val * 3.0).backward()
    l64 = ir.loss(h, BETA, txy, weff, 1.0 / (B * J)).item()
    l32 = ir.loss(h, BETA, txy, weff, 1.0 / (B * J), F32).item()
    want = ir.grad(h, BETA, txy, weff, 3.0 / (B * J))
    fp32 = ir.grad(h, BETA, txy, weff, 3.0 / (B * J), F32)
    rmax = want.abs().amax((1, 2), keepdim=True).clamp(min=1e-300)
    live = (weff != 0)
    yard = ((fp32.double() - want).abs() / rmax)[live].max().item()
    e = ((pred.grad.cpu().double().reshape(B * J, H, W) - want).abs() / rmax)[live].max().item()
    cx, cy = ir.forward(h, BETA)[:2]
    px, py = ir.forward_plain32(h, BETA)
    bx, by = bound((px.double() - cx).abs().max().item(), ir.FLOOR * W), bound((py.double() - cy).abs().max().item(), ir.FLOOR * H)
    bl = loss_bound(1.0 / (B * J), weff, bx, by, H, W, l64)
    print('IntegralL1Loss B %d J %d: loss error %.3g (fp32 %.3g, bound %.3g), gradient %.3g of the row maximum (fp32 %.3g)'
          % (B, J, abs(val.item() - l64), abs(l32 - l64), bl, e, yard))
    assert abs(val.item() - l64) <= bl
    assert e <= bound(yard, ir.FLOOR)
    if use_w:
        assert (pred.grad[0, 1] == 0).all()
    # soft_argmax: the coordinates, and autograd through them
    p2 = h.reshape(B, J, H, W).to(dev).requires_grad_(True)
    c = FL.soft_argmax(p2)
    assert c.shape == (B, J, 2)
    assert (c[..., 0].detach().cpu().double().reshape(-1) - cx).abs().max().item() <= bx
    assert (c[..., 1].detach().cpu().double().reshape(-1) - cy).abs().max().item() <= by
    gc = torch.randn(B * J, 2, generator=torch.Generator().manual_seed(2))
    (c * gc.reshape(B, J, 2).to(dev)).sum().backward()
    want = ir.softargmax_grad(h, BETA, gc)
    rmax = want.abs().amax((1, 2), keepdim=True).clamp(min=1e-300)
    yard = ((ir.softargmax_grad(h, BETA, gc, F32).double() - want).abs() / rmax).max().item()
    assert ((p2.grad.cpu().double().reshape(B * J, H, W) - want).abs() / rmax).max().item() <= bound(yard, ir.FLOOR)


@pytest.mark.parametrize('shape', [(2, 17, 96, 72), (1, 4, 128, 96), (2, 4, 7, 5), (1, 4, 1, 8193)])
def test_decode_against_float64_and_the_standard_masks(dev, shape):
    B, J, H, W = shape
    hm = ir.general_maps(B * J, H, W, 31).reshape(B, J, H, W)
    hm[0, 0] = -hm[0, 0].abs() - 0.01          # maximum < 0: masked
    hm[0, 1] = 0.0                             # maximum == 0: masked
    hm[0, 2, H // 2, W // 3] = NAN             # a NaN: masked, maxval NaN
    center = torch.tensor([[320.0, 240.5], [100.25, 400.0]])[:B]
    scale = torch.tensor([[1.5, 2.0], [0.9, 1.2]])[:B]
    want, maxvals, masked = ir.decode(hm, center, scale, BETA)
    fp32 = ir.decode(hm, center, scale, BETA, F32)[0]
    live = ~masked
    assert masked.sum().item() == 3 and live.any()
    R = Run(dev)
    preds, mv = R.out((B, J, 2), F32, None, 'preds'), R.out((B, J), F32, None, 'maxvals')
    R.call('fami_softargmax_preds_f32', ptr(R.op(hm.double(), F32)), ptr(R.op(center.double(), F32)), ptr(R.op(scale.double(), F32)),
           BETA, ptr(preds), ptr(mv), B, J, H, W, R.st)
    torch.cuda.synchronize(dev)
    s = scale[:, 0].max().item() * 200.0 / W          # image pixels per heatmap pixel of the largest crop
    (yx, yy), (ex, ey) = axis_errors(fp32, want, live), axis_errors(preds.cpu(), want, live)
    print('decode %s: x %.3g image px (fp32 %.3g, floor %.3g)  y %.3g (fp32 %.3g, floor %.3g)'
          % (shape, ex, yx, ir.FLOOR * W * s, ey, yy, ir.FLOOR * H * s))
    assert ex <= bound(yx, ir.FLOOR * W * s) and ey <= bound(yy, ir.FLOOR * H * s)
    if H > 2 and W > 2:          # (the standard decode takes maps larger than 2 x 2)
        p_std, m_std = FL.get_final_preds(hm.to(dev), center.numpy(), scale.numpy())
        R.want_bits('maxvals are the standard decode\'s', mv, m_std.reshape(B, J).cpu())
        R.want_bits('masked joints are the standard decode\'s', preds[masked.to(dev)], p_std[masked.to(dev)].cpu())
    p_mod, m_mod = FL.integral_get_final_preds(hm.to(dev), center.numpy(), scale.numpy())
    R.want_bits('module preds', p_mod, preds.cpu())
    R.want_bits('module maxvals', m_mod.reshape(B, J), mv.cpu())
    fails = R.end()
    assert not fails, '\n'.join(fails)


@pytest.mark.parametrize('flip', [False, True])
def test_predict_integral_is_the_decode_of_its_own_map(dev, e2e, flip):  # noqa: F811
    model, kf, sup = e2e['model'], e2e['kf'], e2e['sup']
    preds, maxvals, final_hm = ev.predict(model, kf, sup, CENTER, SCALE, flip=flip, decode='integral')
    p_std, m_std, hm_std = ev.predict(model, kf, sup, CENTER, SCALE, flip=flip, integral_beta=-1.0)      # ignored by 'standard'
    assert torch.equal(final_hm, hm_std)
    p1, m1 = FL.integral_get_final_preds(final_hm, CENTER, SCALE)
    assert torch.equal(preds, p1) and torch.equal(maxvals, m1)
    assert torch.equal(maxvals, m_std) and not torch.equal(preds, p_std)
    p8, _, _ = ev.predict(model, kf, sup, CENTER, SCALE, flip=flip, decode='integral', integral_beta=8.0)
    assert torch.equal(p8, FL.integral_get_final_preds(final_hm, CENTER, SCALE, beta=8.0)[0]) and not torch.equal(p8, preds)
    want, _, masked = ir.decode(final_hm.cpu(), torch.from_numpy(CENTER), torch.from_numpy(SCALE), BETA)
    fp32 = ir.decode(final_hm.cpu(), torch.from_numpy(CENTER), torch.from_numpy(SCALE), BETA, F32)[0]
    H, W = final_hm.shape[2:]
    s = float(SCALE[:, 0].max()) * 200.0 / W
    (yx, yy), (ex, ey) = axis_errors(fp32, want, ~masked), axis_errors(preds.cpu(), want, ~masked)
    print('predict(decode=integral, flip=%s): x %.3g image px (fp32 %.3g, floor %.3g)  y %.3g (fp32 %.3g, floor %.3g)'
          % (flip, ex, yx, ir.FLOOR * W * s, ey, yy, ir.FLOOR * H * s))
    assert (~masked).any() and ex <= bound(yx, ir.FLOOR * W * s) and ey <= bound(yy, ir.FLOOR * H * s)
