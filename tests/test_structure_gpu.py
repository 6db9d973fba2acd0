"""The structure (limb-direction cosine) kernels on the MI355X (csrc/loss.hip: fami_structure_cos_fwd_f32 / _bwd_f32) with
loss.StructureCosineSimilarity and loss.limb_cosines on top.

Kernel launches go through the C ABI: operands uploaded inside NaN, outputs between guard zones (tests/_stream_exact.Run).

Bounds.  Row values and gcoords are held to the float64 restatement (tests/_structure_ref.py) rounded to fp32.  Every step of
either side is an IEEE float64 operation on identical fp32 inputs in the same order, so equal bits are expected; the ASSERTED
bound is one fp32 ulp of the value, which is what a last-place difference in the float64 sqrt or quotient could move the single
fp32 rounding by.  Each case prints how many entries were not bit-equal (recorded in
profiles/structure/test_structure_gpu.txt).  The loss is scale x the float64 sum of the fp32 row
values: 1e-6 relative (one fp32 rounding, 6e-8, and the order of a float64 sum).  Everything else is bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _structure_ref as sr  # noqa: E402
from _stream_exact import F32, F64, Run, ptr  # noqa: E402

from fami_pose_amd import loss as FL  # noqa: E402
from fami_pose_amd.data import LIMB_PAIRS  # noqa: E402

pytestmark = pytest.mark.gpu
MIN_LEN, EPS = 1.0, 1e-8


def _case(name):
    """-> coords, txy [B,J,2] fp32, w [B,J] fp32, pairs"""
    if name == 'one-limb':
        c, t, w = sr.skeleton_case(1, 2, ((1, 0),), 1)
        return c, t, w, ((1, 0),)
    if name == 'posetrack':
        c, t, w = sr.skeleton_case(2, 17, LIMB_PAIRS, 2)
        w[0, 7] = 0.0                        # the left elbow of sample 0: limbs (5,7) and (7,9) drop out
        w[1, 3] = w[1, 4] = 0.0              # the ears are on no limb: nothing changes
        t[1, 16] = t[1, 14] + np.float32(0.5)          # a target limb shorter than min_len
        c[1, 1] = c[1, 0]                    # a predicted limb of length 0: the clamp branch
        return c, t, w, LIMB_PAIRS
    if name == 'caps':
        pairs = sr.star_pairs()
        c, t, w = sr.skeleton_case(3, 64, pairs, 3)
        w[2, 50] = 0.0
        return c, t, w, pairs
    if name == 'masked-sample':
        c, t, w = sr.skeleton_case(3, 17, LIMB_PAIRS, 4)
        w[1] = 0.0                           # every limb of sample 1 is masked
        return c, t, w, LIMB_PAIRS
    raise KeyError(name)


CASES = ['one-limb', 'posetrack', 'caps', 'masked-sample']


def _within_one_ulp(tag, got, want64):
    """got (device fp32) against the float64 reference: -> (entries not bit-equal to the rounded reference, failure text or None)"""
    g = got.detach().cpu().numpy().astype(np.float64).reshape(want64.shape)
    w32 = want64.astype(np.float32)
    differ = int((g.astype(np.float32).view(np.int32) != w32.view(np.int32)).sum())
    err = np.abs(g - w32.astype(np.float64))
    bad = ~(err <= sr.ulp32(w32.astype(np.float64)))          # (a NaN fails)
    if bad.any():
        i = tuple(int(k[0]) for k in np.nonzero(bad))
        return differ, '%s: %d entries beyond one fp32 ulp, first at %s: kernel %r, reference %r' % (tag, int(bad.sum()), i, g[i], w32[i])
    return differ, None


@pytest.mark.parametrize('name', CASES)
def test_rows_loss_and_gcoords_against_the_restatement(dev, name):
    c, t, w, pairs = _case(name)
    B, J, P = c.shape[0], c.shape[1], len(pairs)
    scale, gs, g0 = 0.75 / (B * P), 0.375, 4.0
    want_rows = sr.rows(c, t, w, pairs, MIN_LEN, EPS)
    want_g = sr.gcoords(c, t, w, pairs, gs, None, MIN_LEN, EPS)
    valid = sr.limbs(c, t, w, pairs, MIN_LEN, EPS)[0]
    assert valid.any() and (name == 'one-limb' or (~valid).any())
    if name == 'masked-sample':
        assert not valid[1].any() and not want_g[1].any()
    if name == 'caps':
        assert valid[:, :40].all()          # joint 0 sums 40 limbs

    R = Run(dev)
    T = torch.from_numpy
    cd, td, wd = R.op(T(c).double(), F32), R.op(T(t).double(), F32), R.op(T(w).double(), F32)
    pd = R.ints(torch.tensor(pairs, dtype=torch.int32).reshape(-1, 2), 'pairs')
    outs = {}
    for tag, wp in (('w', wd), ('NULL', None)):
        loss, ws = R.out((1,), F32, None, 'loss ' + tag), R.out((B * P,), F32, None, 'row values ' + tag)
        R.call('fami_structure_cos_fwd_f32', ptr(cd), ptr(td), ptr(wp), ptr(pd), ptr(loss), B, J, P, MIN_LEN, EPS, scale, ptr(ws), R.st)
        g = R.out((B * J, 2), F32, None, 'gcoords ' + tag)
        R.call('fami_structure_cos_bwd_f32', ptr(cd), ptr(td), ptr(wp), ptr(pd), ptr(g), B, J, P, MIN_LEN, EPS, gs, None, R.st)
        outs[tag] = (loss, ws, g)
    # a second run, and gdev = 4 against scale * 4
    loss2, ws2, g2 = R.out((1,), F32, None, 'loss again'), R.out((B * P,), F32, None, 'row values again'), R.out((B * J, 2), F32, None, 'gcoords again')
    R.call('fami_structure_cos_fwd_f32', ptr(cd), ptr(td), ptr(wd), ptr(pd), ptr(loss2), B, J, P, MIN_LEN, EPS, scale, ptr(ws2), R.st)
    R.call('fami_structure_cos_bwd_f32', ptr(cd), ptr(td), ptr(wd), ptr(pd), ptr(g2), B, J, P, MIN_LEN, EPS, gs, None, R.st)
    gdev = R.op(torch.tensor([g0], dtype=F64), F32)
    g_dev, g_host = R.out((B * J, 2), F32, None, 'gcoords gdev'), R.out((B * J, 2), F32, None, 'gcoords scale * 4')
    R.call('fami_structure_cos_bwd_f32', ptr(cd), ptr(td), ptr(wd), ptr(pd), ptr(g_dev), B, J, P, MIN_LEN, EPS, gs, ptr(gdev), R.st)
    R.call('fami_structure_cos_bwd_f32', ptr(cd), ptr(td), ptr(wd), ptr(pd), ptr(g_host), B, J, P, MIN_LEN, EPS, gs * g0, None, R.st)
    # w = 1 everywhere, uploaded, against w = NULL
    ones = R.op(torch.ones(B, J, dtype=F64), F32)
    loss1, ws1, g1 = R.out((1,), F32, None, 'loss w=1'), R.out((B * P,), F32, None, 'row values w=1'), R.out((B * J, 2), F32, None, 'gcoords w=1')
    R.call('fami_structure_cos_fwd_f32', ptr(cd), ptr(td), ptr(ones), ptr(pd), ptr(loss1), B, J, P, MIN_LEN, EPS, scale, ptr(ws1), R.st)
    R.call('fami_structure_cos_bwd_f32', ptr(cd), ptr(td), ptr(ones), ptr(pd), ptr(g1), B, J, P, MIN_LEN, EPS, gs, None, R.st)
    torch.cuda.synchronize(dev)

    loss, ws, g = outs['w']
    fails = []
    n_rows, f = _within_one_ulp('row values', ws, want_rows.reshape(-1))
    fails += [f] if f else []
    n_g, f = _within_one_ulp('gcoords', g, want_g.reshape(-1, 2))
    fails += [f] if f else []
    n_gd, f = _within_one_ulp('gcoords under gdev', g_dev, sr.gcoords(c, t, w, pairs, gs, g0, MIN_LEN, EPS).reshape(-1, 2))
    fails += [f] if f else []
    n_r1, f = _within_one_ulp('row values, w = NULL', outs['NULL'][1], sr.rows(c, t, None, pairs, MIN_LEN, EPS).reshape(-1))
    fails += [f] if f else []
    n_g1, f = _within_one_ulp('gcoords, w = NULL', outs['NULL'][2], sr.gcoords(c, t, None, pairs, gs, None, MIN_LEN, EPS).reshape(-1, 2))
    fails += [f] if f else []
    l64 = sr.loss(ws.cpu().numpy(), scale)
    el = abs(loss.item() - l64) / abs(l64)
    print('%s (B %d, J %d, P %d): not bit-equal to the rounded restatement: %d of %d row values, %d of %d gcoords (gdev: %d; w = NULL: '
          '%d rows, %d gcoords); loss %.3g relative' % (name, B, J, P, n_rows, B * P, n_g, 2 * B * J, n_gd, n_r1, n_g1, el))
    assert el <= 1e-6
    R.want_bits('a second run, row values', ws2, ws.cpu())
    R.want_bits('a second run, loss', loss2, loss.cpu())
    R.want_bits('a second run, gcoords', g2, g.cpu())
    R.want_bits('gdev = 4 against scale * 4', g_dev, g_host.cpu())
    R.want_bits('w = NULL against w = 1, row values', outs['NULL'][1], ws1.cpu())
    R.want_bits('w = NULL against w = 1, loss', outs['NULL'][0], loss1.cpu())
    R.want_bits('w = NULL against w = 1, gcoords', outs['NULL'][2], g1.cpu())
    fails += R.end()
    assert not fails, '\n'.join(fails)


def test_refusals_write_nothing(dev):
    c, t, w, pairs = _case('posetrack')
    B, J, P = 2, 17, 16
    R = Run(dev)
    T = torch.from_numpy
    cd, td, wd = R.op(T(c).double(), F32), R.op(T(t).double(), F32), R.op(T(w).double(), F32)
    pd = R.ints(torch.tensor(pairs, dtype=torch.int32).reshape(-1, 2), 'pairs')
    loss, ws, g = R.out((1,), F32, None, 'refused loss'), R.out((B * 64,), F32, None, 'refused row values'), R.out((B * 64, 2), F32, None, 'refused gcoords')
    nan, inf = float('nan'), float('inf')

    def both(Bb=B, Jb=J, Pb=P, ml=MIN_LEN, eps=EPS, cp=cd, tp=td, pp=pd, lp=loss, wsp=ws, gp=g):
        R.refused('fami_structure_cos_fwd_f32', ptr(cp), ptr(tp), ptr(wd), ptr(pp), ptr(lp), Bb, Jb, Pb, ml, eps, 1.0, ptr(wsp), R.st)
        R.refused('fami_structure_cos_bwd_f32', ptr(cp), ptr(tp), ptr(wd), ptr(pp), ptr(gp), Bb, Jb, Pb, ml, eps, 1.0, None, R.st)
    for kw in (dict(Bb=0), dict(Bb=-1), dict(Jb=0), dict(Jb=1), dict(Jb=65), dict(Pb=0), dict(Pb=65), dict(Pb=-3), dict(ml=-0.5), dict(ml=nan),
               dict(ml=inf), dict(eps=0.0), dict(eps=-1e-8), dict(eps=nan), dict(eps=inf), dict(cp=None), dict(tp=None), dict(pp=None),
               dict(lp=None, gp=None), dict(wsp=None, gp=None)):
        both(**kw)
    for tns, name in ((loss, 'loss'), (ws, 'row values'), (g, 'gcoords')):
        R.want_untouched('refused ' + name, tns)
    fails = R.end()
    assert not fails, '\n'.join(fails)


def test_module_gradient_is_the_two_launches(dev):
    """StructureCosineSimilarity on a [2,17,24,18] map: the value against the restatement on the module's own coordinates, the
    gradient against the restatement's gcoords (rounded to fp32) pushed through loss.soft_argmax's backward -- the same two
    launches, so bit for bit wherever the gcoords are."""
    B, J, H, W = 2, 17, 24, 18
    g = torch.Generator().manual_seed(12)
    hm = torch.rand(B, J, H, W, generator=g) * 0.2
    peaks = torch.stack([torch.randint(2, W - 2, (B, J), generator=g), torch.randint(2, H - 2, (B, J), generator=g)], -1)
    for b in range(B):
        for j in range(J):
            hm[b, j, peaks[b, j, 1], peaks[b, j, 0]] += 1.0
    txy = (peaks.float() + torch.randn(B, J, 2, generator=g)).contiguous()
    w = torch.ones(B, J, 1)
    w[0, 9] = 0.0
    pred = hm.to(dev).requires_grad_(True)
    crit = FL.StructureCosineSimilarity()
    val = crit(pred, txy.to(dev), w.to(dev))
    (val * 3.0).backward()
    p2 = hm.to(dev).requires_grad_(True)
    coords = FL.soft_argmax(p2)
    cn, tn, wn = coords.detach().cpu().numpy(), txy.numpy(), w.reshape(B, J).numpy()
    valid = sr.limbs(cn, tn, wn, LIMB_PAIRS)[0]
    assert valid.sum() > 16 and not valid.all()
    P = len(LIMB_PAIRS)
    want_rows = sr.rows(cn, tn, wn, LIMB_PAIRS).astype(np.float32)
    l64 = sr.loss(want_rows, 1.0 / (B * P))
    print('StructureCosineSimilarity: value %.8g, restatement %.8g' % (val.item(), l64))
    assert l64 > 0 and abs(val.item() - l64) <= 1e-6 * l64
    gc = sr.gcoords(cn, tn, wn, LIMB_PAIRS, 1.0 / (B * P), 3.0).astype(np.float32)
    coords.backward(torch.from_numpy(gc).to(dev))
    differ = int((pred.grad != p2.grad).sum())
    print('module gradient against the restatement through soft_argmax: %d of %d entries differ' % (differ, pred.grad.numel()))
    assert torch.equal(pred.grad, p2.grad) and pred.grad.abs().max().item() > 0
    assert (pred.grad[0, 9] == 0).all()          # joint 9 of sample 0 is on one limb, and that limb is masked
    # limb_cosines: 1 - the row values, NaN where not valid
    cosv = FL.limb_cosines(coords.detach(), txy.to(dev), w.to(dev)).cpu().numpy()
    assert cosv.shape == (B, P) and np.array_equal(np.isnan(cosv), ~valid)
    assert np.array_equal(cosv[valid], (np.float32(1.0) - want_rows)[valid])
    # use_target_weight=False: the masked limb counts again
    v2 = FL.StructureCosineSimilarity(use_target_weight=False)(hm.to(dev), txy.to(dev), w.to(dev))
    l2 = sr.loss(sr.rows(cn, tn, None, LIMB_PAIRS).astype(np.float32), 1.0 / (B * P))
    assert abs(v2.item() - l2) <= 1e-6 * l2 and l2 != l64

