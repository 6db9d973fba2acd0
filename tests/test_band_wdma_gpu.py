"""The weight-DMA form of the f32 split-product band kernel (csrc/conv_t4.hip, WD instances: the pre-split weight image goes
global -> LDS by DMA into two weight buffers) against the register form it replaces (every workgroup splits its f32 weight
fragments), bit for bit, and against the exact fp64 reference on integer operands.

fami_conv_tune_lds(102040 / 102041) selects the register / DMA form, 7000 keeps the persistent kernel (conv_t5.hip) out of
the way; fami_conv_t4_s3_plan says which form a launch takes and is asserted before the launch it describes.  Every output
is a view between 4096-element guard zones (tests/_conv_exact.Arena), every operand sits inside NaN."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from _conv_exact import EXACT32, Arena, Runner, make_case

pytestmark = pytest.mark.gpu

OFF, ON = 102040, 102041
LDS_CAP = 160 * 1024
F32 = torch.float32

# (N, H, W, Ci, Co), extra tune codes, the plan the launch must have (tiles per band, pixel tiles per wave): the smallest
# geometries that reach each branch of the DMA form.  FILL0 switches the band-filling rule off: by default a launch of fewer than
# 128 workgroups is cut into one-tile bands, in which only wave 0 multiplies and no instance of three tiles per wave is reached.
FILL0 = 102000
BRANCHES = [((2, 12, 9, 16, 48), (FILL0,), 7, 2),       # one chunk: the prologue copy only; seven waves multiply
            ((2, 12, 9, 48, 48), (FILL0,), 7, 2),       # three chunks: each buffer reused once
            ((2, 12, 9, 48, 48), (), 1, 2),             # the same on the default route: the fill rule's one-tile bands
            ((1, 5, 7, 80, 96), (FILL0,), 3, 2),        # odd chunk count, two channel blocks, a ragged last tile
            ((1, 1, 1, 16, 48), (), 1, 2),              # a single pixel
            ((3, 9, 12, 64, 64), (FILL0,), 7, 2),       # the NT = 4 instance
            ((2, 24, 18, 32, 144), (100 + 4,), 4, 2),   # forced 4-tile bands: seven bands, the last ragged, three channel blocks
            ((1, 40, 40, 48, 48), (FILL0,), 20, 3)]     # 100 tiles per frame in five bands of 20: the three-tiles-per-wave instance


def _L():
    from fami_pose_amd._lib import lib
    return lib()


def _plan(L, N, H, W, Ci, Co, dil=1, sgn=1, xbn=0):
    """-> (form, LDS bytes of the register form, LDS bytes the DMA form needs, tiles per band, pixel tiles per wave)"""
    out = (ctypes.c_long * 5)()
    form = L.cdll.fami_conv_t4_s3_plan(N, H, W, Ci, Co, dil, sgn, xbn, out)
    return form, out[0], out[1], out[2], out[3]


def _route(L, code, extra=()):
    L.cdll.fami_conv_tune_lds(-1)
    L.cdll.fami_conv_tune_lds(7000)
    for e in extra:
        L.cdll.fami_conv_tune_lds(e)
    L.cdll.fami_conv_tune_lds(code)


class _Ops:
    """random f32 operands of one geometry (all three bf16 terms of every value are non-zero), packed weights of both modes"""

    def __init__(self, dev, geo, dil=1, seed=0, nan_weights=False):
        L = _L()
        N, H, W, Ci, Co = geo
        g = torch.Generator().manual_seed(seed * 7919 + N * 1000003 + H * 10007 + W * 101 + Ci * 17 + Co)
        self.L, self.dev, self.geo = L, dev, geo
        self.g10 = (N, H, W, Ci, Co, 3, 3, 1, dil, dil)
        self.st = torch.cuda.current_stream(dev).cuda_stream
        A = self.A = Arena(dev)
        r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
        self.x, self.dy = A.operand(r(N, H, W, Ci), F32), A.operand(r(N, H, W, Co), F32)
        self.bias = A.operand(r(Co), F32)
        self.y0, self.dx0 = r(N, H, W, Co), r(N, H, W, Ci)
        w = A.operand(r(Co, Ci, 3, 3) * 0.1, F32)
        self.wp = []
        for m in (0, 1):
            wp = A.poisoned(L.cdll.fami_packed_weight_elems(Co, Ci, 3, 3, m), F32)
            if not nan_weights:
                L.call('fami_pack_conv_weight_f32', w.data_ptr(), wp.data_ptr(), Co, Ci, 3, 3, m, self.st)
            self.wp.append(wp)
        torch.cuda.synchronize(dev)

    def fwd(self, bias=0, relu=0, acc=0):
        N, H, W, Ci, Co = self.geo
        self.A.outs = []
        y = self.A.output((N, H, W, Co), F32, self.y0 if acc else None, 'y')
        self.L.call('fami_conv2d_fwd_f32', self.x.data_ptr(), self.wp[0].data_ptr(), self.bias.data_ptr() if bias else None, None,
                    y.data_ptr(), *self.g10, relu, acc, self.st)
        torch.cuda.synchronize(self.dev)
        assert not self.A.touched(), self.A.touched()
        return y

    def dgrad(self, acc=0):
        N, H, W, Ci, Co = self.geo
        self.A.outs = []
        dx = self.A.output((N, H, W, Ci), F32, self.dx0 if acc else None, 'dx')
        self.L.call('fami_conv2d_dgrad_f32', self.dy.data_ptr(), self.wp[1].data_ptr(), None, dx.data_ptr(), *self.g10, acc, self.st)
        torch.cuda.synchronize(self.dev)
        assert not self.A.touched(), self.A.touched()
        return dx


def _same(a, b, what):
    assert not bool(torch.isnan(a).any()), what
    assert torch.equal(a, b), what


@pytest.mark.parametrize('geo,extra,bt,mts', BRANCHES)
def test_dma_form_is_bitwise_the_register_form(dev, geo, extra, bt, mts):
    """1. forward (bias, ReLU, accumulate on and off) and input gradient (accumulate on and off) under both codes"""
    L = _L()
    N, H, W, Ci, Co = geo
    try:
        ops = _Ops(dev, geo)
        res = {}
        for code in (OFF, ON):
            _route(L, code, extra)
            pl = _plan(L, N, H, W, Ci, Co)
            assert (pl[0], pl[3], pl[4]) == (2 if code == ON else 1, bt, mts), (geo, code, pl)
            assert _plan(L, N, H, W, Co, Ci, 1, -1)[0] in ((0, 2) if code == ON else (0, 1)), (geo, code)
            out = {}
            for bias in (0, 1):
                for relu in (0, 1):
                    for acc in (0, 1):
                        out['fwd', bias, relu, acc] = ops.fwd(bias, relu, acc)
            for acc in (0, 1):
                out['dgrad', acc] = ops.dgrad(acc)
            res[code] = out
        for k in res[OFF]:
            _same(res[ON][k], res[OFF][k], (geo, k))
    finally:
        L.cdll.fami_conv_tune_lds(-1)


@pytest.mark.parametrize('geo', [(2, 12, 9, 48, 216), (2, 12, 9, 48, 108)])
def test_partial_channel_block(dev, geo):
    """2. dilation 3, the dilated route forced: the last 48-wide channel block has a tile that the weight fills only in part (its
    other rows are the image's zeros and come through the DMA: held here, channel by channel) and tiles past the weight's last
    one, which the DMA never copies.  What the prologue's zeros in those tiles buy cannot be seen in an output: the plain
    epilogue, the only one of the dilated route, stores no tile past Co, so their accumulators go nowhere.  The launch of another
    layer with NaN weights immediately before leaves NaN in both LDS weight buffers of the CUs; it holds that nothing of that
    reaches the tiles that ARE stored -- a copy landing a block late or a fragment read past its block would."""
    L = _L()
    N, H, W, Ci, Co = geo
    try:
        ops = _Ops(dev, geo, dil=3)
        other = _Ops(dev, (N, H, W, Ci, 240), dil=3, seed=1, nan_weights=True)
        res = {}
        for code in (OFF, ON):
            _route(L, code, (42,))
            assert _plan(L, N, H, W, Ci, Co, 3)[:1] + _plan(L, N, H, W, Ci, Co, 3)[3:] == (2 if code == ON else 1, 7, 2), (geo, code)
            assert _plan(L, N, H, W, Ci, 240, 3)[0] == (2 if code == ON else 1), (geo, code)
            out = {}
            for bias in (0, 1):
                for relu in (0, 1):
                    assert bool(torch.isnan(other.fwd()).all())
                    out[bias, relu] = ops.fwd(bias, relu, 0)
            res[code] = out
        for k in res[OFF]:
            _same(res[ON][k], res[OFF][k], (geo, k))
    finally:
        L.cdll.fami_conv_tune_lds(-1)


def _xbn(r, code):
    """fami_conv2d_fwd_xbn_f32 on the Runner's integer operands: the input statistics say mean 0, variance 1 (eps 0, gamma 1), so
    the staged tensor is relu(z + beta) exactly -> y, the slot rows of the statistics epilogue, the published mean / invstd"""
    c, L, A = r.c, r.L, r.A
    N, H, W, Ci, Co = c.geo[:5]
    P = 1024
    nb = L.cdll.fami_bn_slots_bytes(Ci)
    xs = torch.zeros(nb // 8, dtype=torch.float64)
    xs[Ci:2 * Ci] = float(P)                      # row 0: sum 0, sum of squares P; the pivots (behind the rows) 0
    xslots = A.operand(xs, torch.float64)
    r._begin()
    y = r._act((N, H, W, Co), None, 'y')
    slots = r._slots(Co, 'slots')
    mean, invstd = A.output((Ci,), F32, None, 'mean'), A.output((Ci,), F32, None, 'invstd')
    L.call('fami_conv2d_fwd_xbn_f32', r.z.data_ptr(), r.wp[0].data_ptr(), r.bias.data_ptr(), y.data_ptr(), N, H, W, Ci, Co,
           slots.data_ptr(), r.pivot.data_ptr(), xslots.data_ptr(), P, r.one.data_ptr(), r.beta.data_ptr(), mean.data_ptr(),
           invstd.data_ptr(), None, None, 0.0, 0.0, r.st)
    torch.cuda.synchronize(r.dev)
    xin = (c.z + c.beta).clamp(min=0)
    wy = F.conv2d(xin.permute(0, 3, 1, 2), c.w, c.bias, 1, 1, 1).permute(0, 2, 3, 1).contiguous()
    dlt = wy.reshape(-1, Co) - c.pivot
    s1, s2 = dlt.sum(0), (dlt * dlt).sum(0)
    assert s2.max().item() < EXACT32 and dlt.abs().sum(0).max().item() < EXACT32       # every fp32 partial sum is exact
    rows = r._rows(slots, Co)
    tag = 'fwd_xbn(%d)' % code
    fails = r._end([(tag + ' y', y, wy, '(n,h,w,c)'), (tag + ' sum(y - pivot)', rows[0], s1, '(c,)'),
                    (tag + ' sum((y - pivot)^2)', rows[1], s2, '(c,)'),
                    (tag + ' mean', mean, torch.zeros(Ci, dtype=torch.float64), '(c,)'),
                    (tag + ' invstd', invstd, torch.ones(Ci, dtype=torch.float64), '(c,)')])
    return fails, (y, rows)


@pytest.mark.parametrize('geo', [(2, 12, 9, 48, 48), (2, 12, 9, 96, 96)])
def test_epilogues_and_xbn_exact(dev, geo):
    """3. + 4. the forward statistics epilogue, the input gradient's BatchNorm-backward epilogue (ReLU modes 0 / 1 / 2) and the
    input BatchNorm applied while staging, on integer operands under both codes: outputs and slot rows equal the exact fp64
    reference under either code (integer sums: the order of the atomics does not matter), hence each other"""
    L = _L()
    c = make_case(tuple(geo) + (3, 1, 1, 1))
    N, H, W, Ci, Co = geo
    try:
        r = Runner(dev, 'f32', c)
        fails, xb = [], {}
        for code in (OFF, ON):
            _route(L, code, (FILL0,))
            pl = _plan(L, N, H, W, Ci, Co, 1, 1, 1)
            assert (pl[0], pl[3], pl[4]) == (2 if code == ON else 1, 7, 2), (geo, code, pl)
            assert L.cdll.fami_conv2d_xbn_ok_f32(N, H, W, Ci, Co) == 1
            for bias, piv in ((0, 0), (1, 1)):
                fails += r.fwd_stats(bias, piv)
            for relu in (0, 1, 2):
                for acc in (0, 1):
                    fails += r.dgrad_bnstats(relu, acc)
            f, xb[code] = _xbn(r, code)
            fails += f
        assert not fails, '\n'.join(fails)
        _same(xb[ON][0], xb[OFF][0], (geo, 'xbn y'))
        assert torch.equal(xb[ON][1], xb[OFF][1]), (geo, 'xbn slot rows')
    finally:
        L.cdll.fami_conv_tune_lds(-1)


@pytest.mark.parametrize('geo,extra,bt,mts', BRANCHES)
def test_dma_form_exact_on_integers(dev, geo, extra, bt, mts):
    """4. the branch geometries on integer operands under the DMA form: forward and input gradient equal the fp64 reference"""
    L = _L()
    N, H, W, Ci, Co = geo
    try:
        r = Runner(dev, 'f32', make_case(tuple(geo) + (3, 1, 1, 1)))
        _route(L, ON, extra)
        pl = _plan(L, N, H, W, Ci, Co)
        assert (pl[0], pl[3], pl[4]) == (2, bt, mts), (geo, pl)
        fails = r.fwd() + r.fwd(1, 1, 1, 0) + r.fwd(1, 0, 0, 1) + r.dgrad() + r.dgrad(1, 1)
        assert not fails, '\n'.join(fails)
    finally:
        L.cdll.fami_conv_tune_lds(-1)


@pytest.mark.parametrize('geo,dil', [((2, 12, 9, 8, 48), 1), ((1, 96, 72, 48, 216), 3)])
def test_fallbacks_keep_the_register_form(dev, geo, dil):
    """5. launches that cannot take the DMA form -- no pre-split image (8 input channels), no room for two weight buffers beside
    the band the plan chose (the dilated 48 -> 216 predictor on a 96x72 map) -- are planned as the register form with the switch
    on, with the band they have with it off, and their results on integer operands equal the exact fp64 reference"""
    L = _L()
    N, H, W, Ci, Co = geo
    try:
        r = Runner(dev, 'f32', make_case(tuple(geo) + (3, 1, dil, dil)))
        plans = {}
        for code in (OFF, ON):
            _route(L, code, (42, FILL0))
            plans[code] = _plan(L, N, H, W, Ci, Co, dil)
        assert plans[ON] == plans[OFF] and plans[ON][0] == 1 and plans[ON][1] <= LDS_CAP, plans
        if dil == 3:
            assert plans[ON][2] > LDS_CAP, plans          # the planner's LDS sum of the DMA form: over 160 KiB
        fails = r.fwd(1, 0, 1, 0) + r.fwd(0, 0, 0, 1)     # (under 102041, the route set last)
        assert not fails, '\n'.join(fails)
    finally:
        L.cdll.fami_conv_tune_lds(-1)
