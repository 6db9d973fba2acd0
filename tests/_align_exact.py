"""Helpers of tests/test_align_exact_gpu.py: operands for which every result of csrc/align.hip is independent of the order of
any sum, the exact fp64 references (CPU), and the launches of the exported entry points through the C ABI into guarded buffers
(tests/_conv_exact.Arena).

Why the results are fully determined:
  x, dy, weights      small integers
  offsets             integers and half-integers: the 1-D bilinear weights are 0, 1/2 or 1, their products multiples of 1/4
  masks               +-2^k, 1/4 .. 4, and some +-16 (beyond the fixed-point bound of the backward's LDS scatter)
  shift translations  half-integers
so a modulated sample is a multiple of 2^-4 with a handful of significant bits (representable in bf16 and fp16: the 16-bit
kernels round it to the storage type before the matrix core), every product a kernel forms is exact in fp32, every fp32 sum stays
below 2^24 units of its last place in any order, and every fixed-point contribution of the backward's input-gradient scatter is a
multiple of the region's resolution.  These conditions are asserted here on the CPU, in fp64, before any launch (assert_exact);
none of them is a tolerance.  A value stored in a 16-bit type is the fp64 reference rounded once."""
import functools
import math

import torch

from _conv_exact import Arena, DT, mismatch, out_dim          # noqa: F401  (re-exported for the test file)

EXACT32 = 2 ** 24
MASK_BOUND = 8.0          # DCN_MASK_BOUND of align.hip
U_COL, U_OFF = 4, 5       # modulated samples / input-gradient contributions are multiples of 2^-4, offset gradients of 2^-5


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g, dtype=torch.int64).double()


def _pick(g, shape, values, probs):
    idx = torch.multinomial(torch.tensor(probs, dtype=torch.float64), int(torch.tensor(shape).prod()), True, generator=g)
    return torch.tensor(values, dtype=torch.float64)[idx].view(shape)


def _multiple(t, bits):
    s = t * 2.0 ** bits
    return bool((s == s.round()).all())


class DcnCase:
    """One geometry (B, H, W, C, G, Co, k, stride, pad, dil): operands and fp64 references, NHWC, offsets ordered (group, tap,
    (dy, dx)), weights OIHW."""

    def __init__(self, geo):
        self.geo = tuple(geo)
        B, H, W, C, G, Co, k, s, p, d = geo
        K, cg = k * k, C // G
        self.K, self.cg = K, cg
        self.Ho, self.Wo = out_dim(H, k, s, p, d), out_dim(W, k, s, p, d)
        Ho, Wo = self.Ho, self.Wo
        self.P = B * Ho * Wo
        g = torch.Generator().manual_seed(20240 + sum((i + 3) * int(v) * 131 for i, v in enumerate(geo)))
        self.x, self.dy = _ints(g, (B, H, W, C), -2, 2), _ints(g, (B, Ho, Wo, Co), -2, 2)
        self.w, self.bias = _ints(g, (Co, C, k, k), -2, 2), _ints(g, (Co,), -4, 4)
        # offsets: mostly within the LDS regions' reach of 3 pixels, some beyond it (global-atomic path), some far outside the map
        small = [v / 2.0 for v in range(-5, 6)]
        beyond = [-5.0, -4.5, -3.5, 3.5, 4.5, 5.0]
        far = [-20.5, -14.0, 13.5, 20.0]
        vals = small + beyond + far
        probs = [0.72 / len(small)] * len(small) + [0.16 / len(beyond)] * len(beyond) + [0.12 / len(far)] * len(far)
        self.off = _pick(g, (B, Ho, Wo, G, K, 2), vals, probs)
        mvals = [s_ * m for s_ in (-1.0, 1.0) for m in (0.25, 0.5, 1.0, 2.0, 4.0, 16.0)]
        mprobs = [0.09, 0.09, 0.09, 0.09, 0.09, 0.05] * 2
        self.msk = _pick(g, (B, Ho, Wo, G, K), mvals, mprobs)
        self.goff0, self.gmsk0 = _ints(g, (B, Ho, Wo, G, K, 2), -4, 4), _ints(g, (B, Ho, Wo, G, K), -4, 4)
        self.gx0, self.dw0 = _ints(g, (B, H, W, C), -4, 4), _ints(g, (Co, C * K), -4, 4)
        assert (self.off.abs() > 3).any() and (self.off.abs() > 12).any() and (self.msk.abs() == 16).any()

    # ---- layouts of the C ABI
    def off_flat(self):
        return self.off.reshape(self.P, -1)

    def msk_flat(self):
        return self.msk.reshape(self.P, -1)

    def om_flat(self):
        return torch.cat([self.off_flat(), self.msk_flat()], 1)

    @functools.lru_cache(maxsize=None)
    def ref(self, masked):
        """fp64 results with the masks (masked) or with a null mask pointer (mask 1): dict of
        col [P, C*K] in weight.view(Co, C*K) order, y [P, Co], gx [B,H,W,C], goff [P, 2GK], gmsk [P, GK], dw [Co, C*K],
        plus the magnitudes assert_exact needs"""
        B, H, W, C, G, Co, k, s, p, d = self.geo
        K, cg, Ho, Wo, P = self.K, self.cg, self.Ho, self.Wo, self.P
        ar = torch.arange
        oy, ox = ar(Ho).view(1, Ho, 1, 1, 1), ar(Wo).view(1, 1, Wo, 1, 1)
        ky, kx = (ar(K) // k).view(1, 1, 1, 1, K), (ar(K) % k).view(1, 1, 1, 1, K)
        py = (oy * s - p + ky * d).double() + self.off[..., 0]
        px = (ox * s - p + kx * d).double() + self.off[..., 1]
        fy, fx = py.floor(), px.floor()
        ly, lx = py - fy, px - fx
        hy, hx = 1 - ly, 1 - lx
        y0, x0 = fy.long(), fx.long()
        xg = self.x.view(B, H * W, G, cg)
        bi, gi = ar(B).view(B, 1, 1, 1, 1), ar(G).view(1, 1, 1, G, 1)

        def corner(yc, xc):
            valid = ((yc >= 0) & (yc < H) & (xc >= 0) & (xc < W))
            idx = yc.clamp(0, H - 1) * W + xc.clamp(0, W - 1)
            return xg[bi, idx, gi] * valid.unsqueeze(-1), valid.double(), idx          # [B,Ho,Wo,G,K,cg]

        (a00, v00, i00), (a01, v01, i01) = corner(y0, x0), corner(y0, x0 + 1)
        (a10, v10, i10), (a11, v11, i11) = corner(y0 + 1, x0), corner(y0 + 1, x0 + 1)
        w00, w01, w10, w11 = hy * hx, hy * lx, ly * hx, ly * lx
        u = lambda t: t.unsqueeze(-1)
        val = a00 * u(w00) + a01 * u(w01) + a10 * u(w10) + a11 * u(w11)
        mk = self.msk if masked else torch.ones_like(self.msk)
        colg = val * u(mk)                                                # [B,Ho,Wo,G,K,cg]
        col = colg.permute(0, 1, 2, 3, 5, 4).reshape(P, C * K)           # column (channel = g*cg + j, tap)
        wm = self.w.reshape(Co, C * K)
        dyf = self.dy.reshape(P, Co)
        y = col @ wm.t() + self.bias
        gcol = (dyf @ wm).view(B, Ho, Wo, G, cg, K).permute(0, 1, 2, 3, 5, 4)          # [B,Ho,Wo,G,K,cg]
        gmsk = (gcol * val).sum(-1)
        gv = gcol * u(mk)
        dpy = u(hx) * (a10 - a00) + u(lx) * (a11 - a01)
        dpx = u(hy) * (a01 - a00) + u(ly) * (a11 - a10)
        goff = torch.stack([(gv * dpy).sum(-1), (gv * dpx).sum(-1)], -1)
        gx = torch.zeros(B * H * W, G, cg, dtype=torch.float64)
        contrib_max, gx_abs = 0.0, torch.zeros_like(gx)
        fine = True
        for wgt, vv, idx in ((w00, v00, i00), (w01, v01, i01), (w10, v10, i10), (w11, v11, i11)):
            c_ = gv * u(wgt * vv)
            fine = fine and _multiple(c_, U_COL)
            contrib_max = max(contrib_max, c_.abs().max().item())
            flat = (bi * (H * W) + idx).expand_as(wgt)
            gidx = gi.expand_as(wgt)
            gx.index_put_((flat.reshape(-1), gidx.reshape(-1)), c_.reshape(-1, cg), accumulate=True)
            gx_abs.index_put_((flat.reshape(-1), gidx.reshape(-1)), c_.abs().reshape(-1, cg), accumulate=True)
        dw = dyf.t() @ col
        r = dict(col=col, y=y, gx=gx.view(B, H, W, C), goff=goff.reshape(P, -1), gmsk=gmsk.reshape(P, -1), dw=dw)
        r['_sums'] = dict(
            y=(col.abs() @ wm.abs().t()).max().item() + 4, gcol=(dyf.abs() @ wm.abs()).max().item(),
            gmsk=(gcol * val).abs().sum(-1).max().item(), goff=max((gv * dpy).abs().sum(-1).max().item(), (gv * dpx).abs().sum(-1).max().item()),
            gx=gx_abs.max().item() + 4, dw=(dyf.abs().t() @ col.abs()).max().item() + 4, contrib=contrib_max, contrib_fine=fine,
            off_fine=_multiple(gv * dpy, U_OFF) and _multiple(gv * dpx, U_OFF) and _multiple(gcol * val, U_OFF))
        return r

    def want_goff(self, masked, acc):
        return self.ref(masked)['goff'] + (self.goff0.reshape(self.P, -1) if acc else 0)

    def want_gmsk(self, masked, acc):
        return self.ref(masked)['gmsk'] + (self.gmsk0.reshape(self.P, -1) if acc else 0)


@functools.lru_cache(maxsize=None)
def make_case(geo):
    return DcnCase(geo)


def representable(t, dtype):
    return bool((t.to(dtype).double() == t).all())


def assert_exact(c, dt):
    """The conditions of the module docstring, on the CPU in fp64, for storage type dt: before any launch."""
    dtype = DT[dt]
    B, H, W, C, G, Co, k, s, p, d = c.geo
    for t in (c.x, c.dy, c.w, c.bias, c.off, c.msk, c.goff0, c.gmsk0, c.gx0):
        assert representable(t, dtype), c.geo
    wm = c.w.reshape(Co, -1)
    wnorm = wm.abs().sum(0).max().item()
    for masked in (True, False):
        r = c.ref(masked)
        sums = r['_sums']
        assert representable(r['col'], dtype) and _multiple(r['col'], U_COL), (c.geo, 'a modulated sample is not representable')
        assert sums['contrib_fine'] and sums['off_fine']
        # every fp32 accumulator, in units of its last place (the sum of magnitudes bounds every partial sum in any order)
        assert sums['y'] * 2 ** U_COL < EXACT32 and sums['gcol'] < EXACT32 and sums['dw'] * 2 ** U_COL < EXACT32
        assert sums['gmsk'] * 2 ** U_OFF < EXACT32 and sums['goff'] * 2 ** U_OFF < EXACT32 and sums['gx'] * 2 ** U_COL < EXACT32
        # fixed-point regions: the coarsest per-workgroup resolution, 2^(e - FIXB) with 2^e > max|dy| x bound x max_k sum_co |W|, divides
        # every contribution (FIXB = 30: 64-bit cells, 20: 32-bit cells of the 16-bit types); a smaller tile maximum only refines it
        bound = c.dy.abs().max().item() * (MASK_BOUND if masked else 1.0) * wnorm
        e = math.frexp(bound)[1]
        assert e - 20 <= -U_COL, (c.geo, e)
        assert sums['contrib'] < 2.0 ** 20          # (any contribution, as a multiple of 2^-4, has fewer than 24 significant bits)
    # the deterministic mode: 2^(42 - e) with 2^e > max|dy|
    assert math.frexp(c.dy.abs().max().item())[1] - 42 <= -U_COL


class DcnRunner:
    """One geometry in one storage type on the device: operands uploaded once (inside NaN), weights packed once, one method per
    entry-point family.  Every method launches into fresh guarded outputs, synchronises, and returns the failures as texts."""

    def __init__(self, dev, dt, c):
        from fami_pose_amd._lib import lib
        self.L, self.dev, self.dt, self.c = lib(), dev, dt, c
        self.dtype, self.esz = DT[dt], 4 if dt == 'f32' else 2
        self.st = torch.cuda.current_stream(dev).cuda_stream
        assert_exact(c, dt)
        B, H, W, C, G, Co, k, s, p, d = c.geo
        self.g11 = (B, H, W, C, Co, G, k, k, s, p, d)
        A = self.A = Arena(dev)
        f32 = torch.float32
        self.x, self.dy = A.operand(c.x, self.dtype), A.operand(c.dy, self.dtype)
        self.off, self.msk, self.om = A.operand(c.off_flat(), self.dtype), A.operand(c.msk_flat(), self.dtype), A.operand(c.om_flat(), self.dtype)
        self.bias = A.operand(c.bias, f32)
        w = A.operand(c.w, f32)
        cd = self.L.cdll
        self.L.call('fami_dcn_tune', -1)
        self.wp = A.poisoned(cd.fami_dcn_packed_weight_elems(Co, C, k, k, G), f32)
        self.L.call('fami_dcn_pack_weight_' + dt, w.data_ptr(), self.wp.data_ptr(), Co, C, k, k, G, self.st)
        self.wpb = A.poisoned(cd.fami_dcn_packed_weight_bwd_elems(Co, C, k, k, G), f32)
        self.L.call('fami_dcn_pack_weight_bwd_f32', w.data_ptr(), self.wpb.data_ptr(), Co, C, k, k, G, self.st)
        torch.cuda.synchronize(dev)

    def _end(self, checks):
        torch.cuda.synchronize(self.dev)
        fails = []
        for nm, got, want, axes in checks:
            m = mismatch(got, want, axes)          # (want is rounded to got's type there: once, from fp64)
            if m:
                fails.append('%s: %s' % (nm, m))
        return fails + self.A.touched()

    def _routed(self, codes, fn):
        try:
            for code in codes:
                self.L.call('fami_dcn_tune', code)
            return fn()
        finally:
            self.L.call('fami_dcn_tune', -1)

    def fwd(self, codes=(), om=False, masked=True, bias=True):
        """fami_dcn_fwd_* (masked False: null mask pointer) / fami_dcn_fwd_om_*"""
        c = self.c
        Co = c.geo[5]
        self.A.outs = []
        y = self.A.output((c.P, Co), self.dtype, None, 'y')
        b = self.bias.data_ptr() if bias else None

        def go():
            if om:
                self.L.call('fami_dcn_fwd_om_' + self.dt, self.x.data_ptr(), self.om.data_ptr(), self.wp.data_ptr(), b, y.data_ptr(), *self.g11, self.st)
            else:
                self.L.call('fami_dcn_fwd_' + self.dt, self.x.data_ptr(), self.off.data_ptr(), self.msk.data_ptr() if masked else None,
                            self.wp.data_ptr(), b, y.data_ptr(), *self.g11, self.st)
        self._routed(codes, go)
        want = c.ref(masked or om)['y'] - (0 if bias else c.bias)
        return self._end([('fwd%s(route %s, mask %d, bias %d)' % ('_om' if om else '', list(codes), masked, bias), y, want, '(pixel, co)')])

    def bwd(self, codes=(), om=False, masked=True, acc=0, det=False, acc_x=0, want_gx=True, want_col=True):
        """fami_dcn_bwd_* / _om_* / _det_* / _det_om_*, then the weight gradient from `col` (through fami_dcn_col_dw_unpermute_f32
        where the kernel wrote its own column order)"""
        c = self.c
        B, H, W, C, G, Co, k, s, p, d = c.geo
        K, P = c.K, c.P
        masked = masked or om
        r = c.ref(masked)
        cd = self.L.cdll
        self.A.outs = []
        f32 = torch.float32
        out = {}

        def go():
            colw = cd.fami_dcn_bwd_col_width(C, Co, G, k, k, s, d, self.esz, int(det))
            perm = cd.fami_dcn_bwd_col_permuted(C, Co, G, k, k, s, d, self.esz, int(det))
            assert colw >= C * K and (perm or colw == C * K)
            col = self.A.output((P, colw), self.dtype, None, 'col') if want_col else None
            gxt = self.dtype if det else f32
            gx = self.A.output((B, H, W, C), gxt, c.gx0 if (acc_x or not det) else None, 'gx') if want_gx else None
            if om:
                prior = torch.cat([c.goff0.reshape(P, -1), c.gmsk0.reshape(P, -1)], 1) if acc else None
                gom = self.A.output((P, 3 * G * K), self.dtype, prior, 'gom')
                goff = gmsk = None
            else:
                goff = self.A.output((P, 2 * G * K), self.dtype, c.goff0.reshape(P, -1) if acc else None, 'goff')
                gmsk = self.A.output((P, G * K), self.dtype, c.gmsk0.reshape(P, -1) if acc else None, 'gmsk') if masked else None
            ptr = lambda t: None if t is None else t.data_ptr()
            head = [self.x.data_ptr()] + ([self.om.data_ptr()] if om else [self.off.data_ptr(), self.msk.data_ptr() if masked else None])
            head += [self.dy.data_ptr(), self.wpb.data_ptr(), ptr(col), ptr(gx)] + ([gom.data_ptr()] if om else [ptr(goff), ptr(gmsk)])
            name = 'fami_dcn_bwd%s%s_%s' % ('_det' if det else '', '_om' if om else '', self.dt)
            if det:
                ws = self.A.output((cd.fami_dcn_bwd_det_workspace(B, H, W, C) // 4,), f32, None, 'workspace')
                self.L.call(name, *head, *self.g11, acc, acc_x, ws.data_ptr(), self.st)
            else:
                self.L.call(name, *head, *self.g11, acc, self.st)
            out.update(col=col, gx=gx, perm=perm, colw=colw, name=name)
            if om:
                out.update(goff=gom[:, :2 * G * K], gmsk=gom[:, 2 * G * K:])
            else:
                out.update(goff=goff, gmsk=gmsk)
            if col is not None:
                torch.cuda.synchronize(self.dev)
                colh = col.detach().cpu().double()
                assert not torch.isnan(colh).any(), 'col holds elements the kernel did not write'
                dwp = c.dy.reshape(P, Co).t() @ colh                                  # [Co, colw], exact in fp64 and in fp32
                if perm:
                    dwd = self.A.operand(dwp, f32)
                    dw = self.A.output((Co, C * K), f32, c.dw0 if acc else None, 'dw')
                    self.L.call('fami_dcn_col_dw_unpermute_f32', dwd.data_ptr(), dw.data_ptr(), Co, C, G, k, k, s, d, self.esz, acc, self.st)
                    out.update(dw=dw, dw_want=r['dw'] + (c.dw0 if acc else 0))
                else:
                    out.update(dw=dwp.to(self.dev), dw_want=r['dw'])
        self._routed(codes, go)
        tag = '%s(route %s, mask %d, acc %d, acc_x %d)' % (out['name'], list(codes), masked, acc, acc_x)
        checks = [(tag + ' goff', out['goff'], c.want_goff(masked, acc), '(pixel, 2(g,tap))')]
        if out['gmsk'] is not None:
            checks.append((tag + ' gmsk', out['gmsk'], c.want_gmsk(masked, acc), '(pixel, (g,tap))'))
        if out['gx'] is not None:
            checks.append((tag + ' gx', out['gx'], r['gx'] + (c.gx0 if (acc_x or not det) else 0), '(b,h,w,c)'))
        if out['col'] is not None:
            if not out['perm']:
                checks.append((tag + ' col', out['col'], r['col'], '(pixel, (c,tap))'))
            checks.append((tag + ' dw', out['dw'], out['dw_want'], '(co, (c,tap))'))
        return self._end(checks)


# ------------------------------------------------------------------ bilinear shift
class ShiftCase:
    def __init__(self, geo):
        self.geo = B, H, W, C = tuple(geo)
        g = torch.Generator().manual_seed(777 + B * 1000 + H * 100 + W * 10 + C)
        self.src, self.gout = _ints(g, (B, H, W, C), -3, 3), _ints(g, (B, H, W, C), -2, 2)
        self.t = torch.tensor([[0.5, -1.5], [-2.5, 3.0], [0.0, 0.5], [12.5, -0.5]], dtype=torch.float64)[:B].contiguous()      # (tx, ty) per sample
        self.gsrc0, self.gt0 = _ints(g, (B, H, W, C), -4, 4), _ints(g, (B, 2), -4, 4)
        ar = torch.arange
        py = ar(H).view(1, H, 1).double() - self.t[:, 1].view(B, 1, 1)
        px = ar(W).view(1, 1, W).double() - self.t[:, 0].view(B, 1, 1)
        py, px = py.expand(B, H, W), px.expand(B, H, W)
        fy, fx = py.floor(), px.floor()
        ly, lx = py - fy, px - fx
        hy, hx = 1 - ly, 1 - lx
        y0, x0 = fy.long(), fx.long()
        bi = ar(B).view(B, 1, 1)
        sf = self.src.view(B, H * W, C)
        self.out = torch.zeros(B, H, W, C, dtype=torch.float64)
        self.gsrc = torch.zeros(B * H * W, C, dtype=torch.float64)
        v = []
        for dy_, dx_, wgt in ((0, 0, hy * hx), (0, 1, hy * lx), (1, 0, ly * hx), (1, 1, ly * lx)):
            yc, xc = y0 + dy_, x0 + dx_
            valid = ((yc >= 0) & (yc < H) & (xc >= 0) & (xc < W)).double()
            idx = yc.clamp(0, H - 1) * W + xc.clamp(0, W - 1)
            a = sf[bi, idx] * valid.unsqueeze(-1)
            v.append(a)
            self.out += a * wgt.unsqueeze(-1)
            self.gsrc.index_put_(((bi * H * W + idx).reshape(-1),), (self.gout * (wgt * valid).unsqueeze(-1)).reshape(-1, C), accumulate=True)
        self.gsrc = self.gsrc.view(B, H, W, C)
        u = lambda t_: t_.unsqueeze(-1)
        dpy = u(hx) * (v[2] - v[0]) + u(lx) * (v[3] - v[1])
        dpx = u(hy) * (v[1] - v[0]) + u(ly) * (v[3] - v[2])
        self.gt = torch.stack([-(self.gout * dpx).sum((1, 2, 3)), -(self.gout * dpy).sum((1, 2, 3))], 1)          # (d/dtx, d/dty)
        self.gt_abs = max((self.gout * dpx).abs().sum((1, 2, 3)).max().item(), (self.gout * dpy).abs().sum((1, 2, 3)).max().item())
        self.fine = _multiple(self.out, 2) and _multiple(self.gsrc, 2) and _multiple(self.gout * dpx, 2) and _multiple(self.gout * dpy, 2)


@functools.lru_cache(maxsize=None)
def make_shift_case(geo):
    return ShiftCase(geo)


def assert_shift_exact(c, dt):
    dtype = DT[dt]
    for t in (c.src, c.gout, c.t, c.gsrc0, c.gt0):
        assert representable(t, dtype if t is not c.t and t is not c.gt0 else torch.float32)
    assert c.fine and c.gt_abs * 4 < EXACT32 and (c.gsrc.abs().max().item() + 4) * 4 < EXACT32
    assert representable(c.out, dtype)          # (multiples of 1/4 of magnitude <= 3)


def run_shift(dev, dt, c):
    """fami_shift_bilinear_fwd_* and _bwd_* (acc 0 and 1, each output alone and both) -> failures as texts"""
    from fami_pose_amd._lib import lib
    L = lib()
    assert_shift_exact(c, dt)
    B, H, W, C = c.geo
    dtype, f32 = DT[dt], torch.float32
    st = torch.cuda.current_stream(dev).cuda_stream
    A = Arena(dev)
    src, gout, t = A.operand(c.src, dtype), A.operand(c.gout, dtype), A.operand(c.t, f32)
    fails = []
    out = A.output((B, H, W, C), dtype, None, 'out')
    L.call('fami_shift_bilinear_fwd_' + dt, src.data_ptr(), t.data_ptr(), out.data_ptr(), B, H, W, C, st)
    torch.cuda.synchronize(dev)
    m = mismatch(out, c.out, '(b,h,w,c)')
    fails += ['shift fwd: ' + m] if m else []
    for acc in (0, 1):
        for do_src, do_t in ((1, 1), (1, 0), (0, 1)):
            gsrc = A.output((B, H, W, C), dtype, c.gsrc0 if acc else None, 'gsrc') if do_src else None
            gt = A.output((B, 2), f32, c.gt0 if acc else None, 'gt') if do_t else None
            ws = A.output((L.cdll.fami_shift_workspace(B) // 4,), f32, None, 'workspace')
            ptr = lambda x_: None if x_ is None else x_.data_ptr()
            L.call('fami_shift_bilinear_bwd_' + dt, gout.data_ptr(), src.data_ptr(), t.data_ptr(), ptr(gsrc), ptr(gt), B, H, W, C, acc, acc,
                   ws.data_ptr(), st)
            torch.cuda.synchronize(dev)
            tag = 'shift bwd(acc %d, gsrc %d, gt %d)' % (acc, do_src, do_t)
            if do_src:
                want = c.gsrc + (c.gsrc0 if acc else 0)
                m = mismatch(gsrc, want.to(dtype).double(), '(b,h,w,c)')
                fails += [tag + ' gsrc: ' + m] if m else []
            if do_t:
                m = mismatch(gt, c.gt + (c.gt0 if acc else 0), '(b, (tx,ty))')
                fails += [tag + ' gt: ' + m] if m else []
    return fails + A.touched()
