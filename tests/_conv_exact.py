"""Helpers of tests/test_conv_exact_gpu.py: small-integer operands, the exact fp64 reference, guarded / poisoned device
buffers and the launches of the convolution entry points through the C ABI.

Why integers: with x, dy, w in {-1, 0, 1} every partial sum of a convolution is an integer far below 2^24, so fp32
accumulation is exact in ANY order -- on the f32 MFMA, on the 16-bit MFMAs, through split-K atomics, slab reduces and the
split-product route (a small integer is its own first bf16 term; the other two terms are zero).  The result is fully
determined and the comparison is torch.equal on every element; below 256 in magnitude it is also exact in bf16 and fp16,
which removes every question of when a 16-bit kernel rounds.  No number in this file is a tolerance: 256 and 2^24 are the
exactness bounds of the 8-bit and the 24-bit significand, and they are asserted on the reference before any launch."""
import ctypes
import functools

import torch
import torch.nn.functional as F

GUARD = 1234.5          # exactly representable in fp32, bf16 and fp16 (as in tests/test_ema_gpu.py)
PAD = 4096              # guard / poison elements in front of and behind every view
DT = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
EXACT16 = 256           # integers up to 2^8 are exact in bf16 (8-bit significand) and in fp16
EXACT32 = 2 ** 24       # ... up to 2^24 in fp32, as a value and as a running sum
STATS_VARIANTS = [(0, 0), (1, 1)]      # (bias, pivot) of the fami_conv2d_fwd_stats_* launches: the ones whose bounds are asserted


def out_dim(i, k, s, p, d):
    return (i + 2 * p - d * (k - 1) - 1) // s + 1


def seed_of(geo, tier):
    s = 1000003 * tier + 17
    for v in geo:
        s = (s * 31 + int(v) + 7) % 2147483629
    return s


def _sparse(g, shape, p):
    """{-1, 0, 1}, nonzero with probability p"""
    sign = torch.randint(0, 2, shape, generator=g, dtype=torch.int64) * 2 - 1
    keep = torch.rand(shape, generator=g, dtype=torch.float64) < p
    return (sign * keep).double()


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g, dtype=torch.int64).double()


class Case:
    """Operands and exact fp64 references of one geometry (N, H, W, Ci, Co, k, stride, pad, dil), NHWC / OIHW, on the CPU.
    dense: the tier that pins the store conversion -- operands in [-2, 2], results beyond 256."""

    def __init__(self, geo, dense=False):
        self.geo, self.dense = tuple(geo), dense
        N, H, W, Ci, Co, k, s, p, d = geo
        self.Ho, self.Wo = out_dim(H, k, s, p, d), out_dim(W, k, s, p, d)
        Ho, Wo = self.Ho, self.Wo
        g = torch.Generator().manual_seed(seed_of(geo, 1 if dense else 0))
        if dense:
            self.x, self.dy, self.w = _ints(g, (N, H, W, Ci), -2, 2), _ints(g, (N, Ho, Wo, Co), -2, 2), _ints(g, (Co, Ci, k, k), -2, 2)
        else:
            self.x, self.dy, self.w = _sparse(g, (N, H, W, Ci), 0.25), _sparse(g, (N, Ho, Wo, Co), 0.25), _sparse(g, (Co, Ci, k, k), 0.5)
        self.bias, self.pivot = _ints(g, (Co,), -4, 4), _ints(g, (Co,), -4, 4)
        self.addy, self.y0 = _ints(g, (N, Ho, Wo, Co), -4, 4), _ints(g, (N, Ho, Wo, Co), -4, 4)
        self.addx, self.dx0 = _ints(g, (N, H, W, Ci), -4, 4), _ints(g, (N, H, W, Ci), -4, 4)
        self.dw0 = _ints(g, (Co, Ci, k, k), -4, 4)
        self.z, self.beta = _ints(g, (N, H, W, Ci), -2, 2), _ints(g, (Ci,), -1, 1)
        xc, dyc = self.x.permute(0, 3, 1, 2), self.dy.permute(0, 3, 1, 2)
        wr = self.w.clone().requires_grad_(True)
        yc = F.conv2d(xc, wr, None, s, p, d)
        assert tuple(yc.shape) == (N, Co, Ho, Wo)
        self.dw, = torch.autograd.grad(yc, wr, dyc)
        self.conv = yc.detach().permute(0, 2, 3, 1).contiguous()
        oph = H - ((Ho - 1) * s - 2 * p + d * (k - 1) + 1)
        opw = W - ((Wo - 1) * s - 2 * p + d * (k - 1) + 1)
        self.dgrad = F.conv_transpose2d(dyc, self.w, None, s, p, (oph, opw), 1, d).permute(0, 2, 3, 1).contiguous()
        assert tuple(self.dgrad.shape) == (N, H, W, Ci)

    # ---- expected results (fp64) of the entry points' variants
    def want_fwd(self, bias=0, addend=0, relu=0, acc=0):
        r = self.conv.clone()
        if bias:
            r += self.bias
        if addend:
            r += self.addy
        if relu:
            r.clamp_(min=0)
        return r + self.y0 if acc else r

    def want_dgrad(self, addend=0, acc=0):
        r = self.dgrad + self.addx if addend else self.dgrad.clone()
        return r + self.dx0 if acc else r

    def want_wgrad(self, acc=0):
        return self.dw + self.dw0 if acc else self.dw.clone()

    def want_stats(self, bias, pivot):
        """y and the per-channel sums of (y - pivot), (y - pivot)^2"""
        y = self.want_fwd(bias=bias)
        dlt = y.reshape(-1, y.shape[-1]) - (self.pivot if pivot else 0)
        return y, dlt.sum(0), (dlt * dlt).sum(0)

    def want_bnstats(self, relu, acc):
        """dz = mask(dx) with the mask of relu(z + beta) (mean 0, invstd 1, gamma 1: xhat = z, all exact), sum dz, sum dz z"""
        full = self.want_dgrad(acc=acc)
        dz = torch.where((self.z + self.beta) > 0, full, torch.zeros_like(full)) if relu else full
        C = dz.shape[-1]
        return dz, dz.reshape(-1, C).sum(0), (dz * self.z).reshape(-1, C).sum(0)


@functools.lru_cache(maxsize=None)
def make_case(geo, dense=False):
    return Case(geo, dense)


_BOUNDS_SEEN = set()


def assert_bounds(c, half):
    """On the reference alone, before any launch: every 16-bit activation output stays within 256 (exact in bf16 / fp16),
    every fp32 output and every fp32 partial sum of the statistics epilogues below 2^24.  A seed that breaks a bound is
    replaced; the bound stays."""
    if (c.geo, c.dense, half) in _BOUNDS_SEEN:
        return
    Ci, Co = c.geo[3], c.geo[4]
    acts = [c.want_fwd(b, a, r, ac) for b in (0, 1) for a in (0, 1) for r in (0, 1) for ac in (0, 1)]
    acts += [c.want_dgrad(a, ac) for a in (0, 1) for ac in (0, 1)]
    top = max(t.abs().max().item() for t in acts)
    if c.dense:
        assert top < EXACT32, (c.geo, top)
        _BOUNDS_SEEN.add((c.geo, c.dense, half))
        return
    assert top <= (EXACT16 if half else EXACT32 - 1), (c.geo, top)
    for ac in (0, 1):
        assert c.want_wgrad(ac).abs().max().item() < EXACT32, c.geo
    for bias, piv in STATS_VARIANTS:
        _, s1, s2 = c.want_stats(bias, piv)
        assert s2.max().item() < EXACT32 and s1.abs().max().item() < EXACT32, c.geo
    for ac in (0, 1):
        dz = c.want_dgrad(acc=ac)
        assert dz.abs().reshape(-1, Ci).sum(0).max().item() < EXACT32 and (dz * c.z).abs().reshape(-1, Ci).sum(0).max().item() < EXACT32, c.geo
    _BOUNDS_SEEN.add((c.geo, c.dense, half))


# ---------------------------------------------------------------------------------------------------------- device buffers
class Arena:
    """Every output is a view into a larger buffer of its dtype with >= PAD elements of GUARD in front and behind; every
    operand the same way inside NaN.  View starts are 256-byte aligned.  Nothing sits flush against an allocation's end."""

    def __init__(self, dev):
        self.dev = dev
        self.outs = []

    def _view(self, n, dtype, fill):
        esz = torch.empty((), dtype=dtype).element_size()
        buf = torch.full((2 * PAD + n + 256,), fill, dtype=dtype, device=self.dev)
        lo = PAD + ((-(buf.data_ptr() + PAD * esz)) % 256) // esz
        v = buf[lo:lo + n]
        assert v.data_ptr() % 256 == 0 and lo >= PAD and buf.numel() - lo - n >= PAD
        return buf, lo, v

    def operand(self, t, dtype):
        """t (CPU fp64) in dtype on the device, surrounded by NaN"""
        buf, lo, v = self._view(t.numel(), dtype, float('nan'))
        v.copy_(t.reshape(-1).to(dtype))
        return v.view(t.shape)

    def poisoned(self, n, dtype):
        """an operand another kernel writes (the packed weight image): NaN inside as well until it is written"""
        return self._view(n, dtype, float('nan'))[2]

    def output(self, shape, dtype, init=None, name='out'):
        n = 1
        for s_ in shape:
            n *= s_
        buf, lo, v = self._view(n, dtype, GUARD)
        if init is None:
            v.fill_(float('nan'))          # an element the kernel fails to write shows up as a NaN
        elif isinstance(init, (int, float)):
            v.fill_(init)
        else:
            v.copy_(init.reshape(-1).to(dtype))
        self.outs.append((name, buf, lo, n))
        return v.view(shape)

    def touched(self):
        """names of the outputs whose guard zones are not bit-for-bit intact (with the first touched offset)"""
        bad = []
        for name, buf, lo, n in self.outs:
            for side, g, base in (('front', buf[:lo], -lo), ('back', buf[lo + n:], n)):
                ne = g != GUARD
                if bool(ne.any()):
                    i = int(ne.nonzero()[0, 0])
                    bad.append('%s: %s guard touched at view offset %d (value %r)' % (name, side, base + i, g[i].item()))
        return bad


def mismatch(got, want, axes):
    """None, or the text of the first mismatching element of got (device, any dtype) against want (CPU fp64, already
    representable in got's dtype)"""
    g = got.detach().cpu()
    w = want.to(g.dtype)
    bad = (g != w) | torch.isnan(g)
    nbad = int(bad.sum())
    if nbad == 0 and torch.equal(g, w):
        return None
    idx = tuple(int(i) for i in bad.nonzero()[0])
    return '%d of %d elements differ (%d NaN); first at %s = %s: kernel %r, reference %r' % (
        nbad, g.numel(), int(torch.isnan(g).sum()), axes, idx, g[idx].item(), w[idx].item())


class Runner:
    """One geometry in one storage type on the device: operands uploaded once (inside NaN), one method per entry point.
    Every method launches into fresh guarded outputs, synchronises, and returns the list of failures as texts."""

    def __init__(self, dev, dt, c):
        from fami_pose_amd._lib import lib
        self.L, self.dev, self.dt, self.c = lib(), dev, dt, c
        self.dtype, self.half = DT[dt], dt != 'f32'
        self.sfx = '_' + dt
        self.st = torch.cuda.current_stream(dev).cuda_stream
        self.geo = c.geo
        N, H, W, Ci, Co, k, s, p, d = c.geo
        self.g10 = (N, H, W, Ci, Co, k, k, s, p, d)                    # the C ABI's (N, H, W, Ci, Co, kh, kw, stride, pad, dil)
        assert_bounds(c, self.half)                                    # ... before any launch
        A = self.A = Arena(dev)
        f32 = torch.float32
        self.x, self.dy = A.operand(c.x, self.dtype), A.operand(c.dy, self.dtype)
        self.bias, self.pivot = A.operand(c.bias, f32), A.operand(c.pivot, f32)
        self.addy, self.addx = A.operand(c.addy, self.dtype), A.operand(c.addx, self.dtype)
        self.z = A.operand(c.z, self.dtype)
        self.yrelu = A.operand((c.z + c.beta).clamp(min=0), self.dtype)
        self.mean, self.one = A.operand(torch.zeros(Ci, dtype=torch.float64), f32), A.operand(torch.ones(Ci, dtype=torch.float64), f32)
        self.beta = A.operand(c.beta, f32)
        w = A.operand(c.w, f32)
        elems = getattr(self.L.cdll, 'fami_packed_weight_elems' + (self.sfx if self.half else ''))
        self.wp = []
        for m in (0, 1):
            wp = A.poisoned(elems(Co, Ci, k, k, m), self.dtype)
            self.L.call('fami_pack_conv_weight' + self.sfx, w.data_ptr(), wp.data_ptr(), Co, Ci, k, k, m, self.st)
            self.wp.append(wp)
        self.ws_bytes = self.L.cdll.fami_conv2d_wgrad_workspace(*self.g10)
        assert self.ws_bytes >= 0
        torch.cuda.synchronize(dev)

    # ---- plumbing
    def _begin(self):
        self.A.outs = []

    def _end(self, checks):
        torch.cuda.synchronize(self.dev)
        fails = []
        for nm, got, want, axes in checks:
            m = mismatch(got, want, axes)
            if m:
                fails.append('%s: %s' % (nm, m))
        return fails + self.A.touched()

    def _act(self, shape, prior, name, dtype=None):
        return self.A.output(shape, dtype or self.dtype, prior, name)

    def _slots(self, C, name):
        nb = self.L.cdll.fami_bn_slots_bytes(C)
        assert nb % 8 == 0 and nb >= 8 * 2 * C * 8 + 4 * C
        return self.A.output((nb // 8,), torch.float64, 0.0, name)

    @staticmethod
    def _rows(slots, C):
        return slots[:8 * 2 * C].view(8, 2, C).sum(0).cpu()          # (unused slot rows stay zero)

    def _workspace(self):
        """-> (view, bytes): the kernels are told exactly the library's figure; the view is never empty (a non-null pointer)"""
        return self.A.output((max((self.ws_bytes + 3) // 4, 1),), torch.float32, None, 'workspace'), self.ws_bytes

    # ---- entry points
    def fwd(self, bias=0, addend=0, relu=0, acc=0, out_f32=0):
        c = self.c
        N, H, W, Ci, Co = c.geo[:5]
        self._begin()
        y = self._act((N, c.Ho, c.Wo, Co), c.y0 if acc else None, 'y', torch.float32 if out_f32 else None)
        p = lambda t, on=1: t.data_ptr() if on else None
        if self.half:
            assert not addend
            self.L.call('fami_conv2d_fwd' + self.sfx, p(self.x), p(self.wp[0]), p(self.bias, bias), p(y), *self.g10, relu, acc, out_f32, self.st)
        else:
            self.L.call('fami_conv2d_fwd_f32', p(self.x), p(self.wp[0]), p(self.bias, bias), p(self.addy, addend), p(y), *self.g10, relu, acc, self.st)
        tag = 'fwd(bias=%d addend=%d relu=%d acc=%d out_f32=%d)' % (bias, addend, relu, acc, out_f32)
        return self._end([(tag, y, c.want_fwd(bias, addend, relu, acc), '(n,h,w,c)')])

    def dgrad(self, addend=0, acc=0):
        c = self.c
        N, H, W, Ci, Co = c.geo[:5]
        self._begin()
        dx = self._act((N, H, W, Ci), c.dx0 if acc else None, 'dx')
        if self.half:
            assert not addend
            self.L.call('fami_conv2d_dgrad' + self.sfx, self.dy.data_ptr(), self.wp[1].data_ptr(), dx.data_ptr(), *self.g10, acc, self.st)
        else:
            self.L.call('fami_conv2d_dgrad_f32', self.dy.data_ptr(), self.wp[1].data_ptr(), self.addx.data_ptr() if addend else None,
                        dx.data_ptr(), *self.g10, acc, self.st)
        return self._end([('dgrad(addend=%d acc=%d)' % (addend, acc), dx, c.want_dgrad(addend, acc), '(n,h,w,c)')])

    def wgrad(self, acc=0):
        c = self.c
        Ci, Co, k = c.geo[3], c.geo[4], c.geo[5]
        self._begin()
        dw = self.A.output((Co, Ci, k, k), torch.float32, c.dw0 if acc else None, 'dw')
        ws, wsb = self._workspace()
        self.L.call('fami_conv2d_wgrad' + self.sfx, self.x.data_ptr(), self.dy.data_ptr(), dw.data_ptr(), ws.data_ptr(), wsb,
                    *self.g10, acc, self.st)
        return self._end([('wgrad(acc=%d)' % acc, dw, c.want_wgrad(acc), '(o,i,kh,kw)')])

    def wgrad_deferred(self, reps=3):
        """`reps` deferred weight gradients (fresh, accumulating, fresh, ...) whose reduces ONE fami_wgrad_reduce_batch call
        launches: each must equal the reference (and so the immediate form, which wgrad() holds to the same reference)"""
        c = self.c
        Ci, Co, k = c.geo[3], c.geo[4], c.geo[5]
        self._begin()
        n = self.L.cdll.fami_wgrad_reduce_desc_longs()
        descs = (ctypes.c_long * (n * reps))()
        outs = []
        for r in range(reps):
            acc = r % 2
            dw = self.A.output((Co, Ci, k, k), torch.float32, c.dw0 if acc else None, 'dw[%d]' % r)
            ws, wsb = self._workspace()
            one = (ctypes.c_long * n)()
            self.L.call('fami_conv2d_wgrad_defer' + self.sfx, self.x.data_ptr(), self.dy.data_ptr(), dw.data_ptr(), ws.data_ptr(), wsb,
                        *self.g10, acc, one, self.st)
            descs[r * n:(r + 1) * n] = one[:]
            outs.append(('wgrad_defer[%d](acc=%d)' % (r, acc), dw, c.want_wgrad(acc), '(o,i,kh,kw)'))
        self.L.call('fami_wgrad_reduce_batch', descs, reps, self.st)
        return self._end(outs)

    def fwd_stats(self, bias=0, pivot=0):
        c = self.c
        N, H, W, Ci, Co = c.geo[:5]
        self._begin()
        y = self._act((N, c.Ho, c.Wo, Co), None, 'y')
        slots = self._slots(Co, 'slots')
        self.L.call('fami_conv2d_fwd_stats' + self.sfx, self.x.data_ptr(), self.wp[0].data_ptr(), self.bias.data_ptr() if bias else None,
                    y.data_ptr(), *self.g10, slots.data_ptr(), self.pivot.data_ptr() if pivot else None, self.st)
        torch.cuda.synchronize(self.dev)
        wy, s1, s2 = c.want_stats(bias, pivot)
        rows = self._rows(slots, Co)
        piv = slots[8 * 2 * Co:].view(torch.float32)[:Co]
        tag = 'fwd_stats(bias=%d pivot=%d)' % (bias, pivot)
        return self._end([(tag + ' y', y, wy, '(n,h,w,c)'), (tag + ' sum(y - pivot)', rows[0], s1, '(c,)'),
                          (tag + ' sum((y - pivot)^2)', rows[1], s2, '(c,)'),
                          (tag + ' stored pivot', piv, c.pivot if pivot else torch.zeros(Co, dtype=torch.float64), '(c,)')])

    def _bn_args(self, relu, slots):
        return (self.z.data_ptr(), self.yrelu.data_ptr() if relu == 1 else None, self.mean.data_ptr(), self.one.data_ptr(),
                self.one.data_ptr(), self.beta.data_ptr(), relu, slots.data_ptr())

    def dgrad_bnstats(self, relu, acc):
        c = self.c
        N, H, W, Ci, Co = c.geo[:5]
        self._begin()
        dx = self._act((N, H, W, Ci), c.dx0 if acc else None, 'dz')
        slots = self._slots(Ci, 'slots')
        self.L.call('fami_conv2d_dgrad_bnstats' + self.sfx, self.dy.data_ptr(), self.wp[1].data_ptr(), dx.data_ptr(), *self.g10, acc,
                    *self._bn_args(relu, slots), self.st)
        torch.cuda.synchronize(self.dev)
        dz, s1, s2 = c.want_bnstats(relu, acc)
        rows = self._rows(slots, Ci)
        tag = 'dgrad_bnstats(relu=%d acc=%d)' % (relu, acc)
        return self._end([(tag + ' dz', dx, dz, '(n,h,w,c)'), (tag + ' sum(dz)', rows[0], s1, '(c,)'), (tag + ' sum(dz xhat)', rows[1], s2, '(c,)')])

    def bwd_pair(self, acc_dx=0, acc_dw=0, relu=None):
        """fami_conv2d_bwd_pair_* + the deferred reduce; relu None: no statistics epilogue (the only form of f32 storage)"""
        c = self.c
        N, H, W, Ci, Co, k = c.geo[:6]
        self._begin()
        dx = self._act((N, H, W, Ci), c.dx0 if acc_dx else None, 'dx')
        dw = self.A.output((Co, Ci, k, k), torch.float32, c.dw0 if acc_dw else None, 'dw')
        ws, wsb = self._workspace()
        desc = (ctypes.c_long * self.L.cdll.fami_wgrad_reduce_desc_longs())()
        head = (self.x.data_ptr(), self.dy.data_ptr(), self.wp[1].data_ptr(), dx.data_ptr(), dw.data_ptr(), ws.data_ptr(), wsb)
        checks = []
        if self.half:
            slots = self._slots(Ci, 'slots') if relu is not None else None
            bn = self._bn_args(relu, slots) if relu is not None else (None, None, None, None, None, None, 0, None)
            self.L.call('fami_conv2d_bwd_pair' + self.sfx, *head, *self.g10, acc_dx, acc_dw, desc, *bn, self.st)
        else:
            assert relu is None
            self.L.call('fami_conv2d_bwd_pair_f32', *head, *self.g10, acc_dx, acc_dw, desc, None, None, None, None, self.st)
        self.L.call('fami_wgrad_reduce_batch', desc, 1, self.st)
        torch.cuda.synchronize(self.dev)
        tag = 'bwd_pair(acc_dx=%d acc_dw=%d relu=%s)' % (acc_dx, acc_dw, relu)
        if relu is None:
            checks.append((tag + ' dx', dx, c.want_dgrad(acc=acc_dx), '(n,h,w,c)'))
        else:
            dz, s1, s2 = c.want_bnstats(relu, acc_dx)
            rows = self._rows(slots, Ci)
            checks += [(tag + ' dz', dx, dz, '(n,h,w,c)'), (tag + ' sum(dz)', rows[0], s1, '(c,)'), (tag + ' sum(dz xhat)', rows[1], s2, '(c,)')]
        checks.append((tag + ' dw', dw, c.want_wgrad(acc_dw), '(o,i,kh,kw)'))
        return self._end(checks)
