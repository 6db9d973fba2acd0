"""Helpers of tests/test_stream_exact_gpu.py, tests/test_loss_exact_gpu.py and tests/test_stream_exact_host.py: operands, fp64
references and launches (through the C ABI, into the guarded buffers of tests/_conv_exact.Arena) of the kernels that run between
the convolutions, the BatchNorms and the DCNs: csrc/elementwise.hip, the linear kernels of csrc/core.hip and csrc/loss.hip.

Every family below is ONE function f(case, dt, R=None).  It builds the operands and the fp64 reference of the case on the CPU and
asserts, on the reference alone, the conditions under which the result is fully determined whatever the order of operations and
whether or not a multiply-add is contracted:
  values               small integers (and halves where a factor is a power of two)
  factors              powers of two
  fp32 sums            below 2^24 units of their last place (the sum of magnitudes bounds every partial sum)
  16-bit outputs       within 256, and the fp64 reference rounded once
With R None it stops there (tests/test_stream_exact_host.py: a bad seed or bound shows without a GPU).  With a Run it uploads the
operands inside NaN, launches into outputs that lie between 4096-element guard zones and start as NaN (or as the stated prior
where the call accumulates) and returns the failures as texts.  No number here is a tolerance; the one exception is softmax_kl
(expf and logf are not determined), whose bound is measured in the test: see softmax_kl()."""
import ctypes
import types
import zlib

import numpy as np
import torch

from _conv_exact import Arena, DT, GUARD, PAD, mismatch          # noqa: F401  (re-exported for the test files)

TYPES = ['f32', 'bf16', 'f16']
CAP = 2048 * 256          # fami_ew_grid: at most 2048 workgroups of 256 threads; one work item more and the loop takes a second trip
EXACT16 = 256
EXACT32 = 2 ** 24
IGUARD = 1234             # guard value of the integer buffers
F32, F64 = torch.float32, torch.float64
TINY = {'f32': 2.0 ** -126, 'bf16': 2.0 ** -126, 'f16': 2.0 ** -14}          # smallest positive normal of the storage type


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g, dtype=torch.int64).double()


def pick(g, shape, values):
    v = torch.tensor(values, dtype=F64)
    return v[torch.randint(0, len(values), tuple(shape), generator=g)]


def representable(t, dtype):
    return bool((t.to(dtype).double() == t).all())


def multiple(t, bits):
    s = t * 2.0 ** bits
    return bool((s == s.round()).all())


def exact_out(t, dt, what):
    """a result the kernel forms in fp32: exact there, and within 256 where it is stored in 16 bits (then rounded once)"""
    assert representable(t, F32), what
    assert dt == 'f32' or t.abs().max().item() <= EXACT16, what


def ptr(t):
    return None if t is None else t.data_ptr()


class StreamArena(Arena):
    """The Arena of the other exact suites, plus: a view that starts `shift` elements behind the 256-byte boundary (the scalar
    paths that an unaligned pointer selects), and guarded integer buffers."""

    def __init__(self, dev):
        super().__init__(dev)
        self.shift = 0
        self.iouts = []

    def at(self, shift):
        self.shift = shift
        return self

    def _view(self, n, dtype, fill):
        k, self.shift = self.shift, 0
        buf, lo, _ = super()._view(n + k, dtype, fill)
        return buf, lo + k, buf[lo + k:lo + k + n]

    def int_output(self, init, name):
        """init (CPU integer tensor) between guard zones of IGUARD"""
        n, esz = init.numel(), init.element_size()
        buf = torch.full((2 * PAD + n + 256,), IGUARD, dtype=init.dtype, device=self.dev)
        lo = PAD + ((-(buf.data_ptr() + PAD * esz)) % 256) // esz
        v = buf[lo:lo + n]
        v.copy_(init.reshape(-1))
        self.iouts.append((name, buf, lo, n))
        return v.view(init.shape)

    def touched(self):
        bad = super().touched()
        for name, buf, lo, n in self.iouts:
            for side, g, base in (('front', buf[:lo], -lo), ('back', buf[lo + n:], n)):
                ne = g != IGUARD
                if bool(ne.any()):
                    i = int(ne.nonzero()[0, 0])
                    bad.append('%s: %s guard touched at view offset %d (value %r)' % (name, side, base + i, g[i].item()))
        return bad


class Run:
    """One case on the device: operands inside NaN, outputs between guards, the comparisons collected and made after one
    synchronise.  end() -> the failures as texts."""

    def __init__(self, dev):
        from fami_pose_amd._lib import lib
        self.L, self.dev = lib(), dev
        self.st = torch.cuda.current_stream(dev).cuda_stream
        self.A = StreamArena(dev)
        self.checks, self.fails, self.keep = [], [], []          # (keep: an operand lives until the case ends, not until its pointer is taken)

    def op(self, t, dtype, shift=0):
        v = self.A.at(shift).operand(t, dtype)
        self.keep.append(v)
        return v

    def out(self, shape, dtype, init=None, name='out', shift=0):
        return self.A.at(shift).output(tuple(shape), dtype, init, name)

    def ints(self, init, name):
        v = self.A.int_output(init, name)
        self.keep.append(v)
        return v

    def call(self, name, *args):
        self.L.call(name, *args)

    def refused(self, name, *args):
        """the return code of a call that must be refused (no exception), and that the library names the entry point"""
        self.L.bind(None)
        rc = getattr(self.L.cdll, name)(*args)
        if rc != -1:
            self.fails.append('%s returned %d, not -1' % (name, rc))
        elif name.encode() not in self.L.cdll.fami_last_error():
            self.fails.append('%s: fami_last_error() does not name it: %r' % (name, self.L.cdll.fami_last_error()))

    def want(self, tag, got, want, axes='(i,)'):
        self.checks.append((tag, got, want, axes))

    def want_untouched(self, tag, got):
        """an output of a refused call: still the NaN it started as, everywhere"""
        self.checks.append((tag, got, None, 'untouched'))

    def want_bits(self, tag, got, want):
        """bit for bit, through an integer view of the same width (signed zeros, NaN payloads)"""
        self.checks.append((tag, got, want, None))

    def end(self):
        torch.cuda.synchronize(self.dev)
        fails = list(self.fails)
        for tag, got, want, axes in self.checks:
            if axes == 'untouched':
                if not bool(torch.isnan(got).all()):
                    fails.append('%s: %d elements were written' % (tag, int((~torch.isnan(got)).sum())))
            elif axes is None:
                it = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[got.element_size()]
                g = got.detach().cpu().contiguous().view(it)
                w = want.to(got.dtype).contiguous().view(it)
                if not torch.equal(g, w):
                    i = int((g != w).reshape(-1).nonzero()[0, 0])
                    fails.append('%s: bits differ, first at %d: kernel %#x, reference %#x' % (tag, i, g.reshape(-1)[i].item(), w.reshape(-1)[i].item()))
            elif got.dtype in (torch.int64, torch.int32):
                g = got.detach().cpu()
                if not torch.equal(g, want):
                    i = int((g != want).reshape(-1).nonzero()[0, 0])
                    fails.append('%s: first difference at %d: kernel %d, reference %d' % (tag, i, g.reshape(-1)[i].item(), want.reshape(-1)[i].item()))
            else:
                m = mismatch(got, want, axes)
                if m:
                    fails.append('%s: %s' % (tag, m))
        return fails + self.A.touched()


# ============================================================================================== csrc/elementwise.hip
# ---- layout converts (work item: one element)
LAYOUT_CASES = [(1, 1, 5, 3), (1, 3, 5, 7), (1, 17, 3, 5), (2, 48, 7, 5), (1, 3, 19, 9), (116, 3, 37, 41)]          # (N, C, H, W)
assert 3 * 19 * 9 == 2 * 256 + 1 and 116 * 3 * 37 * 41 > CAP


def layout(p, dt, R=None):
    """fami_nchw_to_nhwc_* and fami_nhwc_to_nchw_* (accumulate 0 and 1): a pure permutation of integers within 256"""
    N, C, H, W = p
    g = gen('layout', p)
    x, prior = ints(g, (N, C, H, W), -256, 256), ints(g, (N, C, H, W), -4, 4)
    nhwc = x.permute(0, 2, 3, 1).contiguous()
    assert representable(x, DT[dt]) and representable(x + prior, F32)
    if R is None:
        return []
    src = R.op(x, F32)
    dst = R.out((N, H, W, C), DT[dt], None, 'nhwc')
    R.call('fami_nchw_to_nhwc_' + dt, ptr(src), ptr(dst), N, C, H, W, R.st)
    R.want('nchw_to_nhwc%s' % (p,), dst, nhwc, '(n,h,w,c)')
    s2 = R.op(nhwc, DT[dt])
    for acc in (0, 1):
        d2 = R.out((N, C, H, W), F32, prior if acc else None, 'nchw(acc %d)' % acc)
        R.call('fami_nhwc_to_nchw_' + dt, ptr(s2), ptr(d2), N, C, H, W, acc, R.st)
        R.want('nhwc_to_nchw%s acc %d' % (p, acc), d2, x + prior if acc else x, '(n,c,h,w)')
    return R.end()


PACK_CASES = [(1, 0, 5, 3), (1, 0, 19, 9), (3, 0, 4, 7), (1, 1, 5, 3), (3, 1, 3, 5), (1, 3, 7, 5), (3, 3, 5, 9), (3, 3, 123, 119)]          # (B, S, H, W)
assert 4 * 3 * 123 * 119 * 3 > CAP


def pack_frames(p, dt, R=None):
    """fami_pack_frames_*: key frame and S supporting frames, NCHW fp32 -> frame-major NHWC"""
    B, S, H, W = p
    g = gen('pack', p)
    kf = ints(g, (B, 3, H, W), -256, 256)
    sup = ints(g, (B, 3 * S, H, W), -256, 256) if S else None
    frames = torch.cat([kf] + [sup[:, 3 * f:3 * f + 3] for f in range(S)], 0).permute(0, 2, 3, 1).contiguous()
    assert representable(frames, DT[dt]) and tuple(frames.shape) == ((1 + S) * B, H, W, 3)
    if R is None:
        return []
    out = R.out(frames.shape, DT[dt], None, 'frames')
    R.call('fami_pack_frames_' + dt, ptr(R.op(kf, F32)), ptr(R.op(sup, F32)) if S else None, ptr(out), B, S, H, W, R.st)
    R.want('pack_frames%s' % (p,), out, frames, '(f*B+b,y,x,c)')
    return R.end()


# ---- copy_channels: (P, Cs, src_off, Cd, dst_off, Cc, src_shift, dst_shift)
COPY_CASES = [
    (5, 12, 4, 16, 8, 8, 0, 0),                # four-wide; src_off + Cc == Cs and dst_off + Cc == Cd: the last row ends flush against the guard
    (65, 8, 0, 8, 4, 4, 0, 0),                 # four-wide, 65 items
    (257, 8, 4, 12, 0, 4, 0, 0),               # four-wide, 256 + 1 items
    (CAP + 1, 4, 0, 8, 4, 4, 0, 0),            # four-wide, one item past the cap
    (5, 20, 0, 24, 4, 17, 0, 0),               # scalar by Cc = 17 alone
    (5, 12, 3, 16, 8, 8, 0, 0),                # scalar by an odd src_off alone
    (5, 12, 4, 16, 8, 8, 1, 0),                # scalar by the source view's start alone
    (5, 12, 4, 16, 8, 8, 0, 1),                # ... by the destination view's start
    (3, 20, 3, 24, 7, 17, 0, 0),               # scalar, both rows flush
    (257, 1, 0, 3, 2, 1, 0, 0),                # scalar, 256 + 1 items
    ((CAP + 1) // 3, 3, 0, 4, 1, 3, 0, 0),     # scalar, one item past the cap
]
assert (CAP + 1) % 3 == 0


def copy_is_vector(p):
    P, Cs, so, Cd, do, Cc, ss, ds = p
    return ((Cs | so | Cd | do | Cc) & 3) == 0 and ss % 4 == 0 and ds % 4 == 0


def copy_channels(p, dt, R=None):
    """fami_copy_channels_* with accumulate 0 and 1; the untouched channels of dst keep their prior integers"""
    P, Cs, so, Cd, do, Cc, ss, ds = p
    g = gen('copy', p)
    src, prior = ints(g, (P, Cs), -100, 100), ints(g, (P, Cd), -100, 100)
    wants = []
    for acc in (0, 1):
        w = prior.clone()
        w[:, do:do + Cc] = src[:, so:so + Cc] + (prior[:, do:do + Cc] if acc else 0)
        exact_out(w, dt, p)
        wants.append(w)
    if R is None:
        return []
    s = R.op(src, DT[dt], ss)
    for acc in (0, 1):
        d = R.out((P, Cd), DT[dt], prior, 'dst(acc %d)' % acc, ds)
        R.call('fami_copy_channels_' + dt, ptr(s), ptr(d), P, Cs, so, Cd, do, Cc, acc, R.st)
        R.want('copy_channels%s acc %d' % (p, acc), d, wants[acc], '(p,c)')
    return R.end()


# ---- concat / split: (widths, P)
CAT_CASES = [((48, 48), 105), ((48, 96, 16), 105), ((48, 48, 48, 48), 105), ((4, 8), 105), ((8,), 105), ((4, 4, 4, 4), 105), ((4, 4, 4, 4), 1),
             ((4, 8), (CAP + 1) // 3)]


def cat_split(p, dt, R=None):
    """fami_concat_channels_* and fami_split_channels_* (a skipped slice, accumulate per slice)"""
    cs, P = p
    n = len(cs)
    g = gen('cat', p)
    xs = [ints(g, (P, c), -100, 100) for c in cs]
    whole = ints(g, (P, sum(cs)), -100, 100)
    old = [ints(g, (P, c), -100, 100) for c in cs]
    accs = [k % 2 for k in range(n)]
    skip = n - 1 if n > 2 else -1
    want = []
    for k, piece in enumerate(torch.split(whole, list(cs), 1)):
        want.append(old[k] if k == skip else (old[k] + piece if accs[k] else piece.clone()))
        exact_out(want[k], dt, p)
    assert representable(torch.cat(xs, 1), DT[dt])
    if R is None:
        return []
    carr = (ctypes.c_int * 4)(*cs)
    y = R.out((P, sum(cs)), DT[dt], None, 'cat')
    srcs = [R.op(x, DT[dt]) for x in xs]
    R.call('fami_concat_channels_' + dt, (ctypes.c_void_p * 4)(*[ptr(s) for s in srcs]), carr, n, ptr(y), P, R.st)
    R.want('concat%s' % (p,), y, torch.cat(xs, 1), '(p,c)')
    dst = [R.out((P, c), DT[dt], old[k], 'slice %d' % k) for k, c in enumerate(cs)]
    ptrs = (ctypes.c_void_p * 4)(*[None if k == skip else ptr(d) for k, d in enumerate(dst)])
    R.call('fami_split_channels_' + dt, ptr(R.op(whole, DT[dt])), ptrs, carr, (ctypes.c_int * 4)(*accs), n, P, R.st)
    for k in range(n):
        R.want('split%s slice %d (acc %d, skipped %d)' % (p, k, accs[k], k == skip), dst[k], want[k], '(p,c)')
    return R.end()


# ---- axpby: (n, alpha, beta, b given, alias in (None, 'a', 'b'), moved view in (None, 'a', 'b', 'out'))
AXPBY_VEC_CAP, AXPBY_SCALAR_CAP = 4 * (CAP + 1) + 1, CAP + 1          # n4 = CAP + 1 with a one-element tail; CAP + 1 scalar items
AXPBY_CASES = (
    [(n, 0.5, 2.0, 1, None, None) for n in (1, 3, 4, 5, 1027, AXPBY_VEC_CAP)] +
    [(n, -1.0, 1.0, 0, None, None) for n in (3, 5, 1027)] +
    [(n, 1.0, -1.0, 1, 'a', None) for n in (5, 1027)] + [(n, 2.0, 1.0, 1, 'b', None) for n in (5, 1027)] +          # the Trainer's accumulation: out is an operand
    [(1, 2.0, 0.5, 1, None, 'a'), (5, 2.0, 0.5, 1, None, 'a'), (1027, -1.0, 0.5, 1, None, 'a'), (1027, 1.0, 2.0, 1, None, 'b'),
     (1027, 0.5, 0.5, 1, None, 'out'), (1027, 2.0, 1.0, 0, None, 'out'), (1027, 1.0, 1.0, 1, 'a', 'a'), (AXPBY_SCALAR_CAP, 0.5, -1.0, 1, None, 'b')])


def axpby(p, dt, R=None):
    """fami_axpby_*: out = alpha a + beta b, b may be null, out may be a or b; the vector path needs all three views 16-byte
    (8-byte for 16-bit types) aligned"""
    n, alpha, beta, has_b, alias, moved = p
    g = gen('axpby', p)
    a, b = ints(g, (n,), -60, 60), ints(g, (n,), -60, 60)
    want = alpha * a + (beta * b if has_b else 0)
    assert alpha in (1, -1, 0.5, 2) and beta in (1, -1, 0.5, 2)
    exact_out(want, dt, p)
    if R is None:
        return []
    sh = lambda who: int(moved == who)
    if alias == 'a':
        o = av = R.out((n,), DT[dt], a, 'out (= a)', 1 if moved in ('a', 'out') else 0)
        bv = R.op(b, DT[dt], sh('b')) if has_b else None
    elif alias == 'b':
        o = bv = R.out((n,), DT[dt], b, 'out (= b)', 1 if moved in ('b', 'out') else 0)
        av = R.op(a, DT[dt], sh('a'))
    else:
        av = R.op(a, DT[dt], sh('a'))
        bv = R.op(b, DT[dt], sh('b')) if has_b else None
        o = R.out((n,), DT[dt], None, 'out', sh('out'))
    R.call('fami_axpby_' + dt, ptr(av), ptr(bv), ptr(o), n, alpha, beta, R.st)
    R.want('axpby%s' % (p,), o, want)
    return R.end()


# ---- cast_add, widen, fill: (n, moved by one element)
FLAT_CASES = [(1, 0), (3, 0), (4, 0), (5, 0), (257, 0), (1027, 0), (1027, 1), (CAP + 1, 0)]
FILL_VALUES = [0.0, -0.0, 1234.5, float('nan')]
NAN_BITS = {'f32': (torch.int32, 0x7FC00000), 'bf16': (torch.int16, 0x7FC0), 'f16': (torch.int16, 0x7E00)}


def cast_widen_fill(p, dt, R=None):
    """fami_cast_add_* (accumulate 0 and 1), fami_widen_*, fami_fill_* (bitwise)"""
    n, moved = p
    g = gen('flat', p)
    src, prior = ints(g, (n,), -100, 100), ints(g, (n,), -100, 100)
    half = pick(g, (n,), [-3.5, -0.5, 0.0, 0.5, 1.5, 96.0, -256.0, 255.0])
    exact_out(src + prior, dt, p)
    assert representable(src, DT[dt]) and representable(half, DT[dt])
    if R is None:
        return []
    s = R.op(src, F32)
    for acc in (0, 1):
        d = R.out((n,), DT[dt], prior if acc else None, 'cast_add dst(acc %d)' % acc, moved)
        R.call('fami_cast_add_' + dt, ptr(s), ptr(d), n, acc, R.st)
        R.want('cast_add%s acc %d' % (p, acc), d, src + prior if acc else src)
    wide = R.out((n,), F32, None, 'widen dst', moved)
    R.call('fami_widen_' + dt, ptr(R.op(half, DT[dt], moved)), ptr(wide), n, R.st)
    R.want('widen%s' % (p,), wide, half)
    for v in FILL_VALUES:
        o = R.out((n,), DT[dt], None, 'fill %r' % v, moved)
        R.call('fami_fill_' + dt, ptr(o), n, v, R.st)
        want = torch.full((n,), v, dtype=F32)
        if v != v:          # the quiet NaN a float argument arrives as, converted as IEEE 754 converts it: sign, quiet bit, payload truncated
            want = torch.full((n,), NAN_BITS[dt][1], dtype=NAN_BITS[dt][0]).view(DT[dt])
        R.want_bits('fill%s %r' % (p, v), o, want)
    return R.end()


# ---- fuse_sum: (N, H, W, C, ((shift, batchnorm), ...), relu, all-null mean array)
FUSE_CASES = [
    (1, 3, 5, 4, ((0, 0),), 0, 1),                                    # 15 items, one identity term, the all-null mean array
    (1, 5, 41, 20, ((0, 1), (0, 0)), 1, 0),                           # 4 * 256 + 1 items; two terms with the SAME shift
    (2, 6, 10, 20, ((0, 1), (1, 0)), 1, 0),
    (2, 6, 10, 20, ((1, 0), (0, 0)), 0, 1),
    (2, 4, 12, 48, ((0, 1), (1, 1), (2, 0)), 1, 0),
    (1, 8, 24, 4, ((0, 0), (1, 1), (2, 0), (3, 1)), 0, 0),
    (2, 8, 24, 48, ((3, 1), (0, 1), (2, 1), (1, 1)), 1, 0),
    (1, 8, 8, 20, ((3, 0),), 1, 0),
    (1, 724, 732, 4, ((0, 0), (2, 1)), 1, 0),                         # 529968 items: past the cap
]
assert 5 * 41 * 5 == 4 * 256 + 1 and 724 * 732 > CAP


def fuse_sum(p, dt, R=None):
    """fami_fuse_sum_*: the fp64 restatement of the fuse loop of hrnet.py (y = relu(sum_k upsample_nearest(bn_k(x_k))))"""
    N, H, W, C, terms, relu, null_mean = p
    assert C % 4 == 0 and not (null_mean and any(bn for _, bn in terms))
    g = gen('fuse', p)
    xs, bns, total = [], [], torch.zeros(N, H, W, C, dtype=F64)
    for s, bn in terms:
        assert H % (1 << s) == 0 and W % (1 << s) == 0
        x = ints(g, (N, H >> s, W >> s, C), -4, 4) * (2 if bn else 1)
        if bn:
            mean, beta = 2 * ints(g, (C,), -2, 2), ints(g, (C,), -4, 4)
            invstd, gamma = pick(g, (C,), [-2, -1, -0.5, 0.5, 1, 2]), pick(g, (C,), [-2, -1, -0.5, 0.5, 1, 2])
            sc = invstd * gamma
            sf = beta - mean * sc
            assert representable(sc, F32) and representable(sf, F32)
            t = x * sc + sf
            bns.append((mean, invstd, gamma, beta))
        else:
            t = x
            bns.append(None)
        assert multiple(t, 1), 'a term is neither an integer nor a half'
        xs.append(x)
        total += t.repeat_interleave(1 << s, 1).repeat_interleave(1 << s, 2)          # nearest upsampling by 2^s
    want = total.clamp(min=0) if relu else total
    exact_out(total, dt, p)
    if R is None:
        return []
    n = len(terms)
    xd = [R.op(x, DT[dt]) for x in xs]
    arr = lambda vals: (ctypes.c_void_p * 4)(*vals)
    cols = [[None] * n for _ in range(4)]
    for k, b in enumerate(bns):
        if b is not None:
            for j in range(4):
                cols[j][k] = ptr(R.op(b[j], F32))
    y = R.out((N, H, W, C), DT[dt], None, 'y')
    bn_args = [None] * 4 if null_mean else [arr(c) for c in cols]
    R.call('fami_fuse_sum_' + dt, n, arr([ptr(x) for x in xd]), *bn_args, (ctypes.c_int * 4)(*[s for s, _ in terms]), ptr(y), N, H, W, C, relu, R.st)
    R.want('fuse_sum%s' % (p,), y, want, '(n,h,w,c)')
    return R.end()


def fuse_pool_refusals(dt, R):
    """non-positive N / H / W: -1 and nothing written"""
    x = R.op(torch.ones(64, dtype=F64), DT[dt])
    for N, H, W in ((0, 2, 2), (1, 0, 2), (1, 2, 0), (-1, 2, 2)):
        y = R.out((64,), DT[dt], None, 'y of a refused fuse_sum')
        R.refused('fami_fuse_sum_' + dt, 1, (ctypes.c_void_p * 4)(ptr(x)), None, None, None, None, (ctypes.c_int * 4)(0), ptr(y), N, H, W, 4, 0, R.st)
        R.want_untouched('refused fuse_sum(%d, %d, %d)' % (N, H, W), y)
        o = R.out((64,), DT[dt], None, 'out of a refused pool_relu_bwd')
        R.refused('fami_pool_relu_bwd_' + dt, ptr(x), None, ptr(o), N, H, W, 4, 0, 0, R.st)
        R.want_untouched('refused pool_relu_bwd(%d, %d, %d)' % (N, H, W), o)
    return R.end()


# ---- the ReLU-masked gradient passes
def relu_outputs(g, shape, dt):
    """y of a ReLU layer: both zeros, the smallest positive normal of the storage type, negative and positive values"""
    return pick(g, shape, [0.0, -0.0, TINY[dt], -TINY[dt], -1.0, -3.0, 2.0, 5.0])


RELU_CASES = [4, 1028, 4 * (CAP + 1)]          # n: 1, 256 + 1 and CAP + 1 four-wide items


def relu_bwd(n, dt, R=None):
    """fami_relu_bwd_* with accumulate 0 and 1: dx (=|+=) dy (y > 0); both zeros block the gradient"""
    g = gen('relu', n)
    dy, prior, y = ints(g, (n,), -100, 100), ints(g, (n,), -100, 100), relu_outputs(g, (n,), dt)
    masked = torch.where(y > 0, dy, torch.zeros_like(dy))
    exact_out(masked + prior, dt, n)
    assert representable(y, DT[dt]) and (y == 0).any() and (y == TINY[dt]).any()
    if R is None:
        return []
    dyd, yd = R.op(dy, DT[dt]), R.op(y, DT[dt])
    for acc in (0, 1):
        dx = R.out((n,), DT[dt], prior if acc else None, 'dx(acc %d)' % acc)
        R.call('fami_relu_bwd_' + dt, ptr(dyd), ptr(yd), ptr(dx), n, acc, R.st)
        R.want('relu_bwd(n %d, acc %d)' % (n, acc), dx, masked + prior if acc else masked)
    return R.end()


# (N, Hl, Wl, C, shift, relu)
POOL_CASES = ([(2, 3, 5, 4, s, 1) for s in range(5)] + [(1, 1, 1, 48, s, 0) for s in range(5)] + [(1, 1, 1, 4, 4, 1), (2, 3, 5, 48, 2, 0), (1, 257, 1, 4, 1, 1)] +
              [(1, 3, (CAP + 1) // 3, 4, 0, 1), (1, 3, (CAP + 1) // 3, 4, 0, 0)])


def pool_relu_bwd(p, dt, R=None):
    """fami_pool_relu_bwd_*: out[n,hl,wl,c] = sum over the 2^s x 2^s window of dy (y > 0); relu 0 passes a null y"""
    N, Hl, Wl, C, s, relu = p
    f = 1 << s
    g = gen('pool', p)
    dy, y = ints(g, (N, Hl * f, Wl * f, C), -1, 1), relu_outputs(g, (N, Hl * f, Wl * f, C), dt)
    m = torch.where(y > 0, dy, torch.zeros_like(dy)) if relu else dy
    want = m.view(N, Hl, f, Wl, f, C).sum((2, 4))
    assert m.abs().view(N, Hl, f, Wl, f, C).sum((2, 4)).max().item() <= EXACT16          # every partial sum of a window, in any order
    if R is None:
        return []
    out = R.out((N, Hl, Wl, C), DT[dt], None, 'out')
    R.call('fami_pool_relu_bwd_' + dt, ptr(R.op(dy, DT[dt])), ptr(R.op(y, DT[dt])) if relu else None, ptr(out), N, Hl, Wl, C, s, relu, R.st)
    R.want('pool_relu_bwd%s' % (p,), out, want, '(n,hl,wl,c)')
    return R.end()


# ---- f32 / i64 helpers
SCALE_PAIRS_CASES = [(n, acc) for n in (1, 128, 129) for acc in (0, 1)]


def scale_pairs(p, dt=None, R=None):
    """fami_scale_pairs_f32: out[i] (=|+=) in[i] (sx, sy) over n (x, y) pairs"""
    n, acc = p
    sx, sy = 0.5, -4.0
    g = gen('pairs', p)
    x, prior = ints(g, (n, 2), -100, 100), ints(g, (n, 2), -100, 100)
    want = x * torch.tensor([sx, sy], dtype=F64) + (prior if acc else 0)
    assert representable(want, F32)
    if R is None:
        return []
    out = R.out((n, 2), F32, prior if acc else None, 'out')
    R.call('fami_scale_pairs_f32', ptr(R.op(x, F32)), ptr(out), n, sx, sy, acc, R.st)
    R.want('scale_pairs%s' % (p,), out, want, '(pair,xy)')
    return R.end()


I64_CASES = [1, 257, CAP + 1]


def i64_ops(n, dt=None, R=None):
    """fami_incr_i64 and fami_add_i64 on values beyond 2^53: a round trip through a double would show"""
    g = gen('i64', n)
    v = torch.randint(2 ** 53 + 1, 2 ** 62, (n,), generator=g, dtype=torch.int64) | 1          # odd and > 2^53: no double holds it
    inc = torch.randint(-2 ** 40, 2 ** 40, (n,), generator=g, dtype=torch.int64)
    assert bool((v.double().long() != v).all())
    if R is None:
        return []
    a = R.ints(v, 'incr_i64')
    R.call('fami_incr_i64', ptr(a), n, R.st)
    R.want('incr_i64(n %d)' % n, a, v + 1)
    b = R.ints(v, 'add_i64')
    R.call('fami_add_i64', ptr(b), ptr(R.ints(inc, 'add_i64 inc')), n, R.st)
    R.want('add_i64(n %d)' % n, b, v + inc)
    return R.end()


UNSCALE_CASES = [(1028 + r, k, bad) for r in range(4) for k in range(4) for bad in ((None,) if (r + k) % 2 else (None, 'inf', 'nan'))] + \
    [(3, 0, 'nan'), (4 * (CAP + 1) + 2, 0, None), (4 * (CAP + 1) + 2, 1, 'inf')]


def unscale_check(p, dt=None, R=None):
    """fami_unscale_check_f32: g *= f, the flag raised by an inf or a NaN (in the vector part, then in the scalar tail)"""
    n, moved, bad = p
    f = 2.0 ** -13
    g = gen('unscale', p)
    x = ints(g, (n,), -100, 100) * 8192
    assert representable(x * f, F32)
    if R is None:
        return []
    places = [None] if bad is None else sorted({5 % n if n < 8 else 5} | ({n - 1} if n % 4 else set()))
    for where in places:
        xx = x.clone()
        if where is not None:
            xx[where] = float(bad)
        arena = R.out((n,), F32, xx, 'gradient arena', moved)
        flag = R.ints(torch.zeros(2, dtype=torch.int32), 'flag')
        R.call('fami_unscale_check_f32', ptr(arena), n, f, ptr(flag), R.st)
        tag = 'unscale_check%s %s at %s' % (p, bad, where)
        R.want(tag + ' flag', flag, torch.tensor([0 if where is None else 1, 0], dtype=torch.int32))
        torch.cuda.synchronize(R.dev)
        got = arena.detach().cpu().double()
        w = x * f
        if where is not None:
            ok = (torch.isnan(got[where]) if bad == 'nan' else got[where] == float('inf'))
            if not bool(ok):
                R.fails.append(tag + ': the %s did not stay one' % bad)
            got[where] = w[where]
        if not torch.equal(got, w):
            R.fails.append(tag + ': %d elements differ' % int((got != w).sum()))
    return R.end()


def add_batch_chain(R=None):
    """fami_add_batch_f32 where a later pair's SOURCE is an earlier pair's output inside one 32-entry window: (a0 -> X), (X -> Y),
    (Y -> Z): the adds happen in call order, so Y receives X after its add"""
    n = 3000
    g = gen('chain')
    a0, X, Y, Z = (ints(g, (n,), -100, 100) for _ in range(4))
    want = (X + a0, Y + X + a0, Z + Y + X + a0)
    assert all(representable(w, F32) for w in want)
    if R is None:
        return []
    a = R.op(a0, F32)
    xs = [R.out((n,), F32, t, nm) for t, nm in ((X, 'X'), (Y, 'Y'), (Z, 'Z'))]
    chain = [a] + xs
    ptrs, counts = (ctypes.c_long * 6)(), (ctypes.c_int * 3)(n, n, n)
    for i in range(3):
        ptrs[2 * i], ptrs[2 * i + 1] = ptr(chain[i]), ptr(chain[i + 1])
    R.call('fami_add_batch_f32', ptrs, counts, 3, R.st)
    for got, w, nm in zip(xs, want, 'XYZ'):
        R.want('add_batch chain ' + nm, got, w)
    return R.end()


# ============================================================================================== csrc/core.hip: the linear kernels
LINEAR_MKN = [(M, K, N) for M in (1, 3, 4) for K in (1, 63, 64, 65, 144) for N in (1, 2, 13, 64)]
assert any((M * N) % 4 == 0 for M, K, N in LINEAR_MKN) and any((M * N) % 4 for M, K, N in LINEAR_MKN)
# backward: (M, K, N, dx, dw, db, acc_dx, acc_param) -- N = 2 the tail only, 64 the 8-wide main loop only, 13 both
LINEAR_BWD_CASES = [(M, K, N, 1, 1, 1, (i >> 1) & 1, i & 1) for i, (M, K, N) in enumerate((M, K, N) for M in (1, 3, 4) for K in (1, 65, 144) for N in (2, 13, 64))] + \
    [(3, 65, 13, 1, 1, 1, a, b) for a in (0, 1) for b in (0, 1)] + \
    [(3, 65, 13, 0, 1, 1, 0, 1), (3, 65, 13, 1, 0, 0, 1, 0), (4, 63, 13, 1, 0, 0, 0, 0), (3, 65, 13, 1, 1, 0, 0, 1), (4, 144, 64, 0, 1, 0, 0, 0)]


def _linear_operands(M, K, N):
    g = gen('linear', M, K, N)
    c = types.SimpleNamespace(x=ints(g, (M, K), -2, 2), w=ints(g, (N, K), -2, 2), b=ints(g, (N,), -2, 2), dy=ints(g, (M, N), -2, 2),
                              dx0=ints(g, (M, K), -4, 4), dw0=ints(g, (N, K), -4, 4), db0=ints(g, (N,), -4, 4))
    assert 4 * max(M, K, N) + 8 < EXACT32          # every sum of products of integers in [-2, 2], in any order
    return c


def linear_fwd(p, dt=None, R=None):
    """fami_linear_fwd_f32 with b null and non-null"""
    M, K, N = p
    c = _linear_operands(M, K, N)
    y = c.x @ c.w.t()
    if R is None:
        return []
    x, w, b = R.op(c.x, F32), R.op(c.w, F32), R.op(c.b, F32)
    for has_b in (0, 1):
        out = R.out((M, N), F32, None, 'y(b %d)' % has_b)
        R.call('fami_linear_fwd_f32', ptr(x), ptr(w), ptr(b) if has_b else None, ptr(out), M, K, N, R.st)
        R.want('linear_fwd%s b %d' % (p, has_b), out, y + c.b if has_b else y, '(m,n)')
    return R.end()


def linear_bwd(p, dt=None, R=None):
    """fami_linear_bwd_f32: any of dx / dw / db null (db only together with dw), acc_dx and acc_param independently"""
    M, K, N, do_dx, do_dw, do_db, acc_dx, acc_p = p
    c = _linear_operands(M, K, N)
    dx, dw, db = c.dy @ c.w, c.dy.t() @ c.x, c.dy.sum(0)
    if R is None:
        return []
    dxo = R.out((M, K), F32, c.dx0 if acc_dx else None, 'dx') if do_dx else None
    dwo = R.out((N, K), F32, c.dw0 if acc_p else None, 'dw') if do_dw else None
    dbo = R.out((N,), F32, c.db0 if acc_p else None, 'db') if do_db else None
    R.call('fami_linear_bwd_f32', ptr(R.op(c.dy, F32)), ptr(R.op(c.x, F32)), ptr(R.op(c.w, F32)), ptr(dxo), ptr(dwo), ptr(dbo), M, K, N, acc_dx, acc_p, R.st)
    tag = 'linear_bwd%s' % (p,)
    if do_dx:
        R.want(tag + ' dx', dxo, dx + (c.dx0 if acc_dx else 0), '(m,k)')
    if do_dw:
        R.want(tag + ' dw', dwo, dw + (c.dw0 if acc_p else 0), '(n,k)')
    if do_db:
        R.want(tag + ' db', dbo, db + (c.db0 if acc_p else 0), '(n,)')
    return R.end()


def linear_bwd_refusal(R):
    """db without dw was silently not computed: now -1, and nothing is written"""
    M, K, N = 3, 65, 13
    c = _linear_operands(M, K, N)
    dxo, dbo = R.out((M, K), F32, None, 'dx'), R.out((N,), F32, None, 'db')
    R.refused('fami_linear_bwd_f32', ptr(R.op(c.dy, F32)), ptr(R.op(c.x, F32)), ptr(R.op(c.w, F32)), ptr(dxo), None, ptr(dbo), M, K, N, 0, 0, R.st)
    R.want_untouched('refused linear_bwd dx', dxo)
    R.want_untouched('refused linear_bwd db', dbo)
    return R.end()


# ============================================================================================== csrc/loss.hip
WMSE_CASES = [(Rr, L, (i + j) % 2) for i, Rr in enumerate((1, 3, 257)) for j, L in enumerate((1, 255, 256, 257, 6912))] + [(3, 257, 0), (257, 255, 1)]


def wmse(p, dt=None, R=None):
    """fami_wmse_fwd_f32 (a power-of-two scale and the module's 1 / (B L J)) and fami_wmse_bwd_f32 (accumulate 0 / 1, gdev null /
    non-null).  Row sums are exact in fp32, their sum in fp64; the one rounding left is float32(sum64 * scale64)."""
    Rr, L, has_w = p
    g = gen('wmse', p)
    pred, gt = ints(g, (Rr, L), -4, 4), ints(g, (Rr, L), -4, 4)
    w = pick(g, (Rr,), [0, 0.5, 1, 2]) if has_w else torch.ones(Rr, dtype=F64)
    d = (pred - gt) * w[:, None]
    rows = (d * d).sum(1)
    assert multiple(d * d, 2) and rows.max().item() * 4 < EXACT32          # row sums below 2^24 quarter-units
    total = np.float64(rows.sum().item())
    scales = (2.0 ** -10, 1.0 / (1 * L) / Rr)          # JointMSELoss: 1.0 / (B * L) / J with B = 1, J = R
    want_loss = [np.float32(total * np.float64(s)) for s in scales]
    gscale, g0 = 2.0 ** -7, 8.0
    prior = ints(g, (Rr, L), -4, 4)
    grads = {(acc, hg): 2 * gscale * (g0 if hg else 1) * w[:, None] * d + (prior if acc else 0) for acc in (0, 1) for hg in (0, 1)}
    assert all(representable(v, F32) for v in grads.values())
    if R is None:
        return []
    pd, gd, wd = R.op(pred, F32), R.op(gt, F32), R.op(w, F32) if has_w else None
    for s, wl in zip(scales, want_loss):
        loss, ws = R.out((1,), F32, None, 'loss'), R.out((Rr,), F32, None, 'row sums')
        R.call('fami_wmse_fwd_f32', ptr(pd), ptr(gd), ptr(wd), ptr(loss), Rr, L, s, ptr(ws), R.st)
        R.want('wmse_fwd%s scale %r' % (p, s), loss, torch.tensor([float(wl)], dtype=F64))
        R.want('wmse_fwd%s row sums' % (p,), ws, rows)
    gdev = R.op(torch.tensor([g0], dtype=F64), F32)
    for (acc, hg), wg in grads.items():
        dp = R.out((Rr, L), F32, prior if acc else None, 'dpred(acc %d)' % acc)
        R.call('fami_wmse_bwd_f32', ptr(pd), ptr(gd), ptr(wd), ptr(dp), Rr, L, gscale, ptr(gdev) if hg else None, acc, R.st)
        R.want('wmse_bwd%s acc %d gdev %d' % (p, acc, hg), dp, wg, '(r,l)')
    return R.end()


ARGMAX_L = [1, 63, 256, 257, 6912]
NAN, INF = float('nan'), float('inf')


def argmax_rows(L):
    """-> (names, [R, L] float32 ndarray): rows in which the order of the reduction decides the answer"""
    rs = np.random.RandomState(L)
    base = lambda: rs.randint(-50, 50, L).astype(np.float32)
    rows = []

    def peaks(name, at, v=100.0, fill=None):
        if not (all(0 <= a < L for a in at) and len(set(at)) == len(at)):
            return None          # (the row needs a longer L)
        r = base() if fill is None else np.full(L, fill, np.float32)
        r[list(at)] = v
        rows.append((name, r))
        return r
    rows.append(('random', rs.permutation(L).astype(np.float32)))
    peaks('twice in one thread', (7, 7 + 256))
    peaks('twice in one thread, later trips', (300, 300 + 512, 300 + 1024))
    peaks('two lanes of one wave', (3, 40))
    peaks('two waves', (70, 200))
    peaks('two waves, the later one in the lower thread', (250, 256 + 3))          # thread 3 holds index 259, thread 250 index 250
    peaks('only the last element', (L - 1,))
    rows.append(('constant', np.full(L, 2.5, np.float32)))
    rows.append(('all -inf', np.full(L, -INF, np.float32)))
    peaks('+0.0 among -0.0', (L // 2,), 0.0, -0.0)
    peaks('one NaN', (L // 3,), NAN)
    r = peaks('the maximum, then one NaN', (1, L - 1), NAN)
    if r is not None:
        r[1] = 100.0
    peaks('two NaNs', (L - 1, L // 2), NAN)
    peaks('two NaNs in one thread', (260, 4), NAN)
    rows.append(('all NaN', np.full(L, NAN, np.float32)))
    return [n for n, _ in rows], np.stack([r for _, r in rows])


def argmax2d(L, dt=None, R=None):
    """fami_argmax2d_f32 with maxval null and non-null against oracle.ops.argmax_indices / get_max_preds (numpy: the first
    maximum, a NaN above every number, the first NaN among several)"""
    from oracle import ops as O
    names, hm = argmax_rows(L)
    Rr = hm.shape[0]
    idx = O.argmax_indices(hm[None])[0]
    _, mv = O.get_max_preds(hm[None, :, None, :])
    mv = mv.reshape(Rr)
    for nm, row, i, m in zip(names, hm, idx, mv):          # the reference does what the docstring says
        if np.isnan(row).any():
            assert np.isnan(m) and np.isnan(row[i]) and not np.isnan(row[:i]).any(), nm
        else:
            assert m == row.max() and row[i] == m and not (row[:i] == m).any(), nm
    if R is None:
        return []
    h = R.op(torch.from_numpy(hm).double(), F32)
    for has_mv in (0, 1):
        io = R.ints(torch.full((Rr,), -7, dtype=torch.int64), 'idx')
        mo = R.out((Rr,), F32, None, 'maxval') if has_mv else None
        R.call('fami_argmax2d_f32', ptr(h), ptr(io), ptr(mo), Rr, L, R.st)
        torch.cuda.synchronize(R.dev)
        gi = io.cpu().numpy()
        for r in np.nonzero(gi != idx)[0]:
            R.fails.append('argmax2d(L %d, maxval %d) row %r: index %d, reference %d' % (L, has_mv, names[r], gi[r], idx[r]))
        if has_mv:
            gm = mo.cpu().numpy()
            for r in np.nonzero(~((gm == mv) | (np.isnan(gm) & np.isnan(mv))))[0]:
                R.fails.append('argmax2d(L %d) row %r: maxval %r, reference %r' % (L, names[r], gm[r], mv[r]))
    return R.end()


# ---- final_preds: (H, W, an affine that is exact in fp32)
FINAL_CASES = [(8, 6, 1.5), (96, 72, 9.0)]          # s = 200 scale / W = 50 and 25: preds = center + (x - W / 2) s is exact for quarter pixels


def final_maps(H, W):
    """B = 2, J = 5 maps whose decode takes each side of 1 < px < W - 1 and 1 < py < H - 1, no shift, zeroing, ties, a NaN"""
    rs = np.random.RandomState(H * 100 + W)
    hm = rs.randint(1, 6, (10, H, W)).astype(np.float32)
    spots = [(1, 3), (2, 2), (W - 2, H - 2), (W - 1, 4), (3, 1), (3, H - 1), (3, 3)]
    for j, (px, py) in enumerate(spots):
        hm[j, py, px] = 50.0
    hm[6, 3, 2] = hm[6, 3, 4] = 7.0                      # no difference along x: no shift in x
    hm[7] = -rs.randint(0, 6, (H, W))                    # maximum <= 0: coordinates zeroed, px = 0, no shift
    hm[8, 2, 2] = hm[8, 4, 3] = hm[8, H - 3, 2] = 50.0   # ties: the first one
    hm[9, 4, 2] = 50.0
    hm[9, 5, 4] = NAN                                    # a NaN is the maximum: maxval NaN is not > 0, so the joint is zeroed
    return hm.reshape(2, 5, H, W), spots


def final_preds(p, dt=None, R=None):
    """fami_final_preds_f32 against oracle.ops.get_final_preds: maxvals and the pre-affine decision exactly (through an affine
    that fp32 carries exactly), preds at 1e-3 image pixels under a general centre and scale (fp32 against the float64 affine)"""
    from oracle import ops as O
    H, W, sc = p
    hm, spots = final_maps(H, W)
    exact_c, exact_s = np.array([[1000.0, 2000.0], [512.0, 256.0]], np.float32), np.array([[sc, sc], [sc, sc]], np.float32)
    any_c, any_s = np.array([[123.4, 234.5], [611.0, 87.25]], np.float32), np.array([[1.31, 1.75], [2.6, 3.1]], np.float32)
    s = sc * 200.0 / W
    assert s == int(s)
    ref_e, mv = O.get_final_preds(hm, exact_c, exact_s)
    ref_a, _ = O.get_final_preds(hm, any_c, any_s)
    coords = (ref_e - exact_c[:, None, :]) / s + np.array([W / 2.0, H / 2.0])          # the reference's decision before the affine
    quarter = np.round(coords * 4) / 4
    assert np.abs(coords - quarter).max() < 1e-9
    flat = quarter.reshape(10, 2)
    inner = [1 < px < W - 1 and 1 < py < H - 1 for px, py in spots[:6]]
    assert inner == [False, True, True, False, False, False]
    for j, (px, py) in enumerate(spots[:6]):          # the data does what it is there for: no shift on or outside the border
        assert np.abs(flat[j] - (px, py)).max() <= (0.25 if inner[j] else 0), j
    assert flat[6, 0] == 3 and tuple(flat[7]) == (0, 0) and np.abs(flat[8] - (2, 2)).max() <= 0.25
    assert tuple(flat[9]) == (0, 0) and np.isnan(mv.reshape(10)[9])
    if R is None:
        return []
    h = R.op(torch.from_numpy(hm).double(), F32)
    for tag, c, s_, ref in (('exact affine', exact_c, exact_s, None), ('general affine', any_c, any_s, ref_a)):
        preds, mo = R.out((2, 5, 2), F32, None, 'preds'), R.out((2, 5), F32, None, 'maxvals')
        ws = R.ints(torch.full((10,), -7, dtype=torch.int64), 'idx_ws')
        R.call('fami_final_preds_f32', ptr(h), ptr(R.op(torch.from_numpy(c).double(), F32)), ptr(R.op(torch.from_numpy(s_).double(), F32)),
               ptr(preds), ptr(mo), ptr(ws), 2, 5, H, W, R.st)
        torch.cuda.synchronize(R.dev)
        gp, gm = preds.cpu().numpy().astype(np.float64), mo.cpu().numpy().reshape(2, 5, 1)
        if not np.array_equal(gm, mv, equal_nan=True):
            R.fails.append('final_preds%s %s: maxvals %r, reference %r' % (p, tag, gm.ravel(), mv.ravel()))
        if ref is None:
            got = (gp - c[:, None, :]) / s + np.array([W / 2.0, H / 2.0])
            if not np.array_equal(got, quarter):
                R.fails.append('final_preds%s: pre-affine coordinates %r, reference %r' % (p, got.reshape(10, 2), flat))
        else:
            e = np.abs(gp - ref).max()
            if not e < 1e-3:
                R.fails.append('final_preds%s %s: %.3g image pixels from the reference' % (p, tag, e))
    return R.end()


# ---- pck_accuracy: (B, J, valid joints?)
PCK_CASES = [(B, J, 1) for B in (1, 3) for J in (1, 17, 64)] + [(3, 17, 0), (1, 1, 0)]


def pck_maps(B, J, valid):
    """H = W = 20 (norm 2: a one-pixel miss is a distance of exactly 0.5, which thr = 0.5 does not count), a joint without a
    valid target (coordinate <= 1), a prediction with a NaN"""
    H = W = 20
    rs = np.random.RandomState(B * 1000 + J * 10 + valid)
    pred, tgt = np.zeros((B, J, H, W), np.float32), np.zeros((B, J, H, W), np.float32)
    for b in range(B):
        for j in range(J):
            tx, ty = rs.randint(2, 18, 2)
            kind = (b + j) % 5
            if not valid or (J > 1 and j == 1):
                tx = 1 if (b + j) % 2 else tx          # x <= 1 or y <= 1: not a valid target
                ty = ty if (b + j) % 2 else 0
            dx, dy = [(0, 0), (1, 0), (0, -1), (1, 1), (0, 0)][kind]
            tgt[b, j, ty, tx] = 1.0
            pred[b, j, min(max(ty + dy, 0), H - 1), min(tx + dx, W - 1)] = 0.75
            if kind == 4 and J > 2:
                pred[b, j, 19, 19] = NAN          # the NaN wins the argmax, is not > 0, and zeroes the prediction: a miss
    return pred, tgt


def pck(p, dt=None, R=None):
    """fami_pck_accuracy_f32: all J + 3 outputs against oracle.ops.accuracy, each the fp64 figure rounded once"""
    from oracle import ops as O
    B, J, valid = p
    pred, tgt = pck_maps(B, J, valid)
    acc, avg, cnt, _ = O.accuracy(pred, tgt, 0.5)
    want = torch.tensor(list(acc) + [avg, cnt], dtype=F64)
    if valid:
        assert cnt == (J - 1 if J > 1 else 1) and (J == 1 or acc[2] == -1)
        assert B * J < 4 or 0 < avg < 1          # hits (distance 0) and misses (distance exactly 0.5 and beyond) both occur
    else:
        assert cnt == 0 and avg == 0 and acc[0] == 0 and (acc[1:] == -1).all()
    if R is None:
        return []
    out = R.out((J + 3,), F32, None, 'out')
    iws = R.ints(torch.full((2 * B * J,), -7, dtype=torch.int64), 'idx_ws')
    mws = R.out((2 * B * J,), F32, None, 'max_ws')
    R.call('fami_pck_accuracy_f32', ptr(R.op(torch.from_numpy(pred).double(), F32)), ptr(R.op(torch.from_numpy(tgt).double(), F32)), ptr(out), ptr(iws), ptr(mws),
           B, J, 20, 20, 0.5, R.st)
    R.want('pck_accuracy%s' % (p,), out, want, '(acc[0..J], avg, cnt)')
    return R.end()


# ---- Gaussian targets: (B, J, Hh, Wh, sigma)
GAUSS_CASES = [(2, 3, 7, 5, 1), (2, 3, 296, 296, 1)]
assert 2 * 3 * 296 * 296 > CAP


def gauss(p, dt=None, R=None):
    """fami_gauss_target_f32 and fami_gauss_target_ex_f32 (joint weights, quantised) between guards against
    oracle.ops.generate_heatmaps: the target at 1e-6, the weights exactly"""
    from oracle import ops as O
    B, J, Hh, Wh, sigma = p
    rs = np.random.RandomState(Hh + Wh)
    joints = rs.uniform(-8, 4 * max(Hh, Wh) + 8, (B, J, 2)).astype(np.float32)
    joints[0, 0] = (4 * 2 + 2, 4 * 3 + 2)          # x / 4 + 0.5 is an integer: the rounding of the reference
    joints[0, 1] = (-60.0, 10.0)                   # the window lies outside: weight 0
    vis = np.array([[1, 1, 1], [1, 0, 1]], np.float32)[:B, :J]
    jw = np.array([1.0, 2.0, 0.5], np.float32)[:J]
    rt, rw = [], []
    for b in range(B):
        j3 = np.concatenate([joints[b], np.zeros((J, 1), np.float32)], 1)
        t, w = O.generate_heatmaps(j3, np.repeat(vis[b][:, None], 3, 1), sigma, np.array([Wh * 4, Hh * 4]), np.array([Wh, Hh]), J)
        rt.append(t)
        rw.append(w.reshape(-1))
    rt, rw = np.stack(rt), np.stack(rw)
    assert rw[0, 1] == 0 and rw[1, 1] == 0 and rt[0, 0].max() == 1.0
    if R is None:
        return []
    jd, vd, jwd = R.op(torch.from_numpy(joints).double(), F32), R.op(torch.from_numpy(vis).double(), F32), R.op(torch.from_numpy(jw).double(), F32)
    for form in ('plain', 'ex'):
        tg, wt = R.out((B, J, Hh, Wh), F32, None, 'target'), R.out((B, J), F32, None, 'weight')
        if form == 'plain':
            R.call('fami_gauss_target_f32', ptr(jd), ptr(vd), ptr(tg), ptr(wt), B, J, Hh, Wh, Hh * 4, Wh * 4, sigma, R.st)
        else:
            R.call('fami_gauss_target_ex_f32', ptr(jd), ptr(vd), ptr(jwd), ptr(tg), ptr(wt), B, J, Hh, Wh, Hh * 4, Wh * 4, sigma, 0, R.st)
        torch.cuda.synchronize(R.dev)
        e = np.abs(tg.cpu().numpy().astype(np.float64) - rt)
        if not np.nanmax(e) < 1e-6 or np.isnan(e).any():
            R.fails.append('gauss_target%s %s: target off by %.3g (%d NaN)' % (p, form, np.nanmax(e), int(np.isnan(e).sum())))
        R.want('gauss_target%s %s weight' % (p, form), wt, torch.from_numpy(rw * (jw[None] if form == 'ex' else 1)).double(), '(b,j)')
    return R.end()


# ---- softmax_kl: the one family with a tolerance
KL_L = [1, 2, 255, 256, 257, 4095, 4096, 4097, 8192, 8193]
KL_R = [1, 3, 257]
KL_T = 0.05
KL_FLOOR = 2.0 ** -20
KL_MARGIN = 8.0


def kl_reference(Rr, L):
    """operands (randn * 0.2, fp32 values) and, from oracle.ops.softmax_kl_rows in fp64 and in fp32: value, gradient, and the row
    statistics restated the way the kernel defines them (shifted by the fp32 row maxima, which are exact)"""
    from oracle import ops as O
    g = gen('kl', Rr, L)
    a = (torch.randn(Rr, L, generator=g) * 0.2).float()
    b = (torch.randn(Rr, L, generator=g) * 0.2).float()
    prior = ints(g, (Rr, L), -4, 4)
    c = types.SimpleNamespace(a=a, b=b, prior=prior)
    for nm, dtype in (('r64', F64), ('r32', F32)):
        bb = b.to(dtype).requires_grad_(True)
        v = O.softmax_kl_rows(a.to(dtype), bb, KL_T)
        v.backward()
        T = torch.tensor(KL_T, dtype=F32).to(dtype)          # the kernel divides by float32(0.05)
        ma, mb = (a / torch.tensor(KL_T, dtype=F32)).max(1).values.to(dtype), (b / torch.tensor(KL_T, dtype=F32)).max(1).values.to(dtype)
        ea, eb = torch.exp(a.to(dtype) / T - ma[:, None]), torch.exp(b.to(dtype) / T - mb[:, None])
        sa, sb = ea.sum(1), eb.sum(1)
        pa, t = ea / sa[:, None], eb / sb[:, None]
        S = (t * (torch.log(t) + 1 - pa)).sum(1)
        setattr(c, nm, types.SimpleNamespace(value=v.detach(), grad=bb.grad.detach(), ma=ma, mb=mb, sa=sa, sb=sb, S=S))
    return c


def kl_gscale(Rr, L):
    """a power of two that brings the gradient (about gscale / (R L^2 T)) to the order of the prior's small integers"""
    return 2.0 ** int(np.ceil(np.log2(Rr * L * L * KL_T)))


def rel(got, ref):
    got, ref = got.detach().double(), ref.detach().double()
    return float((got - ref).abs().max() / ref.abs().max().clamp(min=1e-300))


def rowrel(got, ref):
    """per element |got - ref| over the row's max |ref| -> the largest"""
    return float(((got.double() - ref.double()).abs() / ref.double().abs().max(1, keepdim=True).values.clamp(min=1e-300)).max())


def softmax_kl(p, dt=None, R=None, report=None):
    """fami_softmax_kl_fwd_f32 / _bwd_f32 (accumulate 0 / 1, gdev null / non-null).  The bound of every figure is 8 x the error
    of the fp32 CPU evaluation against the fp64 one on the same operands (the kernel sums a row in another order and uses the
    device's expf / logf, each good to a few ulp), with a floor of 2^-20 for the rows where fp32 happens to be exact (L = 1).
    ma and mb are exact: a correctly rounded division and a maximum."""
    Rr, L = p
    c = kl_reference(Rr, L)
    r64, r32 = c.r64, c.r32
    gs, g0 = kl_gscale(Rr, L), 0.5
    yard = {'value': rel(r32.value.reshape(1), r64.value.reshape(1))}
    for k in ('sa', 'sb', 'S'):
        yard[k] = rel(getattr(r32, k), getattr(r64, k))
    want, yard_g = {}, {}
    for acc in (0, 1):
        for hg in (0, 1):
            f = gs * (g0 if hg else 1.0)
            want[acc, hg] = r64.grad * f + (c.prior if acc else 0)
            fp32 = r32.grad * torch.tensor(f, dtype=F32) + (c.prior.float() if acc else 0)
            yard_g[acc, hg] = rowrel(fp32, want[acc, hg])
    assert all(np.isfinite(v) for v in list(yard.values()) + list(yard_g.values()))
    if R is None:
        return []
    bound = lambda y: max(KL_MARGIN * y, KL_FLOOR)
    a, b = R.op(c.a.double(), F32), R.op(c.b.double(), F32)
    value, stats, ws = R.out((1,), F32, None, 'value'), R.out((Rr, 5), F32, None, 'stats'), R.out((Rr,), F32, None, 'row values')
    R.call('fami_softmax_kl_fwd_f32', ptr(a), ptr(b), ptr(value), ptr(stats), Rr, L, KL_T, ptr(ws), R.st)
    torch.cuda.synchronize(R.dev)
    st = stats.cpu()
    tag = 'softmax_kl(R %d, L %d)' % p
    line = {'R': Rr, 'L': L}
    e = rel(value.cpu(), r64.value.reshape(1))
    line['value'] = (e, yard['value'])
    if not e <= bound(yard['value']):
        R.fails.append('%s value: relative error %.3g, fp32 yardstick %.3g' % (tag, e, yard['value']))
    for col, k in ((0, 'ma'), (2, 'mb')):
        if not torch.equal(st[:, col], getattr(r32, k)):
            R.fails.append('%s %s differs from max(x / T) in fp32' % (tag, k))
    for col, k in ((1, 'sa'), (3, 'sb'), (4, 'S')):
        e = rel(st[:, col], getattr(r64, k))
        line[k] = (e, yard[k])
        if not e <= bound(yard[k]):
            R.fails.append('%s %s: relative error %.3g, fp32 yardstick %.3g' % (tag, k, e, yard[k]))
    gdev = R.op(torch.tensor([g0], dtype=F64), F32)
    worst = (0.0, 0.0)
    for (acc, hg), w in want.items():
        d = R.out((Rr, L), F32, c.prior if acc else None, 'dBt(acc %d)' % acc)
        R.call('fami_softmax_kl_bwd_f32', ptr(a), ptr(b), ptr(stats), ptr(d), Rr, L, KL_T, gs, ptr(gdev) if hg else None, acc, R.st)
        torch.cuda.synchronize(R.dev)
        e = rowrel(d.cpu(), w)
        if e >= worst[0]:
            worst = (e, yard_g[acc, hg])
        if not e <= bound(yard_g[acc, hg]):
            R.fails.append('%s gradient(acc %d, gdev %d): %.3g of the row maximum, fp32 yardstick %.3g' % (tag, acc, hg, e, yard_g[acc, hg]))
    line['grad'] = worst
    if report is not None:
        report.append(line)
    return R.end()


# every family and its cases: tests/test_stream_exact_host.py walks this table
TYPED = [(layout, LAYOUT_CASES), (pack_frames, PACK_CASES), (copy_channels, COPY_CASES), (cat_split, CAT_CASES), (axpby, AXPBY_CASES),
         (cast_widen_fill, FLAT_CASES), (fuse_sum, FUSE_CASES), (relu_bwd, RELU_CASES), (pool_relu_bwd, POOL_CASES)]
UNTYPED = [(scale_pairs, SCALE_PAIRS_CASES), (i64_ops, I64_CASES), (unscale_check, UNSCALE_CASES), (linear_fwd, LINEAR_MKN), (linear_bwd, LINEAR_BWD_CASES),
           (wmse, WMSE_CASES), (argmax2d, ARGMAX_L), (final_preds, FINAL_CASES), (pck, PCK_CASES), (gauss, GAUSS_CASES),
           (softmax_kl, [(Rr, L) for L in KL_L for Rr in KL_R])]
