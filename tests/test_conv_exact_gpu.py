"""Every convolution route held to EXACT integer results, with guard zones behind every output and NaN around every operand.

Operands are small integers (tests/_conv_exact.py: x, dy, w in {-1, 0, 1}; bias, addend and the prior content of an
accumulated output in [-4, 4]), so every partial sum is an integer below 2^24 and fp32 accumulation is exact in any order --
on the f32 MFMA, the bf16 / fp16 MFMAs, through split-K atomics, slab reduces and the split-product route.  The reference is
fp64 on the CPU (F.conv2d, F.conv_transpose2d, autograd for dW); every comparison is torch.equal, there is no tolerance in
this module.  The bounds that make this true (|value| <= 256 for 16-bit activations, < 2^24 for fp32 results and for the
fp32 partial sums of the statistics epilogues) are asserted on the reference before any launch.  One dense tier per storage
type (operands in [-2, 2], the largest K of the file) leaves the exact range of bf16 on purpose: its reference is the fp64
result converted with round-to-nearest-even, the conversion csrc/common.h documents for the kernels' stores.

Each output (y, dx, dW, the weight-gradient workspace, the fp64 slot rows) is a 256-byte aligned view into a larger buffer
with 4096 elements of a sentinel in front and behind, which must be bit-for-bit intact after the launch (include/fami.h
promises callers no slack on any pointer); each operand (x, dy, z, bias, addend, packed weights) sits the same way inside
NaN, so a neighbour fetched where zero padding belongs, or a channel / pixel tail read into an MFMA lane, poisons an output.

Each case runs on every route that claims its geometry, selected with the knobs of include/fami.h; where the library offers
a query (fami_conv_t5_eligible, fami_conv_t6_eligible, fami_conv2d_bwd_pair_ok*, fami_conv2d_bwd_pair_key*,
fami_conv2d_xbn_ok*) the query is asserted, and the cases taken per route are counted: at least three geometries per route,
at least one of them with a ragged last band, unit or tile.

Left out: fami_conv2d_fwd_xbn_*, fami_conv2d_fwd_bnin_* and fami_conv2d_wgrad_defer_xbn_*.  They compute mean and invstd
from statistics inside the launch (a division and a reciprocal square root: not exact arithmetic); the bit-for-bit tests
against their two-launch forms in test_kernels_half_gpu.py / test_fused_bn_gpu.py keep holding them."""
import ctypes

import pytest
import torch

from _conv_exact import STATS_VARIANTS, Runner, make_case

pytestmark = pytest.mark.gpu

TYPES = ['f32', 'bf16', 'f16']
HALF = ['bf16', 'f16']


def g3(N, H, W, Ci, Co):
    """3x3, stride 1, pad 1"""
    return (N, H, W, Ci, Co, 3, 1, 1, 1)


# (geometry, ragged: the last band / unit / tile / K step of the route's kernels is partial on it)
GENERIC = [((1, 5, 7, 20, 36, 3, 1, 1, 1), 1), ((2, 5, 3, 16, 16, 3, 1, 1, 1), 1), ((3, 7, 5, 16, 16, 3, 2, 1, 1), 1),
           ((2, 13, 9, 96, 192, 3, 2, 1, 1), 1), ((1, 9, 7, 36, 72, 1, 1, 0, 1), 1), ((2, 10, 9, 48, 48, 3, 1, 0, 1), 0),
           ((2, 10, 9, 48, 64, 3, 1, 2, 1), 1), ((2, 11, 7, 64, 48, 5, 1, 2, 1), 1), ((2, 12, 9, 48, 216, 3, 1, 3, 3), 1),
           ((2, 12, 9, 48, 108, 3, 1, 3, 3), 1), ((2, 12, 9, 48, 17, 1, 1, 0, 1), 1), ((2, 6, 5, 384, 384, 3, 1, 1, 1), 1),
           ((2, 16, 12, 3, 64, 3, 2, 1, 1), 0), ((1, 6, 5, 384, 384, 3, 1, 1, 1), 1), ((3, 5, 3, 384, 384, 3, 1, 1, 1), 1),
           ((1, 7, 5, 32, 64, 3, 1, 1, 1), 1), ((2, 12, 9, 96, 48, 3, 1, 1, 1), 1)]
BAND = [(g3(1, 1, 1, 16, 48), 1), (g3(2, 3, 40, 48, 48), 1), (g3(3, 17, 5, 144, 96), 1), (g3(2, 24, 18, 48, 48), 1),
        (g3(1, 7, 33, 32, 144), 1), (g3(2, 16, 12, 64, 64), 0)]
DILATED = [((2, 12, 9, 48, 216, 3, 1, 3, 3), 1), ((2, 12, 9, 48, 108, 3, 1, 3, 3), 1), ((1, 11, 7, 48, 48, 3, 1, 2, 2), 1),
           ((2, 8, 16, 32, 96, 3, 1, 3, 3), 0)]

FWD_VARIANTS = [(0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 1, 1, 0), (1, 0, 0, 1)]     # bias, addend, relu, accumulate
KNOB = {'lds': 'fami_conv_tune_lds', 'wg': 'fami_conv_tune_wgrad_lds', 'st': 'fami_conv_tune_stages'}
# The shims decode a code by its range, and a code past the end of one range lands silently in another knob (8700 + 500 would set
# the f32 band kernel's minimum workgroups): only the codes of include/fami.h that this module uses, with their value ranges.
CODES = {'lds': [(0, 1), (21, 21), (30, 31), (42, 42), (52, 53), (60, 62), (101, 116), (7000, 7001), (7101, 7116), (7401, 7401), (7501, 7599),
                 (7600, 7600), (8000, 8001), (8102, 8116), (8201, 8202), (8400, 8400), (8500, 8501), (8601, 8699), (8701, 8995), (9001, 9001)],
         'wg': [(0, 1), (50, 51), (20000, 20003), (23000, 23009), (23101, 23399), (24000, 24001), (25000, 25001), (30000, 30001)],
         'st': [(100, 101), (110, 111)]}


def _lib():
    from fami_pose_amd._lib import lib
    return lib()


def tune(knobs):
    """the library defaults, then the route's knobs in order"""
    L = _lib()
    L.bind(None)
    L.cdll.fami_tune_reset()
    for fn, code in knobs:
        assert any(lo <= code <= hi for lo, hi in CODES[fn]), 'knob %s(%d) is outside the ranges this module knows' % (KNOB[fn], code)
        getattr(L.cdll, KNOB[fn])(code)


def run_passes(r, fwd=1, dgrad=1, wgrad=1, stats=1, addend=1, defer=1):
    """every entry point of section 2 of the route's kernels on one Runner -> failure texts"""
    N, H, W, Ci, Co = r.geo[:5]
    out_f32 = int(r.half and Co == 17)              # (the heatmap layers: fp32 output in 16-bit mode)
    fails = []
    if fwd:
        seen = set()
        for b, a, rl, ac in FWD_VARIANTS:
            a = a if (addend and not r.half) else 0          # (only the f32 entry points take an addend)
            if (b, a, rl, ac) not in seen:
                seen.add((b, a, rl, ac))
                fails += r.fwd(b, a, rl, ac, out_f32)
        if stats and Co % 4 == 0 and not out_f32:
            for bias, pivot in STATS_VARIANTS:
                fails += r.fwd_stats(bias, pivot)
    if dgrad:
        fails += r.dgrad(0, 0) + r.dgrad(0, 1)
        if addend and not r.half:
            fails += r.dgrad(1, 0)
        if stats and Ci % 4 == 0:
            for relu in (0, 1, 2):
                for acc in (0, 1):
                    fails += r.dgrad_bnstats(relu, acc)
    if wgrad:
        fails += r.wgrad(0) + r.wgrad(1)
        if defer:
            fails += r.wgrad_deferred(3)
    return fails


def drive(dev, dt, route, knobs, cases, claims=None, query=None, passes=run_passes, need=3, need_ragged=1, **kw):
    """Run `passes` for every (geometry, ragged) of `cases` the route claims, under the route's knobs.  claims(geo) -> bool:
    the geometry rule of include/fami.h for routes without a query; query(L, geo) -> bool: the library's own answer, which
    decides (a variant the library does not route there is not run).  Asserts the per-route counts of the cases that were
    launched and returns them.  For a route with neither (the direct kernels, the stem kernels, the DMA-staged stride-2 / dilated /
    wide 1x1 weight gradients) the library offers no query: that its cases reach the intended kernel rests on the geometry rules
    of the plan functions in csrc/ as read when the lists were written -- a probe in the C ABI would be the way to assert it."""
    L = _lib()
    taken = ragged = 0
    try:
        for geo, rag in cases:
            if claims is not None and not claims(geo):
                continue
            tune(knobs)
            if query is not None and not query(L, geo):
                continue
            r = Runner(dev, dt, make_case(geo))
            fails = passes(r, **kw)
            assert not fails, 'route %s, storage %s, geometry (N,H,W,Ci,Co,k,stride,pad,dil) = %s:\n  %s' % (route, dt, geo, '\n  '.join(fails))
            taken += 1
            ragged += rag
    finally:
        L.cdll.fami_tune_reset()
    assert taken >= need and ragged >= need_ragged, 'route %s (%s): %d geometries taken, %d ragged' % (route, dt, taken, ragged)
    return taken, ragged


def is3x3(geo):
    return geo[5:] == (3, 1, 1, 1)


# ------------------------------------------------------------------------------------------------- implicit GEMM + defaults
IGEMM_ROUTES = {
    # direct implicit GEMM in its linear-address form, parity-class stride-2 input gradient, scalar-operand weight gradients
    'direct-linear': ([('lds', 0), ('st', 101), ('st', 111), ('wg', 0)], None),
    # ... in the general form, all-taps stride-2 input gradient, the general per-tap f32 weight-gradient kernel
    'direct-general': ([('lds', 0), ('st', 100), ('st', 110), ('wg', 0), ('wg', 50)], None),
    # the LDS-staged kernels (the register-blocked one with its exact-f32 instance, explicit tiles per band; the DMA kernels of
    # conv_t6.hip off so that the older staged kernels run) and the LDS-staged weight gradients (the pipelined, DMA-staged and
    # split-product kernels off: they come first wherever they are eligible)
    'lds-staged': ([('lds', 1), ('lds', 21), ('lds', 112), ('lds', 30), ('lds', 8000), ('lds', 8500), ('wg', 1), ('wg', 20000), ('wg', 23000), ('wg', 24000), ('wg', 25000), ('wg', 30000)],
                   lambda g: is3x3(g) and (g[4] % 48 == 0 or g[4] % 64 == 0) and g[3] % 16 == 0),
    # the library's default routes without the launch-size rules (small cases): persistent / weight-resident / dilated band kernels
    'default': ([('lds', 7600), ('lds', 7401), ('lds', 8400), ('lds', 42)], None),
}


@pytest.mark.parametrize('dt', TYPES)
@pytest.mark.parametrize('route', list(IGEMM_ROUTES))
def test_generic_kernels_are_exact(dev, dt, route):
    """The 13 generic geometries of the suite (channel tails, odd maps, stride 2, no / extra padding, 5x5, dilation 3, the
    17-channel fp32-output head, the stem) plus split-K ones (384 channels on 6x5 / 5x3 maps: K split over workgroups): forward
    (plain, bias, addend, ReLU, accumulate, bias + addend + ReLU, bias + accumulate), input gradient (plain, addend,
    accumulate), weight gradient (immediate: fresh / accumulating; deferred: several reduces in one batch), the forward
    statistics epilogue (NULL and integer pivot) and the backward statistics epilogue (ReLU modes 0 / 1 / 2, fresh /
    accumulating)."""
    knobs, claims = IGEMM_ROUTES[route]
    # (GENERIC holds three stride-2 and three 384-channel geometries for the stride-2 input-gradient forms and split-K; no query
    #  tells which tile / split a launch took, so nothing here can assert that those sub-routes ran)
    drive(dev, dt, route, knobs, GENERIC, claims)


# ------------------------------------------------------------------------------------------------- f32 band kernel (conv_t4.hip)
def _s3_band(L, geo):
    return L.cdll.fami_conv2d_xbn_ok_f32(*geo[:5]) == 1      # (both split-product kernels would take the shape)


T4_ROUTES = {
    'band-exact-f32': ([('lds', 7000), ('lds', 30), ('lds', 21), ('lds', 112)], None),
    'band-split-2tiles': ([('lds', 7000), ('lds', 31), ('lds', 60), ('lds', 52)], _s3_band),
    'band-split-3tiles': ([('lds', 7000), ('lds', 31), ('lds', 60), ('lds', 53)], _s3_band),
    'band-split-producer-consumer': ([('lds', 7000), ('lds', 31), ('lds', 62), ('lds', 53)], _s3_band),
    'band-split-bt1': ([('lds', 7000), ('lds', 31), ('lds', 60), ('lds', 101)], _s3_band),
    'band-split-bt5': ([('lds', 7000), ('lds', 31), ('lds', 62), ('lds', 105)], _s3_band),
    'band-split-bt7': ([('lds', 7000), ('lds', 31), ('lds', 60), ('lds', 52), ('lds', 107)], _s3_band),
}


@pytest.mark.parametrize('route', list(T4_ROUTES))
def test_f32_band_kernel_is_exact(dev, route):
    """conv_t4.hip in f32 storage: the exact-MFMA instance and the split-product instance (two / three pixel tiles per wave,
    the producer / consumer form, forced tiles per band) with the persistent kernel off -- forward and input gradient with
    their epilogues; one-pixel maps, maps narrower than a tile, ragged last bands."""
    knobs, query = T4_ROUTES[route]
    cases = BAND + [(g, rg) for g, rg in GENERIC if is3x3(g) and g[4] % 16 == 0 and g[3] % 16 == 0]
    drive(dev, 'f32', route, knobs, cases, claims=lambda g: g[4] % 48 == 0 or g[4] % 64 == 0, query=query, wgrad=0, addend=0)


@pytest.mark.parametrize('dt', TYPES)
def test_dilated_band_kernel_is_exact(dev, dt):
    """The dilated 3x3 band kernels (padding = dilation: the 48 -> 216 / 108 predictors of the alignment head, and a dilation-2
    one-frame odd map), on every eligible launch (fami_conv_tune_lds(42)), with the dilated DMA-staged weight gradient."""
    drive(dev, dt, 'band-dilated', [('lds', 42), ('wg', 23009)], DILATED, stats=0)


# ------------------------------------------------------------------------------------------------- f32 persistent kernel (conv_t5.hip)
T5_CASES = BAND + [(g3(1, 9, 33, 48, 96), 1), (g3(2, 5, 7, 96, 144), 1)]


@pytest.mark.parametrize('rows,maxwg', [(0, 0), (1, 0), (2, 1), (3, 3), (5, 12), (0, 1), (2, 12), (5, 0)])
def test_f32_persistent_kernel_is_exact(dev, rows, maxwg):
    """conv_t5.hip: the persistent split-product kernel without its launch-size rules, rows per band forced to 1 / 2 / 3 / 5, grid
    size forced to 8 / 24 / 96 workgroups -- forward and input gradient with their epilogues (the one-launch backward pair of f32
    storage, whose input-gradient half is this kernel: test_backward_pair_is_exact)."""
    knobs = [('lds', 7001), ('lds', 7600), ('lds', 7401)] + ([('lds', 7100 + rows)] if rows else []) + ([('lds', 7500 + maxwg)] if maxwg else [])
    drive(dev, 'f32', 'persistent(rows=%d,maxwg=%d)' % (rows, maxwg), knobs, T5_CASES,
          query=lambda L, g: L.cdll.fami_conv_t5_eligible(*g[:5]) == 1, wgrad=0, addend=0)


# ------------------------------------------------------------------------------------------------- 16-bit conv_t6.hip
# (geometry, rows per band, units knob of the 48-channel kernel | workgroup target of the phased kernel, ragged)
T6_48 = [(g3(1, 10, 72, 48, 48), 0, 0, 1), (g3(2, 8, 72, 48, 48), 2, 0, 1), (g3(2, 8, 72, 48, 48), 4, 1, 1), (g3(3, 16, 64, 48, 48), 8, 2, 0),
         (g3(2, 16, 64, 48, 96), 0, 0, 0), (g3(2, 8, 72, 48, 48), 4, 2, 1)]
T7_48 = [(g3(3, 12, 9, 96, 144), 6, 0, 1), (g3(2, 24, 18, 144, 96), 4, 1, 1), (g3(1, 10, 72, 96, 48), 2, 0, 1), (g3(3, 12, 9, 96, 48), 0, 290, 1),
         (g3(2, 11, 9, 96, 48), 1, 0, 1), (g3(1, 11, 11, 96, 144), 0, 0, 1)]          # (odd x odd maps: one row per band / the plan's choice)
T7_32 = [(g3(1, 10, 72, 64, 64), 2, 0, 1), (g3(3, 12, 9, 128, 192), 6, 290, 1), (g3(2, 16, 36, 256, 64), 8, 3, 0), (g3(2, 24, 18, 64, 128), 4, 1, 1),
         (g3(2, 11, 9, 128, 64), 1, 0, 1), (g3(3, 7, 13, 64, 64), 0, 0, 1)]


def _pair_passes(r):
    fails = r.bwd_pair(0, 0, None) + r.bwd_pair(1, 1, None)
    if r.half:
        fails += r.bwd_pair(0, 0, 2) + r.bwd_pair(1, 1, 1) + r.bwd_pair(0, 1, 0)
    return fails


@pytest.mark.parametrize('dt', HALF)
@pytest.mark.parametrize('kernel', ['weight-resident-48', 'phased-48', 'phased-32'])
def test_dma_staged_16bit_kernels_are_exact(dev, dt, kernel):
    """conv_t6.hip: the 48-channel weight-resident kernel (rows per band 2 / 4 / 8, units of two / four rows, the ninth tile of
    72-pixel rows) and the phased kernel in its 48-channel-phase and 32-channel-phase variants (rows per band, workgroup
    targets), without the minimum job count -- forward and input gradient with their epilogues."""
    table, want = {'weight-resident-48': (T6_48, 1), 'phased-48': (T7_48, 2), 'phased-32': (T7_32, 3)}[kernel]
    taken = ragged = 0
    for geo, rows, mt, rag in table:
        knobs = [('lds', 8001), ('lds', 8501), ('lds', 8400)]
        if rows:
            knobs.append(('lds', (8100 if want == 1 else 8600) + rows))
        if mt:
            knobs.append(('lds', (8200 if want == 1 else 8700) + mt))
        name = '%s(rows=%d,%s=%d)' % (kernel, rows, 'units' if want == 1 else 'target', mt)
        # (need = 1: the query must return this kernel under these knobs, or the row fails; the counts are of launched cases)
        tk, rg = drive(dev, dt, name, knobs, [(geo, rag)], query=lambda L, g: L.cdll.fami_conv_t6_eligible(*g[:5]) == want, need=1,
                       need_ragged=0, wgrad=0, addend=0)
        taken += tk
        ragged += rg
    assert taken >= 3 and ragged >= 1, (kernel, dt, taken, ragged)


# ------------------------------------------------------------------------------------------------- stem
STEM_FWD = [((2, 16, 12, 3, 64, 3, 2, 1, 1), 0), ((3, 38, 26, 3, 64, 3, 2, 1, 1), 1), ((1, 17, 23, 3, 64, 3, 2, 1, 1), 1)]
STEM_WG = [((3, 16, 288, 3, 64, 3, 2, 1, 1), 0), ((2, 8, 144, 3, 64, 3, 2, 1, 1), 0), ((1, 12, 96, 3, 64, 3, 2, 1, 1), 0), ((1, 4, 287, 3, 64, 3, 2, 1, 1), 1)]


@pytest.mark.parametrize('dt', TYPES)
def test_stem_forward_is_exact(dev, dt):
    """conv_stem.hip: the 3 -> 64 stride-2 forward with K dense over (tap, channel), every storage type; odd maps (border taps
    on every side, a ragged last pixel tile), one frame."""
    drive(dev, dt, 'stem-forward', [('lds', 9001)], STEM_FWD, dgrad=0, wgrad=0, addend=0)


@pytest.mark.parametrize('dt', HALF)
def test_stem_weight_gradient_is_exact(dev, dt):
    """conv_wgrad_stem_kernel: units of 288 output pixels (whole rows) -- two / four / six rows per unit, an odd input width."""
    drive(dev, dt, 'stem-weight-gradient', [('wg', 25001)], STEM_WG, fwd=0, dgrad=0)


# ------------------------------------------------------------------------------------------------- weight gradients
WG_3X3 = [(g3(3, 8, 64, 48, 48), 0), (g3(2, 12, 72, 48, 96), 0), (g3(3, 12, 9, 96, 48), 1), (g3(3, 24, 18, 48, 144), 1),
          (g3(3, 12, 9, 128, 64), 1), (g3(2, 24, 72, 128, 64), 0), (g3(1, 12, 9, 96, 48), 1), (g3(2, 16, 36, 48, 48), 0), (g3(2, 13, 9, 96, 96), 1)]
WG_ODD = [(g3(1, 7, 5, 32, 64), 1), (g3(2, 5, 3, 16, 16), 1), (g3(3, 17, 5, 144, 96), 1), (g3(1, 7, 33, 32, 144), 1), (g3(2, 12, 9, 96, 48), 1)]
# the DMA-staged kernel's units are whole output rows, 104 ... 288 pixels in K steps of 32: (2, 24, 36) -> six rows of 18 = 108 pixels,
# a last K step padded with 20 zero rows; (2, 16, 32) -> 128 pixels, no padding; 64-channel blocks: 80 pixels in three K steps
WG_S2 = [((2, 24, 36, 48, 96, 3, 2, 1, 1), 1), ((1, 23, 35, 96, 48, 3, 2, 1, 1), 1), ((2, 16, 32, 48, 48, 3, 2, 1, 1), 0), ((2, 20, 32, 64, 64, 3, 2, 1, 1), 1),
         ((1, 19, 31, 64, 64, 3, 2, 1, 1), 1)]
# ... dilated: five K steps (144 pixels padded to 160, or 160)
WG_DIL = [((2, 24, 18, 48, 216, 3, 1, 3, 3), 1), ((1, 16, 10, 48, 108, 3, 1, 3, 3), 0), ((3, 16, 36, 96, 52, 3, 1, 2, 2), 1), ((1, 20, 8, 48, 48, 3, 1, 3, 3), 0)]
WG_1X1 = [((7, 101, 97, 128, 64, 1, 1, 0, 1), 1), ((9, 96, 80, 64, 128, 1, 1, 0, 1), 0), ((1, 256, 257, 64, 64, 1, 1, 0, 1), 1)]


def _wg6(L, geo):
    out = (ctypes.c_int * 9)()
    L.cdll.fami_conv2d_bwd_pair_key(*geo[:5], out)
    return out[5] != 0          # (KS of the DMA-staged weight-gradient kernel: it takes the launch)


WG_ROUTES = {
    # name: (storage types, knobs, cases, claims, query)
    'scalar-operand': (HALF, [('wg', 0)], WG_ODD + GENERIC[:5] + DILATED[:2], None, None),
    'lds-staged': (TYPES, [('wg', 1), ('wg', 20000), ('wg', 23000), ('wg', 24000), ('wg', 25000), ('wg', 30000)], WG_ODD + WG_3X3[:3], lambda g: is3x3(g) and g[3] % 16 == 0 and g[4] % 16 == 0, None),
    'f32-per-tap-general': (['f32'], [('wg', 0), ('wg', 30000), ('wg', 50)], WG_ODD + GENERIC[:5] + DILATED[:3], None, None),
    'f32-per-tap-linear': (['f32'], [('wg', 0), ('wg', 30000), ('wg', 51)], WG_ODD + DILATED[:3], lambda g: g[6] == 1 and g[3] % 16 == 0 and g[4] % 16 == 0 and g[2] >= 4, None),
    'pipelined-16bit': (HALF, [('wg', 20001), ('wg', 20003), ('wg', 23000), ('wg', 24000), ('wg', 25000)], WG_ODD + WG_S2[:2] + DILATED[:2] + [((2, 9, 7, 48, 96, 1, 1, 0, 1), 1)],
                        lambda g: g[3] % 16 == 0 and g[4] % 4 == 0 and g[5] in (1, 3) and g[7] == g[8] * (g[5] - 1) // 2, None),
    'f32-split-product': (['f32'], [('wg', 30001)], WG_ODD + WG_3X3[:4], None, lambda L, g: L.cdll.fami_conv2d_xbn_ok_f32(*g[:5]) == 1),
    'dma-staged-3x3': (HALF, [('wg', 23001), ('wg', 23003)], WG_3X3, None, _wg6),
    'dma-staged-3x3-units1': (HALF, [('wg', 23001), ('wg', 23003), ('wg', 23101)], WG_3X3, None, _wg6),
    'dma-staged-3x3-units2': (HALF, [('wg', 23001), ('wg', 23003), ('wg', 23102)], WG_3X3, None, _wg6),
    'dma-staged-3x3-units5': (HALF, [('wg', 23001), ('wg', 23003), ('wg', 23105)], WG_3X3, None, _wg6),
    'dma-staged-stride2': (HALF, [('wg', 23001), ('wg', 23005)], WG_S2, None, None),
    'dma-staged-dilated': (HALF, [('wg', 23001), ('wg', 23009)], WG_DIL, None, None),
    'dma-staged-wide-1x1': (HALF, [('wg', 24001)], WG_1X1, None, None),
}


@pytest.mark.parametrize('route,dt', [(r, d) for r in WG_ROUTES for d in WG_ROUTES[r][0]])
def test_weight_gradient_routes_are_exact(dev, route, dt):
    """dW, fresh and accumulating, immediate and deferred (three reduces in one fami_wgrad_reduce_batch call), on the scalar-
    operand and LDS-staged kernels, the f32 per-tap kernels (general / linear-address), the pipelined 16-bit kernel, the f32
    split-product kernel and the DMA-staged kernels (3x3 with forced units per workgroup: a ragged last unit run; stride 2;
    dilated; the wide 1x1 over a flat pixel axis whose last unit is partial).  The kernels are told exactly
    fami_conv2d_wgrad_workspace bytes of workspace, inside guards."""
    types, knobs, cases, claims, query = WG_ROUTES[route]
    drive(dev, dt, 'wgrad/' + route, knobs, cases, claims, query, fwd=0, dgrad=0)


# ------------------------------------------------------------------------------------------------- one-launch backward pair
PAIR_16 = [(g3(2, 8, 72, 48, 48), 0), (g3(1, 10, 72, 48, 48), 1), (g3(3, 16, 64, 48, 48), 0), (g3(2, 16, 64, 48, 96), 0), (g3(3, 12, 9, 96, 144), 1),
           (g3(2, 24, 18, 144, 96), 1), (g3(3, 12, 9, 128, 192), 1), (g3(2, 16, 36, 256, 64), 0), (g3(1, 10, 72, 64, 64), 1),
           (g3(2, 13, 9, 96, 96), 1), (g3(1, 11, 11, 128, 64), 1)]          # (odd x odd maps whose rows still make a whole weight-gradient unit)
PAIR_32 = [(g3(2, 24, 18, 48, 48), 1), (g3(2, 3, 40, 48, 48), 1), (g3(3, 17, 5, 144, 96), 1), (g3(1, 9, 33, 48, 96), 1), (g3(2, 16, 12, 96, 96), 0),
           (g3(1, 24, 18, 48, 48), 1)]


@pytest.mark.parametrize('dt', TYPES)
def test_backward_pair_is_exact(dev, dt):
    """fami_conv2d_bwd_pair_*: input gradient (plain / with the backward-statistics epilogue, fresh / accumulating) and deferred
    weight gradient in one launch, where fami_conv2d_bwd_pair_ok* says a combined instance takes the geometry."""
    if dt == 'f32':
        knobs, cases, ok = [('lds', 7001), ('lds', 7600), ('lds', 7401)], PAIR_32, 'fami_conv2d_bwd_pair_ok_f32'
    else:
        knobs, cases, ok = [('lds', 8001), ('lds', 8501), ('lds', 8400)], PAIR_16, 'fami_conv2d_bwd_pair_ok'
    drive(dev, dt, 'backward-pair', knobs, cases, query=lambda L, g: getattr(L.cdll, ok)(*g[:5], 3, 3, 1, 1, 1) == 1, passes=_pair_passes)


# ------------------------------------------------------------------------------------------------- refusals leave no capture
def _refused(L, name, *args):
    from fami_pose_amd._lib import FamiError
    with pytest.raises(FamiError) as ei:
        L.call(name, *args)
    return str(ei.value)


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_refused_deferred_wgrad_leaves_no_reduce_capture(dev, dt):
    """A fami_conv2d_wgrad_defer_* call refused AFTER its reduce capture was installed (a workspace one byte short of a single
    [kh][kw][Ci][Co] slab: less than any route's plan needs, while one byte short of fami_conv2d_wgrad_workspace -- the largest
    of the plans -- can still satisfy the route that takes the call), then the immediate form: dW is exact, so its reduce
    was launched and not recorded into a capture nobody reads."""
    geo = g3(1, 8, 8, 16, 16)
    tune([])
    r = Runner(dev, dt, make_case(geo))
    slab = 16 * 16 * 9 * 4
    assert r.ws_bytes >= slab
    r._begin()
    dw = r.A.output((16, 16, 3, 3), torch.float32, None, 'dw')
    ws, _ = r._workspace()
    desc = (ctypes.c_long * r.L.cdll.fami_wgrad_reduce_desc_longs())()
    msg = _refused(r.L, 'fami_conv2d_wgrad_defer' + r.sfx, r.x.data_ptr(), r.dy.data_ptr(), dw.data_ptr(), ws.data_ptr(), slab - 1,
                   *r.g10, 0, desc, r.st)
    assert '(-1)' in msg and 'workspace too small' in msg, msg
    fails = r.wgrad(0) + r.wgrad(1)
    assert not fails, 'after a refused deferred call, storage %s:\n  %s' % (dt, '\n  '.join(fails))


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_refused_backward_pair_leaves_no_launch_capture(dev, dt):
    """A fami_conv2d_bwd_pair_* call refused inside its input gradient (kernel size 8) on the smallest geometry of the pair
    tables that fami_conv2d_bwd_pair_ok* takes, then the plain input gradient of that geometry under the same knobs: dx is
    exact, so the kernel was launched and not recorded into a pair capture nobody launches."""
    if dt == 'f32':
        knobs, cases, ok = [('lds', 7001), ('lds', 7600), ('lds', 7401)], PAIR_32, 'fami_conv2d_bwd_pair_ok_f32'
    else:
        knobs, cases, ok = [('lds', 8001), ('lds', 8501), ('lds', 8400)], PAIR_16, 'fami_conv2d_bwd_pair_ok'
    L = _lib()
    try:
        tune(knobs)
        taken = [g for g, _ in cases if getattr(L.cdll, ok)(*g[:5], 3, 3, 1, 1, 1) == 1]
        assert taken, 'no geometry of the pair table is combined'
        geo = min(taken, key=lambda g: g[0] * g[1] * g[2] * (g[3] + g[4]))
        r = Runner(dev, dt, make_case(geo))
        N, H, W, Ci, Co = geo[:5]
        r._begin()
        dx = r._act((N, H, W, Ci), None, 'dx')
        dw = r.A.output((Co, Ci, 3, 3), torch.float32, None, 'dw')
        ws, wsb = r._workspace()
        desc = (ctypes.c_long * L.cdll.fami_wgrad_reduce_desc_longs())()
        head = (r.x.data_ptr(), r.dy.data_ptr(), r.wp[1].data_ptr(), dx.data_ptr(), dw.data_ptr(), ws.data_ptr(), wsb)
        tail = (None, None, None, None, None, None, 0, None) if r.half else (None, None, None, None)
        msg = _refused(L, 'fami_conv2d_bwd_pair' + r.sfx, *head, N, H, W, Ci, Co, 8, 8, 1, 1, 1, 0, 0, desc, *tail, r.st)
        assert '(-2)' in msg and 'unsupported geometry' in msg, msg
        fails = r.dgrad(0, 0) + r.dgrad(0, 1)
        assert not fails, 'after a refused pair call, storage %s, geometry %s:\n  %s' % (dt, geo, '\n  '.join(fails))
    finally:
        L.cdll.fami_tune_reset()


# ------------------------------------------------------------------------------------------------- dense tier
@pytest.mark.parametrize('dt', TYPES)
def test_dense_tier_pins_the_store_conversion(dev, dt):
    """Operands in [-2, 2], K = 9 * 384 (the largest of the file), no accumulate: results of several hundred, exact in fp32
    accumulation but beyond bf16's exact integers -- the stored value must be the round-to-nearest-even conversion of the exact
    result (csrc/common.h), on the direct (split-K) kernels and on the default routes."""
    geo = (2, 6, 5, 384, 384, 3, 1, 1, 1)
    c = make_case(geo, True)
    assert c.conv.abs().max().item() > 256 and c.dgrad.abs().max().item() > 256          # (the tier leaves the exact range)
    L = _lib()
    try:
        for route, knobs in (('direct', [('lds', 0)]), ('default', [('lds', 7600), ('lds', 7401), ('lds', 8400)])):
            tune(knobs)
            r = Runner(dev, dt, c)
            fails = r.fwd(0, 0, 0, 0) + r.fwd(1, 0, 1, 0) + r.dgrad(0, 0)
            assert not fails, 'dense tier, route %s, storage %s, geometry %s:\n  %s' % (route, dt, geo, '\n  '.join(fails))
    finally:
        L.cdll.fami_tune_reset()
