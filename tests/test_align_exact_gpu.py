"""Every exported compute entry point of csrc/align.hip held to EXACT results, with guard zones around every output and NaN
around every operand: fami_shift_bilinear_{fwd,bwd}_*, fami_dcn_fwd_* / _fwd_om_*, fami_dcn_bwd_* / _bwd_om_*,
fami_dcn_bwd_det_* / _bwd_det_om_* in f32, bf16 and f16, the three weight packers (through the passes that read their images)
and fami_dcn_col_dw_unpermute_f32 (through the weight gradient formed from the kernel's own `col`).

The operands (tests/_align_exact.py) make every result independent of the order of any sum -- small integers, integer and
half-integer offsets, power-of-two masks -- and the conditions that make this true are asserted on the fp64 reference before any
launch.  Every comparison is torch.equal against that reference (rounded once where the output is stored in a 16-bit type);
there is no tolerance in this module.  On purpose in the data: offsets beyond the LDS regions' reach of 3 pixels (global-atomic
path), offsets that leave the map (zeroed corners), |mask| = 16 (above the fixed-point bound), a null mask pointer, and acc = 1
on pre-filled outputs.

Shapes: B = 2, 9 x 10 maps (partial 8 x 8 tiles, P no multiple of 16), 3 x 3 taps.
  (C, G, Co) = (8, 2, 16)   C == 4G: the register-fed backward is eligible.  The LDS-window forward is not (G*K = 18 is no multiple
                            of 4: routes 2 and 2 + 256+2 run the direct kernel here), nor is the general backward kernel (no
                            16-aligned chunk of groups), so the routes that force the general kernel and the deterministic entry
                            points run on the other two
  (16, 2, 20)               8 channels per group, Co no multiple of 16: general kernels only, with their channel-tail loads
  (16, 4, 16)               C == 4G and G*K = 36: the LDS-window forward (routes 2, 2 + 256+2) and both backward kernels
with pad = dil = 3 and pad = dil = 1, one stride-2 case on the general kernels, and pad = dil = 7 in 16-bit storage on the
register-fed backward: there the f32 plan no longer fits its LDS while the 16-bit plan does, and the 16-bit weight image still lies
behind an f32 image packed for the head's dilation (test_dcn_backward_register_fed_beyond_the_f32_plan).  Routes through the fami_dcn_tune codes of
include/fami.h, reset in a `finally`."""
import pytest
import torch

from _align_exact import DcnRunner, make_case, make_shift_case, run_shift

pytestmark = pytest.mark.gpu

TYPES = ['f32', 'bf16', 'f16']
FWD_ROUTES = [(0,), (1,), (2,), (16 + 2,), (2, 256 + 2)]
BWD_GENERAL = [(2048,), (2048, 512), (2048, 514)]


def geo(C, G, Co, stride=1, dil=3):
    return (2, 9, 10, C, G, Co, 3, stride, dil, dil)


REGISTER_FED = [geo(8, 2, 16, dil=3), geo(8, 2, 16, dil=1)]
GENERAL = [geo(16, 2, 20, dil=3), geo(16, 2, 20, dil=1), geo(16, 2, 20, stride=2, dil=1), geo(16, 4, 16, dil=3)]


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def window_eligible(g, esz):
    """dcn_win_plan's conditions on the geometry (csrc/align.hip); the window itself is a few KB at these sizes"""
    B, H, W, C, G, Co, k, stride, pad, dil = g
    return stride == 1 and C == 4 * G and (C * esz) % 16 == 0 and (G * k * k) % 4 == 0 and Co <= 64


def test_one_geometry_reaches_the_window_kernel():
    assert [g for g in REGISTER_FED + GENERAL if window_eligible(g, 4) and window_eligible(g, 2)] == [geo(16, 4, 16, dil=3)]


def runner(dev, dt, g):
    return DcnRunner(dev, dt, make_case(g))


def ids(gs):
    return ['C%dG%dCo%ds%dd%d' % (g[3], g[4], g[5], g[7], g[9]) for g in gs]


@pytest.mark.parametrize('dt', TYPES)
def test_shift_forward_and_backward(dev, dt):
    fails = run_shift(dev, dt, make_shift_case((2, 9, 10, 8)))
    assert not fails, fails


@pytest.mark.parametrize('dt', TYPES)
@pytest.mark.parametrize('g', REGISTER_FED + GENERAL, ids=ids(REGISTER_FED + GENERAL))
def test_dcn_forward_on_every_route(dev, dt, g):
    r = runner(dev, dt, g)
    fails = []
    for codes in [()] + FWD_ROUTES:
        fails += r.fwd(codes)
        fails += r.fwd(codes, om=True)
        fails += r.fwd(codes, masked=False, bias=False)
    assert not fails, fails


@pytest.mark.parametrize('dt', TYPES)
@pytest.mark.parametrize('g', REGISTER_FED, ids=ids(REGISTER_FED))
def test_dcn_backward_register_fed(dev, dt, g):
    r = runner(dev, dt, g)
    C, G, Co = g[3], g[4], g[5]
    assert r.L.cdll.fami_dcn_bwd_col_permuted(C, Co, G, 3, 3, 1, g[9], r.esz, 0) == 1          # the default route is the register-fed kernel here
    fails = []
    for codes in [(), (8192,)]:
        for acc in (0, 1):
            fails += r.bwd(codes, acc=acc)
            fails += r.bwd(codes, om=True, acc=acc)
        fails += r.bwd(codes, masked=False)
        fails += r.bwd(codes, want_gx=False, want_col=False)
    assert not fails, fails


@pytest.mark.parametrize('dt', TYPES)
@pytest.mark.parametrize('g', GENERAL, ids=ids(GENERAL))
def test_dcn_backward_general(dev, dt, g):
    r = runner(dev, dt, g)
    fails = []
    for codes in [()] + BWD_GENERAL:
        for acc in (0, 1):
            fails += r.bwd(codes, acc=acc)
        fails += r.bwd(codes, om=True, acc=1)
        fails += r.bwd(codes, masked=False)
    assert r.L.cdll.fami_dcn_bwd_col_permuted(g[3], g[5], g[4], 3, 3, g[7], g[9], r.esz, 0) == (1 if (g[3], g[4], g[5]) == (16, 4, 16) else 0)
    assert not fails, fails


@pytest.mark.parametrize('dt', TYPES)
@pytest.mark.parametrize('g', GENERAL, ids=ids(GENERAL))
def test_dcn_backward_deterministic(dev, dt, g):
    r = runner(dev, dt, g)
    fails = []
    for om in (False, True):
        for acc, acc_x in ((0, 0), (1, 1)):
            fails += r.bwd((), om=om, acc=acc, det=True, acc_x=acc_x)
    fails += r.bwd((), masked=False, det=True)
    fails += r.bwd((), det=True, want_gx=False)          # no input gradient: `col` keeps the deterministic layout
    assert not fails, fails


@pytest.mark.parametrize('dt', ['bf16', 'f16'])
def test_dcn_backward_register_fed_beyond_the_f32_plan(dev, dt):
    """pad = dil = 7 on (8, 2, 16): the register-fed kernel takes the 16-bit launch, the f32 plan does not fit.  The 16-bit weight image
    lies behind the f32 image of the HEAD's plan (dilation 3), which the packer wrote; a launcher that skips the f32 image by the plan
    at the actual dilation (the library before the layout structs did) contracts with the wrong weights and fails this case."""
    g = geo(8, 2, 16, dil=7)
    r = runner(dev, dt, g)
    cd = r.L.cdll
    assert cd.fami_dcn_bwd_col_permuted(8, 16, 2, 3, 3, 1, 7, 2, 0) == 1 and cd.fami_dcn_bwd_col_permuted(8, 16, 2, 3, 3, 1, 7, 4, 0) == 0
    fails = r.bwd(()) + r.bwd((), om=True, acc=1)
    assert not fails, fails
