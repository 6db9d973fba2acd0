"""Degradation of the batched clip crop without a GPU: the numpy restatement of include/fami.h's stages
(tests/_degrade_ref.py) against oracle.ops.cv2_warp_affine_u8 and hand-derived numbers; draw_degradation's determinism,
ranges, modes, untouched global generators and refusals; ClipBatcher's checks with the `degrade` field; and the record
layout against the library's size query."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _degrade_ref as R  # noqa: E402

import fami_pose_amd as fp  # noqa: E402
from fami_pose_amd import data as D  # noqa: E402

SIZE = (40, 52)
SRC = [(60, 90), (180, 260), (97, 131)]               # the three clips of test_prepare_batch_gpu.py
ROT = [0.0, 31.0, -44.0]
FLIP = [False, True, False]
CENTER = [(50.5, 28.25), (140.5, 80.25), (20.0, 70.0)]
SCALE = [(0.45, 0.6), (0.9, 1.2), (0.6, 0.8)]
IDENTITY = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])


def _plain(img, rec, flip=False):
    """the restatement on an identity crop with mean 0 and std 1: the output is N(value of stage 3)"""
    return R.degrade_frame(img, IDENTITY, (img.shape[1], img.shape[0]), flip, False, rec, (0, 0, 0), (1, 1, 1))


def N(v):
    """stage 4 with mean 0 and std 1: v / 255 in float32"""
    return np.asarray(v, np.float32) / np.float32(255)


@pytest.mark.parametrize('bgr', [False, True])
def test_every_flag_off_is_cv2_warp_affine_and_normalize(bgr):
    from oracle import ops as O
    rng = np.random.RandomState(21)
    border = False
    for k in range(3):
        Hs, Ws = SRC[k]
        img = (rng.rand(Hs, Ws, 3) * 255).astype(np.uint8)
        c = np.array(CENTER[k], np.float64)
        if FLIP[k]:
            c[0] = Ws - c[0] - 1
        trans = O.dark_get_affine_transform(c, np.array(SCALE[k]), ROT[k], SIZE)
        src = np.ascontiguousarray(img[:, :, ::-1]) if bgr else img
        want = O.to_tensor_normalize(O.cv2_warp_affine_u8(src, trans, SIZE, flip=FLIP[k]), D.MEAN, D.STD).numpy()
        mi = O.cv2_invert_affine(trans)
        got = R.degrade_frame(img, mi, SIZE, FLIP[k], bgr, {'flags': 0}, D.MEAN, D.STD)
        assert got.dtype == np.float32 and np.array_equal(got, want), k
        # taps = 1 with zero steps is the plain sample
        one = R.degrade_frame(img, mi, SIZE, FLIP[k], bgr, {'flags': R.BLUR, 'taps': 1, 'step_x': 0, 'step_y': 0}, D.MEAN, D.STD)
        assert np.array_equal(one, want), k
        border = border or bool((got[0] == np.float32(-D.MEAN[0] / D.STD[0])).any())
    assert border                                                 # the zero border occurs


def test_colour_by_hand():
    img = np.full((4, 5, 3), 100, np.uint8)
    # 100 * 1.5 - 10 = 140 in every channel; grey, so the saturation step returns it
    out = _plain(img, {'flags': R.COLOUR, 'alpha': 1.5, 'delta': -10.0, 'sat': 1.0})
    assert np.array_equal(out, np.full((3, 4, 5), N(140)))
    # sat on a grey image returns the image.  g = 0.299f v + 0.587f v + 0.114f v is v or an ulp beside it, so v - g is exact;
    # with sat = 1 so is sat * (v - g), and g + (v - g) = v bit for bit, for every byte v.  With another sat the product
    # is rounded once more, at a thousandth of an ulp of v: the result stays within one ulp of v.
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2)
    out = _plain(ramp, {'flags': R.COLOUR, 'alpha': 1.0, 'delta': 0.0, 'sat': 1.0})
    assert np.array_equal(out, _plain(ramp, {'flags': 0}))
    for sat in (0.0, 0.5, 1.7):
        out = _plain(ramp, {'flags': R.COLOUR, 'alpha': 1.0, 'delta': 0.0, 'sat': sat}) * np.float32(255)
        assert (np.abs(out - np.arange(256)) <= np.maximum(np.arange(256), 1) * 2.0 ** -22).all(), sat
    # sat = 0 gives g in all channels: (0.299 * 200 + 0.587 * 100) + 0.114 * 50 in float32, operation by operation
    rgb = np.zeros((2, 2, 3), np.uint8)
    rgb[...] = (200, 100, 50)
    f = np.float32
    g = f(f(f(0.299) * f(200)) + f(f(0.587) * f(100))) + f(f(0.114) * f(50))
    assert abs(float(g) - 124.2) < 1e-4
    out = _plain(rgb, {'flags': R.COLOUR, 'alpha': 1.0, 'delta': 0.0, 'sat': 0.0})
    assert np.array_equal(out, np.full((3, 2, 2), N(g)))
    # the clamp: 200 * 2 = 400 -> 255, 50 * 2 - 150 = -50 -> 0
    out = _plain(rgb, {'flags': R.COLOUR, 'alpha': 2.0, 'delta': -150.0, 'sat': 1.0}) * f(255)
    assert abs(out[0, 0, 0] - 250) < 1e-4 and out[2, 0, 0] == 0 and _plain(
        rgb, {'flags': R.COLOUR, 'alpha': 2.0, 'delta': 0.0, 'sat': 1.0})[0, 0, 0] == 1.0
    # a flag that is off skips the stage, whatever the parameters say
    assert np.array_equal(_plain(rgb, {'flags': 0, 'alpha': 3.0, 'delta': 9.0, 'sat': 0.0}), _plain(rgb, {'flags': 0}))


def test_blur_by_hand():
    # a vertical step edge 0 | 255 between columns 3 and 4; three taps one source pixel apart, horizontally:
    # column 2 sees (0, 0, 0) -> 0; column 3 (0, 0, 255) -> (2 * 255 + 3) / 6 = 85; column 4 (0, 255, 255) ->
    # (2 * 510 + 3) / 6 = 170; column 5 (255, 255, 255) -> (2 * 765 + 3) / 6 = 255
    img = np.zeros((6, 8, 3), np.uint8)
    img[:, 4:] = 255
    rec = {'flags': R.BLUR, 'taps': 3, 'step_x': 1024, 'step_y': 0}
    out = _plain(img, rec)
    assert out.shape == (3, 6, 8)
    assert np.array_equal(out[:, 2, 2:6], np.tile(N([0, 85, 170, 255]), (3, 1)))
    # the taps leave the image at its right edge and read the zero border: column 7 sees (255, 255, 0) -> 170
    assert np.array_equal(out[:, 2, 6:], np.tile(N([255, 170]), (3, 1)))
    # mirrored columns: the edge runs the other way
    flipped = _plain(img, rec, flip=True)
    assert np.array_equal(flipped, out[:, :, ::-1])
    # vertical steps on the same image change nothing away from the border rows
    v = _plain(img, {'flags': R.BLUR, 'taps': 3, 'step_x': 0, 'step_y': 1024})
    assert np.array_equal(v[:, 1:5], _plain(img, {'flags': 0})[:, 1:5]) and np.array_equal(v[:, 0, 4:], np.full((3, 4), N(170)))


def test_lowbias32_by_hand():
    # v = 1:        v ^= v >> 16 -> 0x00000001;  * 0x7feb352d -> 0x7feb352d;  >> 15 is 0xffd6, xor -> 0x7febcafb;
    #               * 0x846ca68b = 0x422bdf5b6889f849 -> low word 0x6889f849;  >> 16 is 0x6889, xor -> 0x688990c0
    # v = 0x10000:  v ^= v >> 16 -> 0x00010001;  * 0x7feb352d = 0x7feb352d + 0x352d0000 (mod 2^32) = 0xb518352d;
    #               >> 15 is 0x16a30, xor -> 0xb5195f1d;  * 0x846ca68b -> low word 0xdcaf72bf;  >> 16 is 0xdcaf,
    #               xor -> 0xdcafae10
    assert int(R.lowbias32(1)) == 0x688990c0
    assert int(R.lowbias32(0x10000)) == 0xdcafae10
    assert int(R.lowbias32(0)) == 0
    got = R.lowbias32(np.array([1, 0x10000], np.uint64))
    assert got.tolist() == [0x688990c0, 0xdcafae10]


def test_occluders_by_hand():
    img = np.full((6, 8, 3), 10, np.uint8)
    rects = [(1, 1, 5, 4, 0, (20, 30, 40)), (3, 2, 7, 6, 0, (50, 60, 70)), (2, 2, 2, 5, 0, (99, 99, 99)),   # the third is empty
             (-4, -4, 1, 1, 0, (1, 2, 3))]                                                           # hangs over a corner
    out = _plain(img, {'flags': R.OCCLUDE, 'rects': rects, 'seed': 0})
    want = np.full((3, 6, 8), 10, np.float32)
    want[:, 1:4, 1:5] = np.float32([20, 30, 40])[:, None, None]
    want[:, 2:6, 3:7] = np.float32([50, 60, 70])[:, None, None]           # the later rectangle wins the overlap
    want[:, 0, 0] = (1, 2, 3)
    assert np.array_equal(out, N(want))
    assert out[0, 2, 3] == N(50) and out[0, 1, 3] == N(20) and out[0, 2, 2] == N(20)
    # in the other order the first one wins it back
    back = _plain(img, {'flags': R.OCCLUDE, 'rects': [rects[1], rects[0]], 'seed': 0})
    assert back[0, 2, 3] == N(20) and back[0, 5, 6] == N(50)
    # noise: pixel (x, y) = (1, 0) of channel 0 in an 8-wide crop is index 1; seed 0 -> lowbias32(1) >> 24 = 0x68;
    # with seed 0x10001 the index 1 becomes 0x10000 -> 0xdc
    n0 = _plain(img, {'flags': R.OCCLUDE, 'rects': [(0, 0, 8, 6, 1, (0, 0, 0))], 'seed': 0})
    n1 = _plain(img, {'flags': R.OCCLUDE, 'rects': [(0, 0, 8, 6, 1, (0, 0, 0))], 'seed': 0x10001})
    assert n0[0, 0, 1] == N(0x68) and n1[0, 0, 1] == N(0xdc) and n0[0, 0, 0] == 0
    assert n0[1, 2, 3] == N(int(R.lowbias32((1 * 6 + 2) * 8 + 3)) >> 24)
    assert len(np.unique(n0)) > 40                                        # it is noise
    # a covered pixel takes the fill in place of the colour stage's result
    both = _plain(img, {'flags': R.OCCLUDE | R.COLOUR, 'alpha': 2.0, 'delta': 0.0, 'sat': 1.0, 'rects': rects[:1], 'seed': 0})
    assert both[0, 1, 1] == N(20) and both[0, 0, 1] == N(20) and both[1, 5, 7] == N(20) and both[1, 1, 1] == N(30)


# ---- draw_degradation ---------------------------------------------------------------------------------------------------
ALWAYS = {'photo_prob': 1.0, 'occlude_prob': 1.0, 'blur_prob_key': 1.0, 'blur_prob_sup': 1.0}


@pytest.mark.parametrize('make', [np.random.RandomState, np.random.default_rng], ids=['RandomState', 'Generator'])
def test_draw_is_deterministic_and_leaves_the_global_generators_alone(make):
    np_state, py_state = np.random.get_state(), random.getstate()        # whatever they are: this test sets neither
    a = D.draw_degradation(3, SIZE, dict(ALWAYS, occlude_frames='independent', occlude_fill='noise'), make(11))
    b = D.draw_degradation(3, SIZE, dict(ALWAYS, occlude_frames='independent', occlude_fill='noise'), make(11))
    c = D.draw_degradation(3, SIZE, dict(ALWAYS, occlude_frames='independent', occlude_fill='noise'), make(12))
    assert a == b and a != c
    assert fp.draw_degradation is D.draw_degradation
    s = np.random.get_state()
    assert s[0] == np_state[0] and np.array_equal(s[1], np_state[1]) and s[2:] == np_state[2:]
    assert random.getstate() == py_state
    # the documented consumption order, replayed: colour u + 3, occluder u, count + 4 per rectangle, seed, blur per frame
    rng, ref = make(3), make(3)
    d = D.draw_degradation(2, SIZE, dict(ALWAYS, occlude_count=(2, 2)), rng)
    u = lambda lo=0.0, hi=1.0: float(ref.uniform(lo, hi))
    u()
    assert d['colour'] == (u(0.7, 1.3), u(-25.0, 25.0), u(0.5, 1.5))
    u(), u(2, 3)
    for _ in range(2 * 4):
        u()
    assert d['seed'] == int(u(0.0, 4294967296.0))
    for f in range(2):
        u()
        length, angle = u(3.0, 15.0), u(0.0, 180.0)
        assert d['blur'][f] == (D.blur_taps(length), length, angle)
    assert float(rng.uniform(0, 1)) == float(ref.uniform(0, 1))          # both generators stand at the same place
    # nothing drawn: four u and the seed
    rng, ref = make(4), make(4)
    d = D.draw_degradation(2, SIZE, {k: 0.0 for k in ALWAYS}, rng)
    assert d['colour'] is None and d['blur'] == [None, None] and d['occluders'] == [[], []]
    for _ in range(5):
        ref.uniform(0.0, 1.0)
    assert float(rng.uniform(0, 1)) == float(ref.uniform(0, 1))


def test_draw_ranges_and_modes():
    W, H = SIZE
    rng = np.random.RandomState(7)
    seen_taps, seen_over = set(), False
    for _ in range(200):
        d = D.draw_degradation(3, SIZE, dict(ALWAYS, occlude_frames='all', blur_length=(1.0, 40.0)), rng)
        alpha, delta, sat = d['colour']
        assert 0.7 <= alpha <= 1.3 and -25 <= delta <= 25 and 0.5 <= sat <= 1.5
        assert 1 <= len(d['occluders'][0]) <= 2 and d['occluders'][0] == d['occluders'][1] == d['occluders'][2]
        for x0, y0, x1, y1, fill in d['occluders'][0]:
            assert fill == (124, 116, 104) and x1 > x0 and y1 > y0
            assert 0.02 * W * H * 0.6 <= (x1 - x0) * (y1 - y0) <= 0.15 * W * H * 1.4          # rounding of small sides
            assert 0.5 / 1.5 <= (x1 - x0) / (y1 - y0) <= 2.0 * 1.5
            assert -(x1 - x0) <= x0 <= W and -(y1 - y0) <= y0 <= H
            seen_over = seen_over or x0 < 0 or y0 < 0 or x1 > W or y1 > H
        for taps, length, angle in d['blur']:
            assert 1.0 <= length <= 40.0 and 0 <= angle < 180 and taps % 2 == 1 and taps <= min(15, length) < taps + 2
            seen_taps.add(taps)
        assert 0 <= d['seed'] < 2 ** 32
        D.check_degradation(d, 3)
    assert seen_over and seen_taps == {1, 3, 5, 7, 9, 11, 13, 15}
    assert [D.blur_taps(v) for v in (1.0, 2.9, 3.0, 4.99, 5.0, 14.9, 15.0, 99.0)] == [1, 1, 3, 3, 5, 13, 15, 15]
    key = D.draw_degradation(3, SIZE, dict(ALWAYS, occlude_frames='key'), np.random.RandomState(8))
    assert key['occluders'][0] and key['occluders'][1] == key['occluders'][2] == []
    ind = D.draw_degradation(3, SIZE, dict(ALWAYS, occlude_frames='independent', occlude_fill='noise'), np.random.RandomState(8))
    assert all(ind['occluders']) and ind['occluders'][0] != ind['occluders'][1] and ind['occluders'][0][0][4] == 'noise'
    # probabilities: key and supporting frames have their own
    sup_only = [D.draw_degradation(3, SIZE, {'blur_prob_key': 0.0, 'blur_prob_sup': 1.0}, rng)['blur'] for _ in range(5)]
    assert all(b[0] is None and b[1] is not None and b[2] is not None for b in sup_only)
    # colour is one draw per clip; defaults come from DEGRADE_DEFAULTS and None means the defaults
    assert D.draw_degradation(3, SIZE, None, np.random.RandomState(9)) == D.draw_degradation(3, SIZE, {}, np.random.RandomState(9))


def test_draw_refusals():
    rng = np.random.RandomState(0)
    bad = [{'photo_prob': 1.5}, {'occlude_prob': -0.1}, {'blur_prob_key': float('nan')}, {'blur_prob_sup': 2},
           {'alpha_range': (0.5, float('inf'))}, {'alpha_range': (1.2, 0.8)}, {'delta_range': (-300, 0)},
           {'sat_range': (float('nan'), 1)}, {'occlude_count': (1, 5)}, {'occlude_count': (1.5, 2)},
           {'occlude_area': (0.1, 1.5)}, {'occlude_aspect': (0, 2)}, {'blur_length': (0.5, 3)}, {'blur_length': (3, 5000)},
           {'occlude_frames': 'some'}, {'occlude_fill': 'black'}, {'no_such_option': 1}]
    for o in bad:
        with pytest.raises(ValueError):
            D.draw_degradation(3, SIZE, o, rng)
    with pytest.raises(ValueError):
        D.draw_degradation(0, SIZE, None, rng)
    # the step bound, checked at the draw when the transform is known: a crop of a 10^6-pixel-wide box
    trans = D.dark_get_affine_transform(np.array([0.0, 0.0]), np.array([2e6, 2e6]), 0.0, SIZE)
    with pytest.raises(ValueError, match='2\\^24'):
        D.draw_degradation(3, SIZE, dict(ALWAYS, blur_length=(15.0, 15.0)), rng, trans=trans)
    ok = D.dark_get_affine_transform(np.array([50.0, 40.0]), np.array([0.5, 0.6]), 20.0, SIZE)
    D.draw_degradation(3, SIZE, dict(ALWAYS, blur_length=(15.0, 15.0)), rng, trans=ok)


GOOD = {'colour': (1.1, 5.0, 0.9), 'blur': [(3, 3.0, 10.0), None, (15, 30.0, 90.0)],
        'occluders': [[(1, 2, 9, 8, (1, 2, 3)), (0, 0, 4, 4, 'noise')], [], [(-5, -5, 100, 100, 'noise')]], 'seed': 77}


def _bad_dicts():
    r = (0, 0, 4, 4, (1, 2, 3))
    return {
        'even taps': dict(GOOD, blur=[(4, 4.0, 0.0), None, None]),
        'taps above 15': dict(GOOD, blur=[(17, 20.0, 0.0), None, None]),
        'taps zero': dict(GOOD, blur=[(0, 1.0, 0.0), None, None]),
        'non-integer taps': dict(GOOD, blur=[(3.5, 4.0, 0.0), None, None]),
        'length nan': dict(GOOD, blur=[(3, float('nan'), 0.0), None, None]),
        'length zero': dict(GOOD, blur=[(3, 0.0, 0.0), None, None]),
        'angle inf': dict(GOOD, blur=[(3, 3.0, float('inf')), None, None]),
        'blur count': dict(GOOD, blur=[None, None]),
        'five rectangles': dict(GOOD, occluders=[[r] * 5, [], []]),
        'occluder count': dict(GOOD, occluders=[[r]]),
        'fractional rectangle': dict(GOOD, occluders=[[(0.5, 0, 4, 4, (1, 2, 3))], [], []]),
        'huge rectangle': dict(GOOD, occluders=[[(0, 0, 1 << 31, 4, (1, 2, 3))], [], []]),
        'nan rectangle': dict(GOOD, occluders=[[(0, float('nan'), 4, 4, (1, 2, 3))], [], []]),
        'fill byte': dict(GOOD, occluders=[[(0, 0, 4, 4, (1, 2, 300))], [], []]),
        'fill name': dict(GOOD, occluders=[[(0, 0, 4, 4, 'mean')], [], []]),
        'alpha nan': dict(GOOD, colour=(float('nan'), 0.0, 1.0)),
        'alpha range': dict(GOOD, colour=(9.0, 0.0, 1.0)),
        'delta inf': dict(GOOD, colour=(1.0, float('inf'), 1.0)),
        'sat negative': dict(GOOD, colour=(1.0, 0.0, -0.5)),
        'seed': dict(GOOD, seed=1 << 32),
        'unknown key': dict(GOOD, hue=3),
        'not a dict': [1, 2, 3],
    }


@pytest.mark.parametrize('name', list(_bad_dicts()))
def test_check_degradation_refusals(name):
    D.check_degradation(GOOD, 3)
    with pytest.raises(ValueError):
        D.check_degradation(_bad_dicts()[name], 3)


def test_records_and_blur_steps():
    mi = np.array([[2.0, 0.0, 5.0], [0.0, 0.5, -3.0]])
    # 3 taps over 3 crop pixels along x: one crop pixel apart = 2 source pixels = 2048 units; along y: 0.5 -> 512
    assert D.blur_steps(3, 3.0, 0.0, mi) == (2048, 0)
    assert D.blur_steps(3, 3.0, 90.0, mi) == (0, 512)
    assert D.blur_steps(15, 30.0, 0.0, mi) == (4096, 0)
    rot = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0]])               # crop x runs along source y
    assert D.blur_steps(5, 5.0, 0.0, rot) == (0, 1024)
    with pytest.raises(ValueError):
        D.blur_steps(15, 15.0, 0.0, np.array([[2400.0, 0, 0], [0, 1.0, 0]]))     # 7 * 2400 * 1024 >= 2^24
    D.blur_steps(15, 15.0, 0.0, np.array([[2300.0, 0, 0], [0, 1.0, 0]]))
    rec = D.degrade_records(GOOD, 3, mi)
    assert rec.dtype.itemsize == 128 and rec.shape == (3,)
    assert rec['flags'].tolist() == [7, 2, 7] and rec['taps'].tolist() == [3, 0, 15]
    assert (rec['step_x'][0], rec['step_y'][0]) == D.blur_steps(3, 3.0, 10.0, mi) and rec['step_y'][2] == 1024
    assert rec['alpha'][1] == np.float32(1.1) and rec['n_rect'].tolist() == [2, 0, 1] and rec['seed'][0] == 77
    r00 = rec['rect'][0][0]
    assert [int(r00[k]) for k in ('x0', 'y0', 'x1', 'y1', 'mode')] == [1, 2, 9, 8, 0] and r00['fill'].tolist() == [1, 2, 3]
    assert rec['rect'][0][1]['mode'] == 1
    assert rec['rect'][2][0]['x1'] == 100 and not rec['reserved'].any()
    off = D.degrade_records(None, 3, mi)
    assert off.tobytes() == bytes(3 * 128)
    # a stage with nothing to do keeps its flag off
    assert D.degrade_records({'occluders': [[], [], []]}, 3, mi)['flags'].tolist() == [0, 0, 0]
    # little-endian layout of the rectangle's last word, as the kernel reads it: fill[0] lowest, mode highest
    assert rec['rect'][0][0].tobytes()[16:] == bytes([1, 2, 3, 0]) and D._DEGRADE_REC.fields['rect'][1] == 48


def _clip(frames, degrade):
    return {'frames': frames, 'joints': np.zeros((17, 3), np.float32), 'joints_vis': np.ones((17, 3), np.float32),
            'center': np.array([30.0, 20.0]), 'scale': np.array([0.3, 0.4]), 'rot': 0.0, 'flip': False, 'degrade': degrade}


def test_clip_batcher_checks_the_field_before_any_device_work(monkeypatch):
    """Counts first (frames, then the degradation dict), then kinds and shapes, then placement; none of it allocates or
    calls an entry point."""
    from fami_pose_amd import _lib
    b = D.ClipBatcher(2, 3, SIZE)
    called = []
    monkeypatch.setattr(_lib._Lib, 'call', lambda self, name, *a: called.append(name))
    monkeypatch.setattr(D.ClipBatcher, '_buffers', lambda self: called.append('_buffers'))
    f = torch.zeros(60, 90, 3, dtype=torch.uint8)
    bad = _bad_dicts()['even taps']
    with pytest.raises(ValueError, match='frames'):               # the frame count comes before the field
        b.prepare([_clip([f, f], bad)])
    with pytest.raises(ValueError, match='taps'):                 # ... the field before kinds, shapes and placement
        b.prepare([_clip([f, f, f.float()], bad)])
    with pytest.raises(ValueError, match='taps'):
        b.prepare([_clip([f, f, f], bad)])
    with pytest.raises(ValueError, match='rectangles'):
        b.prepare([_clip([f, f, f], _bad_dicts()['five rectangles']), _clip([f, f, f], None)])
    with pytest.raises(RuntimeError, match='CUDA'):               # a good field: the placement refusal as before
        b.prepare([_clip([f, f, f], GOOD)])
    with pytest.raises(RuntimeError, match='CUDA'):
        b.prepare([_clip([f, f, f], None)])
    assert called == []


def test_record_size_agrees_with_the_library():
    from fami_pose_amd import _lib
    from fami_pose_amd._lib import lib
    protos = _lib.parse_header()
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('fami_warp_degrade_batch_u8', 'fami_degrade_table_bytes'):
        assert name in protos and hasattr(cdll, name), name
    assert len(protos['fami_warp_degrade_batch_u8'][1]) == 16
    L = lib()
    assert D._DEGRADE_REC.itemsize == 128 and D._DEGRADE_RECT.itemsize == 20
    assert L.cdll.fami_degrade_table_bytes(4, 5) == 4 * 5 * D._DEGRADE_REC.itemsize
    assert L.cdll.fami_degrade_table_bytes(0, 5) == -1 and L.cdll.fami_degrade_table_bytes(4, 0) == -1
    b = D.ClipBatcher(4, 5, SIZE)
    assert b._degrade_bytes == 4 * 5 * 128 and b._bufs is None              # nothing allocated at construction
    # argument checks: refused without a launch
    one, odd = ctypes.c_void_p(64), ctypes.c_void_p(68)
    ok = (1, 1, 8, 8, 0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, None)
    bad = [
        (None, one, one, one) + ok,                                             # null table
        (one, None, one, one) + ok,                                             # null degrade
        (one, odd, one, one) + ok,                                              # misaligned degrade
        (one, one, None, one) + ok,                                             # null key
        (one, one, one, None, 1, 2) + ok[2:],                                   # null sup with F = 2
        (one, one, one, one, 0) + ok[1:],                                       # B = 0
        (one, one, one, one, 1, 0) + ok[2:],                                    # F = 0
        (one, one, one, one, 1, 1, 1 << 16, 1 << 15) + ok[4:],                  # Hd * Wd = 2^31
        (one, one, one, one, 1, 1, 8, 8, 0, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0, None),  # zero std
    ]
    for args in bad:
        assert L.cdll.fami_warp_degrade_batch_u8(*args) == -1, args
        assert b'fami_warp_degrade_batch_u8' in L.cdll.fami_last_error()
