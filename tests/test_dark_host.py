"""Host side of the DARK decode (loss.dark_get_final_preds, evaluate.predict / evaluate_loop(decode='dark')): the numpy
yardstick tests/_dark_ref.py against the fixture tests/golden/dark_final_preds.npz, the Gaussian taps, and the keyword
validation that happens before any device work.

The fixture holds what the reference's OWN dark_get_final_preds (datasets/process/heatmaps_process.py:84-143) returns
for seeded maps (tools/gen_dark_golden.py).  cv2 is absent where it was generated, so the reference ran with
`_dark_ref.cv2_gaussian_blur` as cv2.GaussianBlur and the oracle's `cv2_get_affine_transform` as
cv2.getAffineTransform: `taylor`, the clamp, the log, the rescale and `transform_preds` are the reference's real code,
only those two third-party calls are restatements of their documented definitions (as in g12).  The reference blurs in
float64, stores the blurred map as float32 and does the rest in float32 / float64 mixed; the float64 restatement differs
from it by 3.9e-5 image pixels on this fixture (3.7e-6 heatmap pixels), against the 1e-3 image pixels the project uses
for fp32 affine arithmetic against fp64 (g12)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _dark_ref as dr  # noqa: E402

from fami_pose_amd import evaluate as ev, loss as FL  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dark_final_preds.npz')


@pytest.mark.parametrize('fp32', [False, True])
def test_restatement_matches_the_reference_fixture(fp32):
    g = np.load(GOLD)
    assert g['hm'].shape == (2, 17, 64, 48) and g['hm'].dtype == np.float32
    assert (g['hm'][0, 0] < 0).any() and not (g['hm'][0, 0] > 0).any() and not g['hm'][0, 1].any()
    r = dr.dark_ref(g['hm'], g['center'], g['scale'], 11, fp32=fp32)
    err = np.abs(r['preds'].astype(np.float64) - g['preds']).max()
    print('restatement (fp32=%s) against the fixture: %.3e image px, %d of 34 maps refined' % (fp32, err, r['moved'].sum()))
    assert np.array_equal(r['maxvals'], g['maxvals'])
    assert r['moved'].sum() >= 17                  # the fixture does exercise the Newton step
    assert err < 1e-3
    # the maps without a positive maximum decode to heatmap (0, 0), as in get_final_preds
    for j in (0, 1):
        assert np.array_equal(r['intc'][0, j], [0, 0]) and not r['branch'][0, j]


def test_the_blur_never_sees_the_border_mode():
    """Step 2 of the reference pads by (k-1)//2 zeros, blurs and crops: the cropped part reads only the padded array, so
    the reflect-101 stand-in handed to the reference and plain zero padding agree on it."""
    rng = np.random.RandomState(3)
    for k, (H, W) in ((9, (17, 13)), (11, (24, 18)), (17, (20, 19)), (11, (8, 6))):
        hm = rng.standard_normal((H, W))
        b = (k - 1) // 2
        padded = np.zeros((H + 2 * b, W + 2 * b))
        padded[b:-b, b:-b] = hm
        a = dr.cv2_gaussian_blur(padded, (k, k), 0)[b:-b, b:-b]
        assert a.shape == (H, W) and np.abs(a - dr.blur_zero(hm, k)).max() < 1e-15


def test_taps():
    assert dr.sigma_of(11) == 2.0 and abs(dr.sigma_of(17) - 2.9) < 1e-12
    for k in (9, 11, 13, 15, 17):
        t = FL.gaussian_taps(k)
        assert t.dtype == np.float32 and t.shape == (k,)
        assert np.array_equal(t, dr.taps(k).astype(np.float32))
        assert np.array_equal(t, t[::-1])                                    # symmetric bit for bit (the kernel relies on it)
        assert abs(float(t.astype(np.float64).sum()) - 1.0) < 1e-7
        assert t.argmax() == k // 2 and (np.diff(t[:k // 2 + 1]) > 0).all()
    x = np.arange(11) - 5.0
    w = np.exp(-x * x / 8.0)                                                 # sigma(11) = 2.0
    assert np.array_equal(FL.gaussian_taps(11), (w / w.sum()).astype(np.float32))


@pytest.mark.parametrize('k', [3, 5, 7, 8, 10, 12, 19, 21, 0, -11, 11.5, True, 1])
def test_blur_kernel_is_validated(k):
    with pytest.raises(ValueError):
        FL.check_blur_kernel(k)
    with pytest.raises(ValueError):
        FL.gaussian_taps(k)


class _NoDevice:
    """a model / batch source that fails the test when touched: the keywords are checked before any device work"""

    def __call__(self, *a, **k):
        raise AssertionError('the model was called')

    def parameters(self):
        raise AssertionError('the model was touched')

    def eval(self):
        raise AssertionError('the model was touched')

    def __iter__(self):
        raise AssertionError('the batches were read')

    training = False


@pytest.mark.parametrize('kw', [{'decode': 'DARK'}, {'decode': 'unbiased'}, {'decode': None}, {'decode': ''},
                                {'decode': 'dark', 'blur_kernel': 10}, {'decode': 'dark', 'blur_kernel': 7},
                                {'decode': 'dark', 'blur_kernel': 19}, {'decode': 'dark', 'blur_kernel': 3}])
def test_front_door_keywords_are_checked_before_any_device_work(kw):
    m = _NoDevice()
    with pytest.raises(ValueError):
        ev.predict(m, None, None, None, None, **kw)
    with pytest.raises(ValueError):
        ev.predict(m, None, None, None, None, flip=True, **kw)
    with pytest.raises(ValueError):
        ev.evaluate_loop(m, _NoDevice(), 4, **kw)


def test_blur_kernel_is_ignored_by_the_standard_decode():
    """blur_kernel belongs to decode='dark' as shift_heatmap belongs to flip=True: with the default decode it is not read."""
    assert ev._decoder('standard', 4) is FL.get_final_preds


def test_lds_query_and_device_only():
    """The size rule of the kernel is host arithmetic of the library: callable without a GPU."""
    from fami_pose_amd._lib import lib
    c = lib().cdll
    limit = c.fami_dark_preds_lds_limit()
    assert limit <= 160 * 1024
    for k in (9, 11, 13, 15, 17):
        for H, W in ((64, 48), (96, 72), (128, 96)):                          # the heatmap sizes of BASELINE.json
            need = c.fami_dark_preds_lds_bytes(H, W, k)
            assert need == 4 * (H * (W + k - 1) + (H + k - 1) * W) and need <= limit, (H, W, k)
    assert c.fami_dark_preds_lds_bytes(256, 192, 11) > limit
    for H, W, k in ((0, 4, 11), (4, -1, 11), (8, 8, 7), (8, 8, 12), (8, 8, 19)):
        assert c.fami_dark_preds_lds_bytes(H, W, k) == -1
    assert c.fami_dark_preds_f32(None, None, None, None, 11, None, None, 1, 1, 8, 8, None) == -1
    import torch
    with pytest.raises(RuntimeError):
        FL.dark_get_final_preds(torch.zeros(1, 1, 8, 8), np.zeros((1, 2)), np.ones((1, 2)))     # device only, like loss.py
