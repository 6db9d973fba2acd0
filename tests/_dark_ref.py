"""numpy restatement of the reference's dark_get_final_preds (datasets/process/heatmaps_process.py:84-143) for any odd blur
kernel size -- the yardstick of tests/test_dark_host.py and tests/test_dark_gpu.py, and the source of the one stand-in
(`cv2_gaussian_blur`) that tools/gen_dark_golden.py hands to the reference's own code.

    1. get_max_preds on the unblurred fp32 map: flat argmax, first maximum on ties, (x, y) zeroed where the maximum <= 0
    2. gaussian_blur: zero-pad by (k-1)//2, cv2.GaussianBlur(dr, (k, k), 0), crop, rescale by origin_max / max(blurred).
       For sigmaX = 0 OpenCV takes sigma = 0.3 ((k-1) 0.5 - 1) + 0.8 and taps exp(-x^2 / (2 sigma^2)) normalised to sum 1
       (k >= 9: below that it uses fixed tables); the filter is separable, rows first.  The cropped outputs read only inside
       the padded array, so OpenCV's reflect-101 border never reaches them (`cv2_gaussian_blur` keeps that border all the
       same; tests/test_dark_host.py checks that it and plain zero padding give one cropped result).
    3. log(max(., 1e-10))
    4. taylor: where 1 < px < W-2 and 1 < py < H-2 and dxx dyy - dxy^2 != 0, coord -= Hessian^-1 gradient (5-point stencil)
    5. transform_preds for rot 0: image = center + (coord - (W/2, H/2)) * (200 scale[0] / W)

`dark_ref(..., fp32=False)` runs steps 2-5 in float64 on the fp32 map (it does not round the blurred map to fp32 as the
reference does: it is the exact statement the fp32 implementations are measured against); `fp32=True` runs every
operation in float32 in the order above, taps rounded to float32: a CPU stand-in for the device kernel's arithmetic.
One deviation, as in the kernel: where the ratio of step 2 is not finite the refinement is skipped (the reference
yields NaN there)."""
import numpy as np


def sigma_of(k):
    return 0.3 * ((k - 1) * 0.5 - 1) + 0.8


def taps(k):
    """float64 [k]: the normalised Gaussian of cv2.getGaussianKernel(k, 0) for k >= 9."""
    assert k % 2 == 1 and k >= 9
    x = np.arange(k, dtype=np.float64) - (k - 1) * 0.5
    t = np.exp(-(x * x) / (2.0 * sigma_of(k) ** 2))
    return t / t.sum()


def _pass(a, t, axis):
    """valid correlation of `a` with taps `t` along `axis` in a's dtype, taps in ascending order"""
    k = len(t)
    n = a.shape[axis] - (k - 1)
    out = None
    for i in range(k):
        sl = [slice(None)] * a.ndim
        sl[axis] = slice(i, i + n)
        term = a[tuple(sl)] * t[i]
        out = term if out is None else out + term
    return out


def blur_zero(hm, k, dtype=np.float64):
    """[..., H, W] -> the k x k Gaussian blur with zero padding, rows first, in `dtype`."""
    r = (k - 1) // 2
    t = taps(k).astype(dtype)
    a = np.asarray(hm).astype(dtype)
    pad = [(0, 0)] * (a.ndim - 2)
    a = _pass(np.pad(a, pad + [(0, 0), (r, r)]), t, a.ndim - 1)
    return _pass(np.pad(a, pad + [(r, r), (0, 0)]), t, a.ndim - 2)


def cv2_gaussian_blur(src, ksize, sigmaX=0):
    """Stand-in for cv2.GaussianBlur(src, (k, k), 0) on a 2-D float array: same shape and dtype, default border
    (BORDER_REFLECT_101 = numpy's 'reflect'), separable, rows first."""
    k = int(ksize[0])
    assert ksize[0] == ksize[1] and sigmaX == 0 and src.ndim == 2
    r = (k - 1) // 2
    t = taps(k).astype(src.dtype)
    a = _pass(np.pad(src, [(0, 0), (r, r)], mode='reflect'), t, 1)
    return _pass(np.pad(a, [(r, r), (0, 0)], mode='reflect'), t, 0)


def make_maps(rng, B, J, H, W, noise=1e-2):
    """Construction 1: one Gaussian peak per map, sigma 3, amplitude U(0.2, 1), centre U(-2, W+2) x U(-2, H+2), plus
    noise * N(0, 1) (real negatives, so the clamp of step 3 engages) -> float32 [B,J,H,W]."""
    amp = rng.uniform(0.2, 1.0, (B, J, 1, 1))
    cx = rng.uniform(-2.0, W + 2.0, (B, J, 1, 1))
    cy = rng.uniform(-2.0, H + 2.0, (B, J, 1, 1))
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    hm = amp * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2.0 * 3.0 ** 2)) + noise * rng.standard_normal((B, J, H, W))
    return hm.astype(np.float32)


def dark_ref(hm, center, scale, k=11, fp32=False):
    """hm float32 [B,J,H,W], center / scale [B,2] -> dict:
    preds [B,J,2] image coordinates, maxvals [B,J,1] float32, intc [B,J,2] the integer coordinates of step 1,
    coords [B,J,2] the refined heatmap coordinates, branch [B,J] (the guard of step 4 held and the ratio was finite),
    moved [B,J] (branch and det != 0), det [B,J] (nan where no branch), ratio [B,J]."""
    hm = np.asarray(hm)
    assert hm.dtype == np.float32 and hm.ndim == 4
    F = np.float32 if fp32 else np.float64
    B, J, H, W = hm.shape
    flat = hm.reshape(B, J, -1)
    idx = flat.argmax(2)
    maxvals = flat.max(2)
    pos = maxvals > 0
    intc = np.stack([(idx % W) * pos, (idx // W) * pos], -1).astype(F)
    bl = blur_zero(hm, k, F)
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = maxvals.astype(F) / bl.reshape(B, J, -1).max(2)
        lg = np.log(np.maximum(bl * ratio[:, :, None, None], F(1e-10)))
    coords = intc.copy()
    branch = np.zeros((B, J), bool)
    moved = np.zeros((B, J), bool)
    det = np.full((B, J), np.nan)
    for b in range(B):
        for j in range(J):
            px, py = int(intc[b, j, 0]), int(intc[b, j, 1])
            if not (1 < px < W - 2 and 1 < py < H - 2 and np.isfinite(ratio[b, j])):
                continue
            h = lg[b, j]
            branch[b, j] = True
            dx = F(0.5) * (h[py, px + 1] - h[py, px - 1])
            dy = F(0.5) * (h[py + 1, px] - h[py - 1, px])
            dxx = F(0.25) * (h[py, px + 2] - F(2) * h[py, px] + h[py, px - 2])
            dxy = F(0.25) * (h[py + 1, px + 1] - h[py - 1, px + 1] - h[py + 1, px - 1] + h[py - 1, px - 1])
            dyy = F(0.25) * (h[py + 2, px] - F(2) * h[py, px] + h[py - 2, px])
            d = dxx * dyy - dxy * dxy
            det[b, j] = d
            if d != 0:
                moved[b, j] = True
                coords[b, j, 0] -= (dyy * dx - dxy * dy) / d
                coords[b, j, 1] -= (dxx * dy - dxy * dx) / d
    c = np.asarray(center).astype(np.float32).astype(F).reshape(B, 1, 2)
    s = (np.asarray(scale).astype(np.float32).astype(F).reshape(B, 2)[:, 0] * F(200) / F(W)).reshape(B, 1, 1)
    preds = c + (coords - np.array([0.5 * W, 0.5 * H], F)) * s
    return {'preds': preds, 'maxvals': maxvals.reshape(B, J, 1), 'intc': intc, 'coords': coords, 'branch': branch,
            'moved': moved, 'det': det, 'ratio': ratio}
