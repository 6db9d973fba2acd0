"""Reference of the integral (soft-argmax) coordinate term and decode for tests/test_integral_host.py, tests/test_integral_gpu.py
and tests/test_train_gpu_integral.py: the definition of include/fami.h restated in float64, and the "plain fp32" yardstick (the
evaluation a careful fp32 program makes: torch.softmax(beta * h) followed by weighted sums, all fp32, on the CPU) whose own
error against float64 sets the bounds of the accuracy tests.

Everything takes the fp32 OPERANDS the kernel sees (CPU tensors) and follows the one rounding the definition fixes: a = beta * h
is formed in fp32 (beta as fp32) before anything is widened, so both evaluations and the kernel start from the same logits."""
import numpy as np
import torch

F32, F64 = torch.float32, torch.float64
MARGIN = 8.0              # the project's rule (tests/_stream_exact.py, softmax_kl): 8 x the fp32 yardstick's own error ...
FLOOR = 2.0 ** -20        # ... with a floor of 2^-20 of the coordinate range (of the row maximum for the gradient)


def logits(h, beta):
    """a = beta * h, ONE fp32 rounding -> [R,L] fp32"""
    return (h.to(F32).reshape(h.shape[0], -1) * torch.tensor(beta, dtype=F32)).to(F32)


def grids(H, W, dtype):
    l = torch.arange(H * W)
    return (l % W).to(dtype), torch.div(l, W, rounding_mode='floor').to(dtype)


def forward(h, beta, dtype=F64, e32=False):
    """h [R,H,W] fp32 -> cx, cy [R] (heatmap pixels), m [R] (fp32 row maxima of a), Z [R], p [R,L] in dtype.
    e32: e = exp(a - m) is rounded to fp32 before it is summed (the exact cases: expf(-512) IS 0 there, where float64 keeps
    4e-223)"""
    R, H, W = h.shape
    a32 = logits(h, beta)
    m = a32.max(1).values
    x, y = grids(H, W, dtype)
    e = torch.exp(a32.to(dtype) - m.to(dtype)[:, None])
    if e32:
        e = e.to(F32).to(dtype)
    Z = e.sum(1)
    return (e * x).sum(1) / Z, (e * y).sum(1) / Z, m, Z, e / Z[:, None]


def forward_plain32(h, beta):
    """the yardstick: torch.softmax of the fp32 logits, then weighted sums, all fp32 -> cx, cy [R] fp32"""
    R, H, W = h.shape
    p = torch.softmax(logits(h, beta), 1)
    x, y = grids(H, W, F32)
    return (p * x).sum(1), (p * y).sum(1)


def rows(cx, cy, txy, w, H, W):
    """w_r (|cx - tx| / W + |cy - ty| / H) in the dtype of cx"""
    t = txy.to(cx.dtype)
    return w.to(cx.dtype) * ((cx - t[:, 0]).abs() / W + (cy - t[:, 1]).abs() / H)


def loss(h, beta, txy, w, scale, dtype=F64):
    R, H, W = h.shape
    cx, cy = forward(h, beta, dtype)[:2] if dtype == F64 else forward_plain32(h, beta)
    return rows(cx, cy, txy, w, H, W).sum() * scale


def grad(h, beta, txy, w, g, dtype=F64, e32=False):
    """d loss / d h with loss = g sum_r rows_r, the closed form of include/fami.h (sgn(0) = 0) -> [R,H,W] in dtype"""
    R, H, W = h.shape
    if dtype == F64:
        cx, cy, _, _, p = forward(h, beta, F64, e32)
    else:
        cx, cy = forward_plain32(h, beta)
        p = torch.softmax(logits(h, beta), 1)
    x, y = grids(H, W, dtype)
    t = txy.to(dtype)
    sx, sy = torch.sign(cx - t[:, 0]) / W, torch.sign(cy - t[:, 1]) / H
    c = torch.tensor(g, dtype=dtype) * w.to(dtype) * torch.tensor(beta, dtype=F32).to(dtype)
    d = c[:, None] * p * (sx[:, None] * (x[None] - cx[:, None]) + sy[:, None] * (y[None] - cy[:, None]))
    return d.reshape(R, H, W)


def loss_autograd(h, beta, txy, w, g):
    """the same loss written with differentiable torch float64 operations: (value, d / d h).  The rounding of a = beta * h to
    fp32 has no derivative: torch differentiates softmax and the sums with respect to the logits a, and d a / d h = beta."""
    R, H, W = h.shape
    a = logits(h, beta).double().requires_grad_(True)
    p = torch.softmax(a, 1)
    x, y = grids(H, W, F64)
    cx, cy = (p * x).sum(1), (p * y).sum(1)
    v = g * (w.double() * ((cx - txy[:, 0].double()).abs() / W + (cy - txy[:, 1].double()).abs() / H)).sum()
    v.backward()
    return v.detach(), (a.grad * float(np.float32(beta))).reshape(R, H, W)


def softargmax_grad(h, beta, gc, dtype=F64):
    """d (sum_r gc[r,0] cx_r + gc[r,1] cy_r) / d h -> [R,H,W]"""
    R, H, W = h.shape
    if dtype == F64:
        cx, cy, _, _, p = forward(h, beta, F64)
    else:          # the plain fp32 yardstick, as in grad()
        cx, cy = forward_plain32(h, beta)
        p = torch.softmax(logits(h, beta), 1)
    x, y = grids(H, W, dtype)
    gc = gc.to(dtype)
    b = torch.tensor(beta, dtype=F32).to(dtype)
    d = b * p * (gc[:, 0:1] * (x[None] - cx[:, None]) + gc[:, 1:2] * (y[None] - cy[:, None]))
    return d.reshape(R, H, W)


def affine(x, y, center, scale, H, W, dtype=F64):
    """transform_preds for rot 0 (the inverse affine of get_final_preds): heatmap (x, y) [B,J] -> image coordinates [B,J,2]"""
    s = (scale[:, 0].to(dtype) * 200.0 / W)[:, None]
    c = center.to(dtype)
    return torch.stack([c[:, 0:1] + (x - 0.5 * W) * s, c[:, 1:2] + (y - 0.5 * H) * s], -1)


def decode(hm, center, scale, beta, dtype=F64):
    """hm [B,J,H,W] fp32 -> (preds [B,J,2] in dtype, maxvals [B,J] fp32, masked [B,J] bool): the soft-argmax through the
    inverse affine; a joint whose maximum is not > 0 (NaN included) decodes from (0, 0) as get_final_preds does"""
    B, J, H, W = hm.shape
    h = hm.reshape(B * J, H, W)
    if dtype == F64:
        cx, cy = forward(h, beta, F64)[:2]
    else:
        cx, cy = forward_plain32(h, beta)
    flat = hm.reshape(B, J, -1)
    maxvals = torch.where(torch.isnan(flat).any(2), torch.tensor(float('nan')), flat.max(2).values)
    masked = ~(maxvals > 0)
    cx = torch.where(masked, torch.zeros((), dtype=dtype), cx.reshape(B, J))
    cy = torch.where(masked, torch.zeros((), dtype=dtype), cy.reshape(B, J))
    return affine(cx, cy, center, scale, H, W, dtype), maxvals, masked


def subpixel_map(H, W, cx, cy, sigma=3):
    """The map fami_gauss_target_ex_f32(subpixel = 1) draws for a visible joint at heatmap position (cx, cy) (float64): fp32
    Gaussian at the real-valued centre inside the (2 * 3 sigma + 1)^2 window of the rounded centre, zero elsewhere."""
    mx, my = int(cx + 0.5), int(cy + 0.5)
    r = 3 * sigma
    m = np.zeros((H, W), np.float32)
    inv = np.float32(2 * sigma * sigma)
    for y in range(max(0, my - r), min(H, my + r + 1)):
        for x in range(max(0, mx - r), min(W, mx + r + 1)):
            dx, dy = np.float32(np.float64(x) - cx), np.float32(np.float64(y) - cy)
            m[y, x] = np.exp(-(dx * dx + dy * dy) / inv, dtype=np.float32)
    return m


# ---- the exact cases: K pixels at 0, every other pixel at -64, beta = 8, 16 x 8 maps
EX_H, EX_W, EX_BETA, EX_LOW = 16, 8, 8.0, -64.0
EX_CASES = [(K, R) for K in (1, 2, 4) for R in (1, 15)]


def exact_case(K, R):
    """-> operands and results of one exact case, with the conditions under which every result is determined whatever the
    summation order and whether or not a multiply-add is contracted asserted HERE, on the reference alone:
      every non-maximal term is expf(-512), which is 0 in fp32 (and in float64 it is below 2^-700: it changes no fp32 result);
      e is 0 or 1, so Z = K and the sums of e x, e y are small integers; K is a power of two: cx, cy are multiples of 1/4;
      the targets are multiples of 1/4, W and H powers of two, the weights, scales and gdev powers of two (or 0):
      row values are multiples of 2^-7 below 2^3, their fp64 sum and its one rounding to fp32 are exact;
      gradient elements are multiples of 2^-9 below 2^5 and the prior holds small integers: every sum fits 24 bits."""
    g = torch.Generator().manual_seed(1000 * K + R)
    H, W = EX_H, EX_W
    h = torch.full((R, H * W), EX_LOW, dtype=F32)
    cx, cy = torch.zeros(R, dtype=F64), torch.zeros(R, dtype=F64)
    for r in range(R):
        idx = torch.randperm(H * W, generator=g)[:K]
        h[r, idx] = 0.0
        cx[r], cy[r] = (idx % W).double().mean(), torch.div(idx, W, rounding_mode='floor').double().mean()
    h = h.reshape(R, H, W)
    assert np.exp(np.float32(EX_BETA * EX_LOW)) == 0.0 and np.float32(EX_BETA) * np.float32(EX_LOW) == -512.0
    assert bool((cx * 4 == (cx * 4).round()).all()) and bool((cy * 4 == (cy * 4).round()).all())
    f64 = forward(h, EX_BETA, e32=True)
    assert torch.equal(f64[0], cx) and torch.equal(f64[1], cy) and torch.equal(f64[3], torch.full((R,), float(K), dtype=F64))
    txy = torch.stack([torch.randint(0, 4 * W, (R,), generator=g).double() / 4, torch.randint(0, 4 * H, (R,), generator=g).double() / 4], 1)
    txy[0] = torch.stack([cx[0], cy[0] + 0.25])          # sgn(0) = 0 on one axis of the first row
    w = torch.tensor([0.0, 0.5, 1.0, 2.0], dtype=F64)[torch.randint(0, 4, (R,), generator=g)]
    if R > 1:
        w[1] = 0.0
    rv = rows(cx, cy, txy, w, H, W)
    assert bool((rv * 128 == (rv * 128).round()).all()) and rv.max().item() < 8 and rv.sum().item() * 128 < 2 ** 24
    scales = (2.0 ** -3, 2.0 ** -10)
    want_loss = [torch.tensor([rv.sum().item() * s], dtype=F64) for s in scales]
    assert all(v.float().double().equal(v) for v in want_loss)
    gscale, g0 = 2.0 ** -3, 4.0
    prior = torch.randint(-4, 5, (R, H, W), generator=g).double()
    grads = {}
    for acc in (0, 1):
        for hg in (0, 1):
            d = grad(h, EX_BETA, txy, w, gscale * (g0 if hg else 1.0), e32=True)
            assert bool((d * 512 == (d * 512).round()).all()) and d.abs().max().item() < 32
            # ... and it is the float64 autograd gradient of the same loss, to rounding
            assert (d - loss_autograd(h, EX_BETA, txy, w, gscale * (g0 if hg else 1.0))[1]).abs().max().item() < 1e-12
            grads[acc, hg] = d + (prior if acc else 0)
    return dict(h=h, cx=cx, cy=cy, txy=txy, w=w, rows=rv, scales=scales, want_loss=want_loss, gscale=gscale, g0=g0, prior=prior,
                grads=grads, K=K, R=R)


# ---- general operands
def general_maps(R, H, W, seed):
    """R maps: Gaussian noise of 0.2 (logits of 4 at beta = 20: a broad distribution over many pixels), and on every second
    row a sigma-3 sub-pixel peak on top where the map has room for one (the shape the head produces)"""
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(R, H, W, generator=g) * 0.2
    if H >= 8 and W >= 8:
        for r in range(0, R, 2):
            c = torch.rand(2, generator=g).double() * torch.tensor([W - 1.0, H - 1.0], dtype=F64)
            h[r] += torch.from_numpy(subpixel_map(H, W, c[0].item(), c[1].item()))
    return h.float()


def general_targets(h, beta, seed):
    """targets at least a quarter pixel from the float64 coordinates on both axes (the sign of cx - tx is then the same for
    every evaluation), weights in (0.5, 1.5)"""
    R = h.shape[0]
    g = torch.Generator().manual_seed(seed + 1)
    cx, cy = forward(h, beta)[:2]
    off = (0.25 + torch.rand(R, 2, generator=g).double() * 3) * (torch.randint(0, 2, (R, 2), generator=g).double() * 2 - 1)
    txy = (torch.stack([cx, cy], 1) + off).float()
    assert bool(((txy.double() - torch.stack([cx, cy], 1)).abs() >= 0.2).all())
    w = (0.5 + torch.rand(R, generator=g)).float()
    return txy, w
