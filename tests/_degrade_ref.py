"""A numpy restatement of the degradation stages written out in include/fami.h (fami_warp_degrade_batch_u8): tap
sampling in integers, colour in np.float32 operation by operation, occluders, normalisation.  It is held to
oracle.ops.cv2_warp_affine_u8 and to hand-derived numbers in test_degrade_host.py and is the reference of
test_degrade_gpu.py.  Nothing here is imported from the code under test."""
import numpy as np

BLUR, COLOUR, OCCLUDE = 1, 2, 4
F32 = np.float32


def lowbias32(v):
    v = np.asarray(v, np.uint64) & 0xffffffff
    v ^= v >> 16
    v = (v * 0x7feb352d) & 0xffffffff
    v ^= v >> 15
    v = (v * 0x846ca68b) & 0xffffffff
    v ^= v >> 16
    return v


def origin(mi, size):
    """(X0 + adelta, Y0 + bdelta) of every output pixel, [Hd,Wd] int64, in 1/1024 source pixel"""
    Wd, Hd = int(size[0]), int(size[1])
    mi = np.asarray(mi, np.float64)
    x, y = np.arange(Wd, dtype=np.float64), np.arange(Hd, dtype=np.float64)
    rnd = lambda v: np.clip(np.rint(v), -2147483648.0, 2147483647.0).astype(np.int64)
    adelta, bdelta = rnd(mi[0, 0] * x * 1024.0), rnd(mi[1, 0] * x * 1024.0)
    X0, Y0 = rnd((mi[0, 1] * y + mi[0, 2]) * 1024.0) + 16, rnd((mi[1, 1] * y + mi[1, 2]) * 1024.0) + 16
    return X0[:, None] + adelta[None, :], Y0[:, None] + bdelta[None, :]


def sample(src, X, Y, flip):
    """One bilinear sample per output pixel at (X, Y) in 1/32 source pixel -> [Hd,Wd,C] int64 in 0..255: integer
    weights summing to 2^15, zero border, columns mirrored under flip."""
    Hs, Ws = src.shape[:2]
    sx, sy = np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767)
    fx, fy = X & 31, Y & 31
    w = [(32 - fy) * (32 - fx) * 32, (32 - fy) * fx * 32, fy * (32 - fx) * 32, fy * fx * 32]
    acc = np.full(X.shape + (src.shape[2],), 1 << 14, np.int64)
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        yy, xx = sy + dy, sx + dx
        ok = (yy >= 0) & (yy < Hs) & (xx >= 0) & (xx < Ws)
        col = Ws - 1 - xx if flip else xx
        tap = src[np.clip(yy, 0, Hs - 1), np.clip(col, 0, Ws - 1)].astype(np.int64) * ok[..., None]
        acc += tap * w[k][..., None]
    return acc >> 15


def degrade_frame(src, mi, size, flip, bgr, rec, mean, std):
    """src [Hs,Ws,3] uint8, mi the 2x3 inverse map, rec a dict with the fields of fami_degrade_frame_t (flags, taps,
    step_x, step_y, alpha, delta, sat, seed, rects = [(x0, y0, x1, y1, mode, (f0, f1, f2)), ...]) -> [3,Hd,Wd] float32."""
    Wd, Hd = int(size[0]), int(size[1])
    src = np.asarray(src)
    if bgr:
        src = src[:, :, ::-1]                                    # output channel c reads source channel 2 - c
    PX, PY = origin(mi, size)
    flags = rec.get('flags', 0)
    if flags & BLUR:                                             # stage 1
        taps = int(rec['taps'])
        assert taps % 2 == 1 and 1 <= taps <= 15
        total = np.zeros((Hd, Wd, 3), np.int64)
        for k in range(-(taps - 1) // 2, (taps - 1) // 2 + 1):
            total += sample(src, (PX + k * int(rec['step_x'])) >> 5, (PY + k * int(rec['step_y'])) >> 5, flip)
        u = (2 * total + taps) // (2 * taps)
    else:
        u = sample(src, PX >> 5, PY >> 5, flip)
    t = u.astype(F32)
    if flags & COLOUR:                                           # stage 2: each operation rounded to float32
        alpha, delta, sat = F32(rec['alpha']), F32(rec['delta']), F32(rec['sat'])
        t = (t * alpha).astype(F32) + delta
        g = ((F32(0.299) * t[..., 0]) + (F32(0.587) * t[..., 1])) + (F32(0.114) * t[..., 2])
        assert t.dtype == F32 and g.dtype == F32
        t = g[..., None] + (sat * (t - g[..., None])).astype(F32)
        t = np.minimum(np.maximum(t, F32(0)), F32(255))
        assert t.dtype == F32
    if flags & OCCLUDE:                                          # stage 3: the later rectangle wins
        yy, xx = np.mgrid[0:Hd, 0:Wd]
        assert len(rec['rects']) <= 4
        for x0, y0, x1, y1, mode, fill in rec['rects']:
            cover = (xx >= x0) & (xx < x1) & (yy >= y0) & (yy < y1)
            for c in range(3):
                if mode:
                    idx = ((c * Hd + yy) * Wd + xx) & 0xffffffff
                    val = (lowbias32(idx ^ (int(rec['seed']) & 0xffffffff)) >> 24).astype(F32)
                else:
                    val = F32(fill[c])
                t[..., c] = np.where(cover, val, t[..., c])
    mean, std = np.asarray(mean, F32), np.asarray(std, F32)
    out = ((t / F32(255)) - mean) / std                          # stage 4
    assert out.dtype == F32
    return np.ascontiguousarray(out.transpose(2, 0, 1))


def degrade_clip(frames, mi, size, flip, bgr, recs, mean, std):
    """frames [F,Hs,Ws,3] -> (key [3,Hd,Wd], sup [3(F-1),Hd,Wd]) as the batched launch lays them out"""
    out = [degrade_frame(frames[f], mi, size, flip, bgr, recs[f], mean, std) for f in range(len(frames))]
    Wd, Hd = int(size[0]), int(size[1])
    return out[0], (np.concatenate(out[1:]) if len(out) > 1 else np.zeros((0, Hd, Wd), F32))
