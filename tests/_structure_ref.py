"""The structure (limb-direction cosine) term restated in float64 numpy, operation for operation as include/fami.h words it: the
reference of tests/test_structure_host.py (hand-derived numbers, torch's cosine_similarity under autograd) and
tests/test_structure_gpu.py (the kernels of csrc/loss.hip).  numpy evaluates every float64 operation on its own, so nothing here
is contracted; the order of the operations is the header's."""
import numpy as np

F32, F64 = np.float32, np.float64


def _f32(v):
    """a scalar the C ABI takes as `float`, as the float64 the kernel widens it to"""
    return F64(F32(v))


def limbs(coords, txy, w, pairs, min_len=1.0, eps=1e-8):
    """coords, txy [B,J,2] (read as fp32), w [B,J] or None, pairs [P,2] ->
    valid [B,P] bool, cos [B,P] float64 (0 where not valid), dcos [B,P,2] float64 = dcos/du (0 where not valid)"""
    c, t = np.asarray(coords, F32).astype(F64), np.asarray(txy, F32).astype(F64)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    a, b = pairs[:, 0], pairs[:, 1]
    eps, ml2 = _f32(eps), _f32(min_len) * _f32(min_len)
    with np.errstate(all='ignore'):
        td, ud = t[:, b] - t[:, a], c[:, b] - c[:, a]
        tx, ty, ux, uy = td[..., 0], td[..., 1], ud[..., 0], ud[..., 1]
        tt = tx * tx + ty * ty
        valid = tt > ml2
        if w is not None:
            wf = np.asarray(w, F32).reshape(c.shape[0], c.shape[1])
            valid = valid & (wf[:, a] > 0) & (wf[:, b] > 0)
        uu = ux * ux + uy * uy
        ut = ux * tx + uy * ty
        nu, nt = np.sqrt(uu), np.sqrt(tt)
        clamp = nu <= eps
        mu, mt = np.where(clamp, eps, nu), np.where(nt <= eps, eps, nt)
        nn = mu * mt
        cos = ut / nn
        dx, dy = tx / nn, ty / nn
        n2 = nu * nu
        dx = np.where(clamp, dx, dx - (cos * ux) / n2)
        dy = np.where(clamp, dy, dy - (cos * uy) / n2)
    zero = np.zeros_like(cos)
    return valid, np.where(valid, cos, zero), np.stack([np.where(valid, dx, zero), np.where(valid, dy, zero)], -1)


def rows(coords, txy, w, pairs, min_len=1.0, eps=1e-8):
    """-> the row values l[s,p] = valid ? 1 - cos : 0 in float64 [B,P] (the kernel stores them rounded once to fp32)"""
    valid, cos, _ = limbs(coords, txy, w, pairs, min_len, eps)
    return np.where(valid, 1.0 - cos, 0.0)


def loss(rows32, scale):
    """scale * the float64 sum of the fp32 row values"""
    return float(np.asarray(rows32, F32).astype(F64).sum() * F64(scale))


def gcoords(coords, txy, w, pairs, scale, gdev=None, min_len=1.0, eps=1e-8):
    """-> [B,J,2] float64: g sum_p valid_p (-dcos/du_p) (+1 at b_p, -1 at a_p), the limbs in list order; g = scale (* gdev) as
    the fp32 product; 0 for a joint on no valid limb.  (The kernel rounds it once to fp32.)"""
    valid, _, d = limbs(coords, txy, w, pairs, min_len, eps)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    B, J = np.asarray(coords).shape[:2]
    g = F64(F32(scale) * F32(gdev)) if gdev is not None else _f32(scale)
    acc = np.zeros((B, J, 2), F64)
    on = np.zeros((B, J), bool)
    for p, (a, b) in enumerate(pairs):
        v = valid[:, p]
        acc[v, b] = acc[v, b] - d[v, p]
        acc[v, a] = acc[v, a] + d[v, p]
        on[v, a] = on[v, b] = True
    with np.errstate(all='ignore'):
        return np.where(on[..., None], g * acc, 0.0)


def ulp32(v):
    """one unit in the last place of fp32 at |v| (float64 array in, float64 out); the smallest subnormal at 0"""
    v32 = np.abs(np.asarray(v, F64)).astype(F32)
    return (np.nextafter(v32, F32(np.inf)) - v32).astype(F64)


# ---- seeded inputs of the GPU tests: predicted limbs at least 0.5 px long, target limbs well clear of min_len
def skeleton_case(B, J, pairs, seed, H=24.0, W=18.0):
    """-> coords, txy [B,J,2] fp32 and w [B,J] fp32 (all 1) such that every limb of `pairs` has a predicted length >= 0.5 px and
    a target length >= 1.5 px: joints are drawn again until both hold."""
    rng = np.random.RandomState(seed)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    size = np.array([W, H])
    t = (rng.rand(B, J, 2) * size).astype(F32)
    c = (t + rng.randn(B, J, 2) * 1.5).astype(F32)
    for _ in range(1000):
        lt = np.linalg.norm(t[:, pairs[:, 1]].astype(F64) - t[:, pairs[:, 0]], axis=-1)
        lc = np.linalg.norm(c[:, pairs[:, 1]].astype(F64) - c[:, pairs[:, 0]], axis=-1)
        bad = (lt < 1.5) | (lc < 0.5)
        if not bad.any():
            break
        s, p = np.nonzero(bad)
        j = pairs[p, 1]
        t[s, j] = (rng.rand(len(s), 2) * size).astype(F32)
        c[s, j] = (t[s, j] + rng.randn(len(s), 2) * 1.5).astype(F32)
    else:
        raise AssertionError('no admissible draw')
    return c, t, np.ones((B, J), F32)


def star_pairs(J=64, P=64):
    """the caps: joint 0 on 40 limbs (as a and as b in turn), then a chain and a few repeats, every joint index below J"""
    out = [((0, k) if k % 2 else (k, 0)) for k in range(1, 41)]
    out += [(k, k + 1) for k in range(41, 63)]
    out += [(63, 1), (5, 62)]
    assert len(out) == P and all(0 <= a < J and 0 <= b < J and a != b for a, b in out)
    return tuple(out)
