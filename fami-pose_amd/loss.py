"""On-device heatmap loss, Gaussian targets and decode (NCHW boundary tensors).

Mirrors posetimation/loss/mse_loss.py:13-40 (JointMSELoss),
datasets/process/heatmaps_process.py:146-203 (generate_heatmaps) and :16-44
(get_max_preds), engine/core/utils/evaluate.py:13-75 (accuracy).  The reductions
run in HIP; only the final [B,J]-sized PCK bookkeeping (a few dozen scalars)
is host arithmetic, as in the reference.
"""
import numpy as np
import torch
import torch.nn as nn

from ._lib import lib
from .data import LIMB_PAIRS


def _p(t):
    return None if t is None else t.data_ptr()


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _need_cuda(t):
    if not t.is_cuda:
        raise RuntimeError("fami_pose_amd losses run on the HIP path only (tensor is on %s)" % t.device)


class _WMSE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, w, scale):
        R, L = pred.shape[0] * pred.shape[1], pred[0, 0].numel()
        out = torch.empty(1, device=pred.device)
        ws = torch.empty(R, device=pred.device)
        lib().call('fami_wmse_fwd_f32', _p(pred), _p(gt), _p(w), _p(out), R, L, float(scale), _p(ws), _stream(pred))
        ctx.save_for_backward(pred, gt, w)
        ctx.scale = scale
        return out.reshape(())

    @staticmethod
    def backward(ctx, g):
        pred, gt, w = ctx.saved_tensors
        R, L = pred.shape[0] * pred.shape[1], pred[0, 0].numel()
        d = torch.empty_like(pred)
        lib().call('fami_wmse_bwd_f32', _p(pred), _p(gt), _p(w), _p(d), R, L, float(ctx.scale),
                   _p(g.reshape(1).contiguous()), 0, _stream(pred))
        return d, None, None, None


class JointMSELoss(nn.Module):
    """(1/J) sum_j mean_{b,p} (w_bj (pred - gt))^2, one fused reduction instead of the reference's J-step loop."""

    def __init__(self, use_target_weight=True, divided_num_joints=True):
        super().__init__()
        self.use_target_weight = use_target_weight
        self.divided_num_joints = divided_num_joints

    def forward(self, output, target, target_weight):
        _need_cuda(output)
        B, J = output.shape[:2]
        L = output[0, 0].numel()
        scale = 1.0 / (B * L) / (J if self.divided_num_joints else 1)
        w = target_weight.reshape(B * J).float().contiguous() if self.use_target_weight else None
        return _WMSE.apply(output.float().contiguous(), target.float().contiguous(), w, scale)


class _OHKM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, w, k, scale):
        B, J = pred.shape[:2]
        L = pred[0, 0].numel()
        out = torch.empty(1, device=pred.device)
        sel_w = torch.empty(B * J, device=pred.device)
        ws = torch.empty(B * J, device=pred.device)
        lib().call('fami_ohkm_fwd_f32', _p(pred), _p(gt), _p(w), _p(out), _p(sel_w), B, J, L, k, float(scale), _p(ws),
                   _stream(pred))
        ctx.save_for_backward(pred, gt, sel_w)
        ctx.scale = scale
        return out.reshape(())

    @staticmethod
    def backward(ctx, g):
        pred, gt, sel_w = ctx.saved_tensors
        R, L = pred.shape[0] * pred.shape[1], pred[0, 0].numel()
        d = torch.empty_like(pred)
        lib().call('fami_wmse_bwd_f32', _p(pred), _p(gt), _p(sel_w), _p(d), R, L, float(ctx.scale),
                   _p(g.reshape(1).contiguous()), 0, _stream(pred))
        return d, None, None, None, None


def check_ohkm_topk(k, num_joints=None):
    """-> int(k), or ValueError: an integer (not a bool) with 1 <= k (<= num_joints where that is known)."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1 or (num_joints is not None and k > num_joints):
        raise ValueError('OHKM topk is an integer with 1 <= topk <= the number of joints%s, not %r' %
                         ('' if num_joints is None else ' (%d)' % num_joints, k))
    return int(k)


class JointOHKMMSELoss(nn.Module):
    """Online hard keypoint mining (the HRNet family's JointsOHKMMSELoss): per sample only the `topk` joints with the largest
    loss count, (1/B) sum_b (1/k) sum_{j in top-k of b} mean_p (w_bj (pred - gt))^2.  The selection runs on the device
    (fami_ohkm_fwd_f32: larger first, equal losses by lower joint index, NaN first) and carries no gradient; the backward
    pass is JointMSELoss's with the weights of the unselected joints zeroed.  HRNet's factor 0.5 is deliberately NOT
    here: topk = J is then exactly this project's JointMSELoss, and a caller who wants HRNet's value puts the 0.5 into
    the weight of the term (the Trainer's mse_weight)."""

    def __init__(self, topk=8, use_target_weight=True):
        super().__init__()
        self.topk = check_ohkm_topk(topk)
        self.use_target_weight = use_target_weight

    def forward(self, output, target, target_weight):
        _need_cuda(output)
        B, J = output.shape[:2]
        k = check_ohkm_topk(self.topk, J)
        L = output[0, 0].numel()
        w = target_weight.reshape(B * J).float().contiguous() if self.use_target_weight else None
        return _OHKM.apply(output.float().contiguous(), target.float().contiguous(), w, k, 1.0 / (B * L * k))


ENCODINGS = ('quantised', 'subpixel')


def check_target_options(encoding, joint_weights, num_joints=None):
    """-> (subpixel flag, joint weights as a tuple of floats or None), or ValueError -- host arithmetic only."""
    if encoding not in ENCODINGS:
        raise ValueError("encoding is 'quantised' or 'subpixel', not %r" % (encoding,))
    if joint_weights is not None:
        jw = joint_weights.detach().cpu().reshape(-1).tolist() if torch.is_tensor(joint_weights) else \
            [float(v) for v in np.asarray(joint_weights, dtype=np.float64).reshape(-1)]
        if not jw or (num_joints is not None and len(jw) != num_joints):
            raise ValueError('joint_weights holds %d values for %s joints' %
                             (len(jw), 'no' if num_joints is None else num_joints))
        joint_weights = tuple(jw)
    return encoding == 'subpixel', joint_weights


def generate_heatmaps(joints, joints_vis, sigma, image_size, heatmap_size, encoding='quantised', joint_weights=None):
    """joints [B,J,2|3] (pixels, device), joints_vis [B,J] or [B,J,3] -> target [B,J,Hh,Wh], weight [B,J,1].
    image_size / heatmap_size are (w, h) as in the reference.
    joint_weights: J factors (sequence or tensor) of the returned weights, the reference's USE_DIFFERENT_JOINTS_WEIGHT
    (heatmaps_process.py:200-201; data.JOINTS_WEIGHT is PoseTrack's vector); whether a map is drawn still follows the
    unmultiplied weight.
    encoding='subpixel': the Gaussian is centred at the real-valued position joint / stride instead of the rounded one --
    the encoding the DARK decode (dark_get_final_preds) assumes.  Window and weight stay those of the rounded centre, so
    the two encodings differ only in the values inside the window, and a joint at a non-negative integer position gets
    the same bits under both.  At exactly half a pixel the sub-pixel map has two equal maxima and its first one is the
    LOWER pixel, where the quantised centre is the upper one."""
    B, J = joints.shape[:2]
    sub, jw = check_target_options(encoding, joint_weights, J)
    _need_cuda(joints)
    xy = joints[..., :2].float().contiguous()
    vis = (joints_vis[..., 0] if joints_vis.dim() == 3 else joints_vis).float().contiguous()
    Wh, Hh = int(heatmap_size[0]), int(heatmap_size[1])
    target = torch.empty(B, J, Hh, Wh, device=joints.device)
    weight = torch.empty(B, J, device=joints.device)
    if not sub and jw is None:
        lib().call('fami_gauss_target_f32', _p(xy), _p(vis), _p(target), _p(weight), B, J, Hh, Wh, int(image_size[1]),
                   int(image_size[0]), int(sigma), _stream(joints))
    else:
        jw = None if jw is None else torch.tensor(jw, dtype=torch.float32, device=joints.device)
        lib().call('fami_gauss_target_ex_f32', _p(xy), _p(vis), _p(jw), _p(target), _p(weight), B, J, Hh, Wh,
                   int(image_size[1]), int(image_size[0]), int(sigma), int(sub), _stream(joints))
    return target, weight.reshape(B, J, 1)


def argmax_indices(hm, with_max=False):
    """flat row-major argmax per (b, j), first max on ties -> int64 [B,J]."""
    _need_cuda(hm)
    B, J = hm.shape[:2]
    L = hm[0, 0].numel()
    idx = torch.empty(B, J, dtype=torch.int64, device=hm.device)
    mx = torch.empty(B, J, device=hm.device)
    lib().call('fami_argmax2d_f32', _p(hm.float().contiguous()), _p(idx), _p(mx), B * J, L, _stream(hm))
    return (idx, mx) if with_max else idx


def get_max_preds(hm):
    """-> preds [B,J,2] float32 (x, y; zeroed where max <= 0), maxvals [B,J,1]."""
    idx, mx = argmax_indices(hm, with_max=True)
    W = hm.shape[3]
    preds = torch.stack([(idx % W).float(), torch.div(idx, W, rounding_mode='floor').float()], -1)
    preds = preds * (mx > 0).float().unsqueeze(-1)
    return preds, mx.unsqueeze(-1)


def get_final_preds(batch_heatmaps, center, scale):
    """On-device get_final_preds (datasets/process/heatmaps_process.py:47-73): heatmaps [B,J,H,W] (device),
    center / scale [B,2] -> (preds [B,J,2] image coordinates, maxvals [B,J,1]) as device tensors."""
    _need_cuda(batch_heatmaps)
    B, J, H, W = batch_heatmaps.shape
    dev = batch_heatmaps.device
    c = torch.as_tensor(center, dtype=torch.float32, device=dev).reshape(B, 2).contiguous()
    sc = torch.as_tensor(scale, dtype=torch.float32, device=dev).reshape(B, 2).contiguous()
    preds = torch.empty(B, J, 2, device=dev)
    mx = torch.empty(B, J, device=dev)
    ws = torch.empty(B * J, dtype=torch.int64, device=dev)
    lib().call('fami_final_preds_f32', _p(batch_heatmaps.float().contiguous()), _p(c), _p(sc), _p(preds), _p(mx), _p(ws),
               B, J, H, W, _stream(batch_heatmaps))
    return preds, mx.unsqueeze(-1)


def check_blur_kernel(k):
    """-> int(k), or ValueError: the DARK decode accepts an odd Gaussian kernel size with 9 <= k <= 17.  (OpenCV uses fixed
    tables instead of the formula for k = 3, 5, 7, and nothing available here can pin them.)"""
    if isinstance(k, bool) or int(k) != k or int(k) % 2 == 0 or not 9 <= int(k) <= 17:
        raise ValueError('blur_kernel must be an odd integer with 9 <= k <= 17, got %r' % (k,))
    return int(k)


def gaussian_taps(k):
    """The k taps of cv2.GaussianBlur(., (k, k), 0) as float32: sigma = 0.3 ((k - 1) / 2 - 1) + 0.8 (2.0 for k = 11),
    exp(-x^2 / (2 sigma^2)) normalised to sum 1 in float64, then rounded."""
    k = check_blur_kernel(k)
    sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    x = np.arange(k, dtype=np.float64) - (k - 1) * 0.5
    t = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return (t / t.sum()).astype(np.float32)


_TAPS_CACHE = {}


def _taps_on(dev, k):
    """gaussian_taps(k) as a device tensor; one upload per (device, k)."""
    key = (str(dev), k)
    t = _TAPS_CACHE.get(key)
    if t is None:
        t = _TAPS_CACHE[key] = torch.from_numpy(gaussian_taps(k)).to(dev)
    return t


def dark_get_final_preds(batch_heatmaps, center, scale, blur_kernel=11):
    """On-device dark_get_final_preds (datasets/process/heatmaps_process.py:84-143), the distribution-aware decode: argmax
    of the unblurred map, a blur_kernel x blur_kernel Gaussian blur rescaled to the original maximum, log, one Newton step
    at the peak, inverse affine -- one launch (csrc/decode.hip).  Same conventions as get_final_preds: heatmaps [B,J,H,W]
    (device), center / scale [B,2] -> (preds [B,J,2] image coordinates, maxvals [B,J,1]) as device tensors."""
    k = check_blur_kernel(blur_kernel)
    _need_cuda(batch_heatmaps)
    B, J, H, W = batch_heatmaps.shape
    need, limit = lib().cdll.fami_dark_preds_lds_bytes(H, W, k), lib().cdll.fami_dark_preds_lds_limit()     # host arithmetic
    if need > limit:
        raise ValueError('dark_get_final_preds: a %dx%d map at blur_kernel %d needs %d bytes of LDS (the padded map and its '
                         'row pass, 4 (H (W + k - 1) + (H + k - 1) W)); the limit is %d' % (H, W, k, need, limit))
    dev = batch_heatmaps.device
    c = torch.as_tensor(center, dtype=torch.float32, device=dev).reshape(B, 2).contiguous()
    sc = torch.as_tensor(scale, dtype=torch.float32, device=dev).reshape(B, 2).contiguous()
    preds = torch.empty(B, J, 2, device=dev)
    mx = torch.empty(B, J, device=dev)
    lib().call('fami_dark_preds_f32', _p(batch_heatmaps.float().contiguous()), _p(c), _p(sc), _p(_taps_on(dev, k)), k,
               _p(preds), _p(mx), B, J, H, W, _stream(batch_heatmaps))
    return preds, mx.unsqueeze(-1)


def check_integral_options(weight, beta):
    """-> (float(weight), float(beta)), or ValueError -- host arithmetic only.  weight: a finite number > 0 (the factor of
    the integral L1 term); beta: a finite number > 0 (the soft-argmax sharpness, 1 / temperature)."""
    for name, v in (('weight', weight), ('beta', beta)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
            raise ValueError('integral L1 %s is a finite number, not %r' % (name, v))
    if not weight > 0:
        raise ValueError('integral L1 weight must be > 0 (None switches the term off), got %r' % (weight,))
    if not 0 < beta <= float(np.finfo(np.float32).max):
        raise ValueError('integral beta must be > 0 and finite in fp32, got %r' % (beta,))
    return float(weight), float(beta)


def _softargmax_fwd(hm, beta):
    """hm [B,J,H,W] fp32 contiguous -> (coords [B*J,2], stats [B*J,2])"""
    B, J, H, W = hm.shape
    coords = torch.empty(B * J, 2, device=hm.device)
    stats = torch.empty(B * J, 2, device=hm.device)
    lib().call('fami_softargmax_fwd_f32', _p(hm), _p(coords), _p(stats), B * J, H, W, beta, _stream(hm))
    return coords, stats


class _SoftArgmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hm, beta):
        coords, stats = _softargmax_fwd(hm, beta)
        ctx.save_for_backward(hm, coords, stats)
        ctx.beta = beta
        return coords.reshape(hm.shape[0], hm.shape[1], 2).clone()

    @staticmethod
    def backward(ctx, g):
        hm, coords, stats = ctx.saved_tensors
        B, J, H, W = hm.shape
        d = torch.empty_like(hm)
        lib().call('fami_softargmax_bwd_f32', _p(hm), _p(coords), _p(stats), _p(g.float().contiguous()), _p(d), B * J, H, W,
                   ctx.beta, 0, _stream(hm))
        return d, None


def soft_argmax(hm, beta=20.0):
    """Heatmaps [B,J,H,W] (device) -> the expectation of the pixel position under softmax(beta * hm) per map, [B,J,2] =
    (x, y) in heatmap pixels (fami_softargmax_fwd_f32; differentiable: fami_softargmax_bwd_f32).  beta = 20 is the
    reference's heatmap temperature T = 0.05 (Alignment_V15.py:250-277)."""
    _, beta = check_integral_options(1.0, beta)
    _need_cuda(hm)
    if hm.dim() != 4:
        raise ValueError('soft_argmax takes heatmaps [B,J,H,W], got %s' % (tuple(hm.shape),))
    return _SoftArgmax.apply(hm.float().contiguous(), beta)


def heatmap_xy(joints, image_size, heatmap_size):
    """joints [B,J,2|3] (input-image pixels, device) -> [B,J,2] heatmap pixels, joint / feature stride: the position
    generate_heatmaps(encoding='subpixel') centres its Gaussian at (the same expression, rounded to fp32), and the
    target_xy of IntegralL1Loss.  image_size / heatmap_size are (w, h)."""
    _need_cuda(joints)
    B, J = joints.shape[:2]
    xy = joints[..., :2].float().contiguous()
    out = torch.empty(B, J, 2, device=joints.device)
    lib().call('fami_heatmap_xy_f32', _p(xy), _p(out), B * J, int(heatmap_size[1]), int(heatmap_size[0]), int(image_size[1]),
               int(image_size[0]), _stream(joints))
    return out


class _IntegralL1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hm, txy, w, beta, scale):
        B, J, H, W = hm.shape
        coords, stats = _softargmax_fwd(hm, beta)
        out = torch.empty(1, device=hm.device)
        ws = torch.empty(B * J, device=hm.device)
        lib().call('fami_integral_l1_fwd_f32', _p(coords), _p(txy), _p(w), _p(out), B * J, H, W, float(scale), _p(ws),
                   _stream(hm))
        ctx.save_for_backward(hm, coords, stats, txy, w)
        ctx.beta, ctx.scale = beta, scale
        return out.reshape(())

    @staticmethod
    def backward(ctx, g):
        hm, coords, stats, txy, w = ctx.saved_tensors
        B, J, H, W = hm.shape
        d = torch.empty_like(hm)
        lib().call('fami_integral_l1_bwd_f32', _p(hm), _p(coords), _p(stats), _p(txy), _p(w), _p(d), B * J, H, W, ctx.beta,
                   float(ctx.scale), _p(g.reshape(1).float().contiguous()), 0, _stream(hm))
        return d, None, None, None, None


class IntegralL1Loss(nn.Module):
    """Integral pose regression (Sun et al., ECCV 2018), the coordinate term the reference's train loop constructs
    (alignment_mi_function_term6_1.py:61-69; its file was never released, so the definition is this project's, include/fami.h):
    (1 / (B J)) sum_bj w_bj (|cx - tx| / W + |cy - ty| / H) with (cx, cy) = soft_argmax(output, beta) and target_xy [B,J,2]
    the joint in HEATMAP pixels (joint / feature stride).  The gradient reaches `output` only."""

    def __init__(self, beta=20.0, use_target_weight=True):
        super().__init__()
        _, self.beta = check_integral_options(1.0, beta)
        self.use_target_weight = use_target_weight

    def forward(self, output, target_xy, target_weight):
        _need_cuda(output)
        B, J = output.shape[:2]
        w = target_weight.reshape(B * J).float().contiguous() if self.use_target_weight else None
        txy = target_xy.detach().reshape(B * J, 2).float().contiguous()
        return _IntegralL1.apply(output.float().contiguous(), txy, w, self.beta, 1.0 / (B * J))


def integral_get_final_preds(batch_heatmaps, center, scale, beta=20.0):
    """The integral decode: the soft-argmax of every map (soft_argmax; no blur, no Newton step) through the inverse affine of
    get_final_preds -- one launch (fami_softargmax_preds_f32).  maxvals, and every joint the standard decode masks
    (maximum <= 0 or NaN), are bit for bit get_final_preds'.  Same conventions: heatmaps [B,J,H,W] (device), center /
    scale [B,2] -> (preds [B,J,2] image coordinates, maxvals [B,J,1]) as device tensors.
    The expectation runs over the WHOLE map: a peak near a border, whose tail the map cuts off, is pulled inward (up to
    0.29 px for a sigma-3 target at beta = 20), and mass elsewhere in the map pulls toward it."""
    _, beta = check_integral_options(1.0, beta)
    _need_cuda(batch_heatmaps)
    B, J, H, W = batch_heatmaps.shape
    dev = batch_heatmaps.device
    c = torch.as_tensor(center, dtype=torch.float32, device=dev).reshape(B, 2).contiguous()
    sc = torch.as_tensor(scale, dtype=torch.float32, device=dev).reshape(B, 2).contiguous()
    preds = torch.empty(B, J, 2, device=dev)
    mx = torch.empty(B, J, device=dev)
    lib().call('fami_softargmax_preds_f32', _p(batch_heatmaps.float().contiguous()), _p(c), _p(sc), beta, _p(preds), _p(mx),
               B, J, H, W, _stream(batch_heatmaps))
    return preds, mx.unsqueeze(-1)


STRUCTURE_MAX = 64      # limbs and joints per sample the structure kernels take (csrc/loss.hip STRUCT_MAX)


def check_structure_options(weight, pairs, min_len, eps, num_joints=None):
    """-> (float(weight), pairs as a tuple of (a, b) int tuples, float(min_len), float(eps)), or ValueError -- host arithmetic
    only, before anything is uploaded.  weight: a finite number > 0 (the factor of the structure term); pairs: 1..64 limbs
    (a, b) of integer joint indices with a != b, inside 0..num_joints-1 where num_joints (2..64) is known; min_len: finite, >= 0,
    in heatmap pixels; eps: finite, > 0.  min_len and eps must be finite in fp32 (eps also non-zero there)."""
    for name, v in (('weight', weight), ('min_len', min_len), ('eps', eps)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
            raise ValueError('structure cosine %s is a finite number, not %r' % (name, v))
    f32max = float(np.finfo(np.float32).max)
    if not weight > 0:
        raise ValueError('structure cosine weight must be > 0 (None switches the term off), got %r' % (weight,))
    if not 0 <= min_len <= f32max:
        raise ValueError('structure cosine min_len must be >= 0 and finite in fp32, got %r' % (min_len,))
    if not (0 < eps <= f32max and float(np.float32(eps)) > 0):
        raise ValueError('structure cosine eps must be > 0 and finite in fp32, got %r' % (eps,))
    if num_joints is not None and not 2 <= num_joints <= STRUCTURE_MAX:
        raise ValueError('the structure cosine term takes 2..%d joints, got %r' % (STRUCTURE_MAX, num_joints))
    try:
        rows = [tuple(p) for p in pairs]
    except TypeError:
        raise ValueError('structure cosine pairs is a sequence of (a, b) joint indices, not %r' % (pairs,))
    if not 1 <= len(rows) <= STRUCTURE_MAX:
        raise ValueError('the structure cosine term takes 1..%d limbs, got %d' % (STRUCTURE_MAX, len(rows)))
    out = []
    for p in rows:
        if len(p) != 2 or any(isinstance(i, bool) or not isinstance(i, (int, np.integer)) for i in p):
            raise ValueError('a limb is a pair (a, b) of integer joint indices, got %r' % (p,))
        a, b = int(p[0]), int(p[1])
        hi = (STRUCTURE_MAX if num_joints is None else num_joints) - 1
        if not (0 <= a <= hi and 0 <= b <= hi):
            raise ValueError('limb %r: joint indices lie in 0..%d' % (p, hi))
        if a == b:
            raise ValueError('limb %r joins a joint to itself' % (p,))
        out.append((a, b))
    return float(weight), tuple(out), float(min_len), float(eps)


_PAIRS_CACHE = {}


def _pairs_on(dev, pairs):
    """a checked pair table as an int32 device tensor [P,2]; one upload per (device, table)."""
    key = (str(dev), pairs)
    t = _PAIRS_CACHE.get(key)
    if t is None:
        t = _PAIRS_CACHE[key] = torch.tensor(pairs, dtype=torch.int32).reshape(-1, 2).to(dev)
    return t


def _structure_rows(coords, txy, w, pairs_t, B, J, min_len, eps, scale):
    """-> (loss [1], row values [B*P]): fami_structure_cos_fwd_f32 on contiguous fp32 device tensors"""
    P = pairs_t.shape[0]
    out = torch.empty(1, device=coords.device)
    rows = torch.empty(B * P, device=coords.device)
    lib().call('fami_structure_cos_fwd_f32', _p(coords), _p(txy), _p(w), _p(pairs_t), _p(out), B, J, P, min_len, eps,
               float(scale), _p(rows), _stream(coords))
    return out, rows


class _StructureCos(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hm, txy, w, pairs_t, beta, min_len, eps, scale):
        B, J = hm.shape[:2]
        coords, stats = _softargmax_fwd(hm, beta)
        out, _ = _structure_rows(coords, txy, w, pairs_t, B, J, min_len, eps, scale)
        ctx.save_for_backward(hm, coords, stats, txy, w, pairs_t)
        ctx.opts = (beta, min_len, eps, scale)
        return out.reshape(())

    @staticmethod
    def backward(ctx, g):
        hm, coords, stats, txy, w, pairs_t = ctx.saved_tensors
        beta, min_len, eps, scale = ctx.opts
        B, J, H, W = hm.shape
        gcoords = torch.empty(B * J, 2, device=hm.device)
        d = torch.empty_like(hm)
        lib().call('fami_structure_cos_bwd_f32', _p(coords), _p(txy), _p(w), _p(pairs_t), _p(gcoords), B, J, pairs_t.shape[0],
                   min_len, eps, float(scale), _p(g.reshape(1).float().contiguous()), _stream(hm))
        lib().call('fami_softargmax_bwd_f32', _p(hm), _p(coords), _p(stats), _p(gcoords), _p(d), B * J, H, W, beta, 0, _stream(hm))
        return d, None, None, None, None, None, None, None


class StructureCosineSimilarity(nn.Module):
    """The structure term the reference's train loop constructs beside JointMSELoss and IntegralL1Loss
    (alignment_mi_function_term6_1.py:60-70; its file was never released, so the definition is this project's, include/fami.h):
    (1 / (B P)) sum_bp valid_bp (1 - cos(c[b_p] - c[a_p], t[b_p] - t[a_p])) with c = soft_argmax(output, beta), t = target_xy
    [B,J,2] in HEATMAP pixels and pairs the P limbs (a, b).  A limb counts (valid) when both its joints have a target weight
    > 0 and its target is longer than min_len pixels; the denominator stays B P.  min_len = 1.0 is a starting value, not
    tuned on data.  The gradient reaches `output` only, through fami_structure_cos_bwd_f32 and fami_softargmax_bwd_f32."""

    def __init__(self, pairs=LIMB_PAIRS, beta=20.0, min_len=1.0, eps=1e-8, use_target_weight=True):
        super().__init__()
        _, self.beta = check_integral_options(1.0, beta)
        _, self.pairs, self.min_len, self.eps = check_structure_options(1.0, pairs, min_len, eps)
        self.use_target_weight = use_target_weight

    def forward(self, output, target_xy, target_weight):
        _need_cuda(output)
        B, J = output.shape[:2]
        check_structure_options(1.0, self.pairs, self.min_len, self.eps, J)
        w = target_weight.reshape(B * J).float().contiguous() if self.use_target_weight else None
        txy = target_xy.detach().reshape(B * J, 2).float().contiguous()
        return _StructureCos.apply(output.float().contiguous(), txy, w, _pairs_on(output.device, self.pairs), self.beta,
                                   self.min_len, self.eps, 1.0 / (B * len(self.pairs)))


def limb_cosines(coords, target_xy, w, pairs=LIMB_PAIRS, min_len=1.0, eps=1e-8):
    """The cosine of every limb, for logging: coords / target_xy [B,J,2] (device, heatmap pixels), w [B,J] or [B,J,1] target
    weights or None -> [B,P] fp32 on the device, NaN where the limb is not valid.  The values are 1 - the rows of
    fami_structure_cos_fwd_f32; which limbs are valid is restated here with tensor operations."""
    _need_cuda(coords)
    B, J = coords.shape[:2]
    _, pairs, min_len, eps = check_structure_options(1.0, pairs, min_len, eps, J)
    c = coords.detach().reshape(B * J, 2).float().contiguous()
    t = target_xy.detach().reshape(B * J, 2).float().contiguous()
    wv = None if w is None else w.detach().reshape(B * J).float().contiguous()
    pt = _pairs_on(coords.device, pairs)
    _, rows = _structure_rows(c, t, wv, pt, B, J, min_len, eps, 1.0)
    a, b = pt[:, 0].long(), pt[:, 1].long()
    td = t.reshape(B, J, 2).double()
    d = td[:, b] - td[:, a]
    valid = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] > float(np.float32(min_len)) ** 2
    if wv is not None:
        wb = wv.reshape(B, J)
        valid &= (wb[:, a] > 0) & (wb[:, b] > 0)
    return torch.where(valid, 1.0 - rows.reshape(B, len(pairs)), torch.full_like(rows, float('nan')).reshape(B, len(pairs)))


def accuracy(output, target, thr=0.5):
    """PCK on heatmap argmax (evaluate.py:39-75).  -> (acc[J+1], avg_acc, cnt, pred[B,J,2] ndarray)."""
    pred, _ = get_max_preds(output)
    tgt, _ = get_max_preds(target)
    pred, tgt = pred.cpu().numpy(), tgt.cpu().numpy()          # 2*B*J*2 floats cross the bus, not 2 heatmap stacks
    B, J = pred.shape[:2]
    h, w = output.shape[2], output.shape[3]
    norm = np.ones((B, 2)) * np.array([h, w]) / 10
    valid = (tgt[:, :, 0] > 1) & (tgt[:, :, 1] > 1)
    d = np.linalg.norm(pred.astype(np.float32) / norm[:, None, :] - tgt.astype(np.float32) / norm[:, None, :], axis=2)
    dists = np.where(valid, d, -1.0).T
    acc = np.zeros(J + 1)
    avg, cnt = 0.0, 0
    for c in range(J):
        use = dists[c] != -1
        acc[c + 1] = (dists[c][use] < thr).sum() * 1.0 / use.sum() if use.sum() > 0 else -1
        if acc[c + 1] >= 0:
            avg += acc[c + 1]
            cnt += 1
    avg = avg / cnt if cnt != 0 else 0
    if cnt != 0:
        acc[0] = avg
    return acc, avg, cnt, pred
