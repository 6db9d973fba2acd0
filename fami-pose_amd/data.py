"""Input pipeline on the device: what the reference's DataLoader workers do per clip with cv2 and
torchvision -- one affine crop shared by the key frame and its supporting frames, optional flip, ToTensor + Normalize,
joint transform, visibility rule (datasets/zoo/posetrack/PoseTrack_Alignment.py:380-440,
datasets/process/affine_transform.py:45-82, datasets/process/pose_process.py:12-26,
datasets/transforms/build.py:12-23) -- as host arithmetic on 2x3 matrices plus ONE kernel launch per clip
(`fami_warp_normalize_u8`, twice: key frame, supporting frames) or ONE per batch (`ClipBatcher`,
`fami_warp_normalize_batch_u8`).  crop_clip / prepare_clip / ClipBatcher.prepare are deterministic given the draws of
the augmentation (half body / scale / rotation / flip); `draw_augmentation` restates those draws in the reference's
order on generators the caller hands in.  Beyond the reference: `draw_degradation` draws occluders, a line blur and a
colour change per clip, which ClipBatcher applies to the 8-bit crop inside its one launch
(`fami_warp_degrade_batch_u8`; the rule is written out in include/fami.h).  HIP path only: there is no CPU fallback."""
import random

import numpy as np
import torch

from ._lib import lib

MEAN = (0.485, 0.456, 0.406)      # datasets/transforms/build.py:13-14 (RGB)
STD = (0.229, 0.224, 0.225)
FLIP_PAIRS = ((3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16))   # PoseTrack_Alignment.py:40
JOINTS_WEIGHT = (1., 1., 1., 1., 1., 1., 1., 1.2, 1.2, 1.5, 1.5, 1., 1., 1.2, 1.2, 1.5, 1.5)    # PoseTrack_Alignment.py:41-43
# The limbs (a, b) of the 17-joint PoseTrack order for loss.StructureCosineSimilarity.  This project's table (the reference's
# lives in a module it did not ship): head chain 2-0-1, neck to shoulders, the two arms, trunk, the two legs.  The ears (3, 4),
# which PoseTrack does not annotate, are on no limb; as undirected limbs the set is closed under FLIP_PAIRS.
LIMB_PAIRS = ((2, 0), (0, 1), (1, 5), (1, 6), (5, 6), (5, 7), (7, 9), (6, 8), (8, 10), (5, 11), (6, 12), (11, 12), (11, 13),
              (13, 15), (12, 14), (14, 16))
UPPER_BODY_IDS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10)                            # PoseTrack_Alignment.py:44
PIXEL_STD = 200                                                                # datasets/zoo/base.py:27


def _solve_affine(src, dst):
    """cv2.getAffineTransform: M with M @ [x, y, 1] = dst for three point pairs (float64)."""
    A = np.zeros((6, 6))
    b = np.zeros(6)
    for i in range(3):
        A[2 * i, 0:3] = (src[i, 0], src[i, 1], 1.0)
        A[2 * i + 1, 3:6] = (src[i, 0], src[i, 1], 1.0)
        b[2 * i], b[2 * i + 1] = dst[i, 0], dst[i, 1]
    return np.linalg.solve(A, b).reshape(2, 3)


def dark_get_affine_transform(center, scale, rot, output_size, inv=0):
    """affine_transform.py:45-77 (shift 0): image -> crop transform anchored on (w-1)/2 pixel centres."""
    scale = np.asarray(scale, np.float64)
    scale_tmp = scale * 200.0
    src_w = scale_tmp[0]
    dst_w, dst_h = output_size[0], output_size[1]
    rad = np.pi * rot / 180
    sn, cs = np.sin(rad), np.cos(rad)
    px, py = 0.0, (src_w - 1) * -0.5
    src_dir = np.array([px * cs - py * sn, px * sn + py * cs])
    dst_dir = np.array([0, (dst_w - 1) * -0.5], np.float32)
    src = np.zeros((3, 2), np.float32)
    dst = np.zeros((3, 2), np.float32)
    src[0, :] = center
    src[1, :] = np.asarray(center) + src_dir
    dst[0, :] = [(dst_w - 1) * 0.5, (dst_h - 1) * 0.5]
    dst[1, :] = np.array([(dst_w - 1) * 0.5, (dst_h - 1) * 0.5]) + dst_dir
    for pts in (src, dst):
        d = pts[0] - pts[1]
        pts[2, :] = pts[1] + np.array([-d[1], d[0]], np.float32)
    src, dst = src.astype(np.float64), dst.astype(np.float64)
    return _solve_affine(dst, src) if inv else _solve_affine(src, dst)


def invert_affine(M):
    """The dst -> src map cv2.warpAffine derives from the forward matrix (float64, cv2's operation order)."""
    M = np.asarray(M, np.float64).copy().reshape(6)
    D = M[0] * M[4] - M[1] * M[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = M[4] * D, M[0] * D
    M[0] = A11
    M[1] *= -D
    M[3] *= -D
    M[4] = A22
    b1 = -M[0] * M[2] - M[1] * M[5]
    b2 = -M[3] * M[2] - M[4] * M[5]
    M[2], M[5] = b1, b2
    return M.reshape(2, 3)


def fliplr_joints(joints, joints_vis, width, matched_parts=FLIP_PAIRS):
    """pose_process.py:12-26 on copies: mirror x, swap left/right joints, zero invisible joints."""
    joints, joints_vis = joints.copy(), joints_vis.copy()
    joints[:, 0] = width - joints[:, 0] - 1
    for a, b in matched_parts:
        joints[a, :], joints[b, :] = joints[b, :], joints[a, :].copy()
        joints_vis[a, :], joints_vis[b, :] = joints_vis[b, :], joints_vis[a, :].copy()
    return joints * joints_vis, joints_vis


def transform_joints(joints, joints_vis, trans, image_size):
    """PoseTrack_Alignment.py:434-443: visible joints through the crop transform (affine_transform.py:79-82); joints that
    leave [0, W] x [0, H] become invisible."""
    joints, joints_vis = joints.copy(), joints_vis.copy()
    for i in range(joints.shape[0]):
        if joints_vis[i, 0] > 0.0:
            joints[i, 0:2] = np.dot(trans, np.array([joints[i, 0], joints[i, 1], 1.0]).T)[:2]
    for i in range(joints.shape[0]):
        x, y = joints[i, 0], joints[i, 1]
        if x < 0 or y < 0 or x > image_size[0] or y > image_size[1]:
            joints_vis[i] = 0
    return joints, joints_vis


def crop_clip(frames_u8, center, scale, rot, image_size, flip=False, bgr=False, out_key=None, out_sup=None):
    """frames_u8: uint8 CUDA tensor [F, Hs, Ws, 3] (key frame first, then the supporting frames) of ONE clip.
    -> (key [3, H, W], sup [3*(F-1), H, W]) fp32 CUDA tensors: the reference's `input_x` and the channel-concatenated
    supporting frames, written into `out_key` / `out_sup` (e.g. slices of the batch tensors) when given; plus the 2x3
    transform for the joints.  center is the caller's (already flipped if flip, PoseTrack_Alignment.py:414).
    The per-clip path (this and prepare_clip) has no degradation: that is ClipBatcher's, in the batched launch."""
    if not (torch.is_tensor(frames_u8) and frames_u8.is_cuda and frames_u8.dtype == torch.uint8):
        raise RuntimeError('crop_clip: uint8 CUDA frames expected (HIP path only, no CPU fallback)')
    F, Hs, Ws, C = frames_u8.shape
    assert C == 3 and frames_u8.is_contiguous()
    W, H = int(image_size[0]), int(image_size[1])
    trans = dark_get_affine_transform(center, scale, rot, image_size)
    mi = invert_affine(trans)
    dev = frames_u8.device
    key = out_key if out_key is not None else torch.empty(3, H, W, device=dev)
    sup = out_sup if out_sup is not None else torch.empty(3 * (F - 1), H, W, device=dev)
    assert key.is_contiguous() and sup.is_contiguous() and key.dtype == torch.float32 and sup.dtype == torch.float32
    st = torch.cuda.current_stream(dev).cuda_stream
    L = lib()
    common = (float(mi[0, 0]), float(mi[0, 1]), float(mi[0, 2]), float(mi[1, 0]), float(mi[1, 1]), float(mi[1, 2]),
              int(bool(flip)), int(bool(bgr)), *MEAN, *STD, st)
    L.call('fami_warp_normalize_u8', frames_u8.data_ptr(), key.data_ptr(), 1, Hs, Ws, Hs * Ws * 3, H, W, 3 * H * W,
           *common)
    if F > 1:
        L.call('fami_warp_normalize_u8', frames_u8[1:].data_ptr(), sup.data_ptr(), F - 1, Hs, Ws, Hs * Ws * 3, H, W,
               3 * H * W, *common)
    return key, sup, trans


def prepare_clip(frames_u8, joints, joints_vis, center, scale, rot, image_size, flip=False, bgr=False,
                 out_key=None, out_sup=None):
    """One training sample as the reference's `__getitem__` builds it (after its random draws): flip bookkeeping for the
    joints and the centre, crop of every frame on the device, joints through the same transform.
    joints, joints_vis: [J, 3] numpy (image coordinates).  -> key, sup (device), joints [J,3], joints_vis [J,3] (numpy);
    feed joints[:, :2] / joints_vis[:, 0] to Trainer(targets_from_joints=True) for the on-device Gaussian targets."""
    center = np.asarray(center, np.float64).copy()
    if flip:
        Ws = frames_u8.shape[2]
        joints, joints_vis = fliplr_joints(joints, joints_vis, Ws)
        center[0] = Ws - center[0] - 1
    key, sup, trans = crop_clip(frames_u8, center, scale, rot, image_size, flip, bgr, out_key, out_sup)
    joints, joints_vis = transform_joints(joints, joints_vis, trans, image_size)
    return key, sup, joints, joints_vis


def half_body_transform(joints, joints_vis, num_joints, upper_body_ids, aspect_ratio, pixel_std, np_rng=np.random):
    """pose_process.py:45-81: the box of the visible upper- or lower-body joints -> (center [2], scale [2]), float32.
    Draws ONE np_rng.randn() -- `randn() < 0.5`, not rand(): the upper half is taken with probability ~0.69 when it has
    more than two visible joints; else the lower half if that has more than two, else the upper one.  Fewer than two
    selected joints -> (None, None).  The intermediate arrays are float32, as in the reference."""
    upper_joints, lower_joints = [], []
    for joint_id in range(num_joints):
        if joints_vis[joint_id][0] > 0:
            (upper_joints if joint_id in upper_body_ids else lower_joints).append(joints[joint_id])
    if np_rng.randn() < 0.5 and len(upper_joints) > 2:
        selected = upper_joints
    else:
        selected = lower_joints if len(lower_joints) > 2 else upper_joints
    if len(selected) < 2:
        return None, None
    selected = np.array(selected, dtype=np.float32)
    center = selected.mean(axis=0)[:2]
    left_top, right_bottom = np.amin(selected, axis=0), np.amax(selected, axis=0)
    w = right_bottom[0] - left_top[0]
    h = right_bottom[1] - left_top[1]
    if w > aspect_ratio * h:
        h = w * 1.0 / aspect_ratio
    elif w < aspect_ratio * h:
        w = h * aspect_ratio
    scale = np.array([w * 1.0 / pixel_std, h * 1.0 / pixel_std], dtype=np.float32)
    return center, scale * 1.5


def _augmentation_options(c):
    """cfg (TRAIN.* / MODEL.* as the reference's datasets/zoo/base.py:27-43 reads them) or a dict of keyword options
    -> the dict of keyword options.  A missing key is an error: no value is assumed."""
    if 'TRAIN' not in c:
        o = dict(c)
        o.setdefault('upper_body_ids', UPPER_BODY_IDS)
        o.setdefault('pixel_std', PIXEL_STD)
        return o
    t, m = c['TRAIN'], c['MODEL']
    return {'num_joints_half_body': t['NUM_JOINTS_HALF_BODY'], 'prob_half_body': t['PROB_HALF_BODY'],
            'scale_factor': t['SCALE_FACTOR'], 'rot_factor': t['ROT_FACTOR'], 'flip': t['FLIP'],
            'num_joints': m['NUM_JOINTS'], 'aspect_ratio': m['IMAGE_SIZE'][0] * 1.0 / m['IMAGE_SIZE'][1],
            'upper_body_ids': UPPER_BODY_IDS, 'pixel_std': PIXEL_STD}


def draw_augmentation(joints, joints_vis, center, scale, cfg_or_kwargs, np_rng=np.random, py_rng=random):
    """The random draws of one training sample, PoseTrack_Alignment.py:386-412 -> (center, scale, rot, flip) for
    prepare_clip / ClipBatcher.prepare.  cfg_or_kwargs: a cfg with TRAIN.NUM_JOINTS_HALF_BODY / PROB_HALF_BODY /
    SCALE_FACTOR / ROT_FACTOR / FLIP and MODEL.NUM_JOINTS / IMAGE_SIZE, or a dict with the keys num_joints_half_body,
    prob_half_body, scale_factor, rot_factor, flip, num_joints, aspect_ratio (and optionally upper_body_ids, pixel_std).
    The reference draws from TWO generators, numpy.random and Python's random, and short-circuit evaluation decides
    which draws happen; the consumption order below is normative (np_rng: anything with rand() / randn(), py_rng:
    anything with random()):
      1. np_rng.rand() ONLY IF sum(joints_vis[:, 0]) > NUM_JOINTS_HALF_BODY; if it is below PROB_HALF_BODY,
         half_body_transform follows, which draws one np_rng.randn() and replaces (center, scale).  A (None, None)
         result keeps the full box: the reference would crash there (`None * float` at :400), and with more than 8
         visible joints it cannot happen (one half then has more than two of them).
      2. one np_rng.randn() for the scale: scale * clip(randn * sf + 1, 1 - sf, 1 + sf); for a list or tuple sf is the
         FIRST element of TRAIN.SCALE_FACTOR.
      3. py_rng.random() <= 0.6 FIRST; np_rng.randn() for the rotation is drawn only if that holds (Python evaluates
         the condition of `a if c else b` before `a`): rot = clip(randn * rf, -2 rf, 2 rf), else 0.
      4. py_rng.random() <= 0.5 ONLY IF TRAIN.FLIP is on.
    The inputs are not modified: the reference mirrors `center` in place at :412, here the mirrored centre stays in
    prepare_clip / ClipBatcher.prepare, which take the unmirrored one together with `flip`."""
    o = _augmentation_options(cfg_or_kwargs)
    if np.sum(joints_vis[:, 0]) > o['num_joints_half_body'] and np_rng.rand() < o['prob_half_body']:
        c_half, s_half = half_body_transform(joints, joints_vis, o['num_joints'], o['upper_body_ids'],
                                             o['aspect_ratio'], o['pixel_std'], np_rng)
        if c_half is not None:
            center, scale = c_half, s_half
    sf, rf = o['scale_factor'], o['rot_factor']
    if isinstance(sf, (list, tuple)):
        sf = sf[0]
    scale = scale * np.clip(np_rng.randn() * sf + 1, 1 - sf, 1 + sf)
    rot = np.clip(np_rng.randn() * rf, -rf * 2, rf * 2) if py_rng.random() <= 0.6 else 0
    flip = bool(o['flip'] and py_rng.random() <= 0.5)
    return np.array(center), scale, rot, flip


_CLIP_REC = np.dtype([('m', np.float64, 6), ('flip', np.int32), ('Hs', np.int32), ('Ws', np.int32),
                      ('reserved', np.int32)])           # fami_warp_clip_t (include/fami.h)
_DEGRADE_RECT = np.dtype([('x0', np.int32), ('y0', np.int32), ('x1', np.int32), ('y1', np.int32), ('fill', np.uint8, 3),
                          ('mode', np.uint8)])           # fami_degrade_rect_t
_DEGRADE_REC = np.dtype([('flags', np.uint32), ('taps', np.int32), ('step_x', np.int32), ('step_y', np.int32),
                         ('alpha', np.float32), ('delta', np.float32), ('sat', np.float32), ('seed', np.uint32),
                         ('n_rect', np.int32), ('reserved', np.int32, 3), ('rect', _DEGRADE_RECT, 4)])   # fami_degrade_frame_t
DEGRADE_BLUR, DEGRADE_COLOUR, DEGRADE_OCCLUDE = 1, 2, 4  # FAMI_DEGRADE_*
MEAN_FILL = tuple(int(round(m * 255)) for m in MEAN)     # the 'mean' occluder: (124, 116, 104)

# Starting values, not tuned: no dataset was available to tune them on.
DEGRADE_DEFAULTS = {
    'photo_prob': 0.5, 'alpha_range': (0.7, 1.3), 'delta_range': (-25.0, 25.0), 'sat_range': (0.5, 1.5),
    'occlude_prob': 0.5, 'occlude_count': (1, 2), 'occlude_area': (0.02, 0.15), 'occlude_aspect': (0.5, 2.0),
    'occlude_frames': 'key', 'occlude_fill': 'mean',
    'blur_prob_key': 0.3, 'blur_prob_sup': 0.1, 'blur_length': (3.0, 15.0)}
_ALPHA_MAX, _DELTA_MAX, _SAT_MAX, _LENGTH_MAX, _RECT_MAX, _STEP_MAX = 8.0, 255.0, 8.0, 1024.0, 1 << 20, 1 << 24


def blur_taps(length):
    """The largest odd number <= min(15, length) (1 for a length below 3)."""
    n = int(min(15.0, np.floor(length)))
    return max(1, n if n % 2 else n - 1)


def blur_steps(taps, length, angle, mi):
    """A line blur of `length` crop pixels at `angle` degrees (0 = along x, 90 = along y of the crop), sampled by `taps`
    taps length / taps crop pixels apart, through the linear part of the clip's inverse transform `mi` (2x3, dst -> src)
    -> (step_x, step_y): the tap spacing in 1/1024 source pixel, the units of the kernel's fixed-point walk.
    ValueError when a tap would be displaced by 2^24 units or more (fami.h's bound)."""
    d = length / taps
    dx, dy = d * np.cos(np.pi * angle / 180), d * np.sin(np.pi * angle / 180)
    s = (1024.0 * (mi[0, 0] * dx + mi[0, 1] * dy), 1024.0 * (mi[1, 0] * dx + mi[1, 1] * dy))
    half = (taps - 1) // 2
    if not all(np.isfinite(v) and half * abs(np.rint(v)) < _STEP_MAX and abs(v) < _STEP_MAX for v in s):
        raise ValueError('degrade: blur step (%r, %r) x %d taps reaches 2^24 fixed-point units' % (s[0], s[1], taps))
    return int(np.rint(s[0])), int(np.rint(s[1]))


def _finite_in(name, v, lo, hi):
    v = float(v)
    if not (np.isfinite(v) and lo <= v <= hi):
        raise ValueError('degrade: %s = %r outside [%g, %g]' % (name, v, lo, hi))
    return v


def check_degradation(d, num_frames):
    """The refusals (ValueError) of a per-clip degradation dict, draw_degradation's result or a hand-made one:
      'colour'     None or (alpha, delta, sat): finite, alpha and sat in [0, 8], delta in [-255, 255]
      'blur'       None or num_frames entries, each None or (taps, length, angle): taps odd in 1..15, length in crop
                   pixels finite in (0, 1024], angle in degrees finite
      'occluders'  None or num_frames lists of at most 4 rectangles (x0, y0, x1, y1, fill): integers of magnitude
                   <= 2^20 in crop pixels, half-open, possibly empty or outside the crop; fill 'noise' or three bytes
      'seed'       0 .. 2^32 - 1 (the noise fill's)
    A missing key reads as None (seed: 0).  -> (colour, blur, occluders, seed) normalised to plain Python values."""
    if not isinstance(d, dict):
        raise ValueError('degrade: a dict or None expected, not %s' % type(d).__name__)
    unknown = set(d) - {'colour', 'blur', 'occluders', 'seed'}
    if unknown:
        raise ValueError('degrade: unknown keys %s' % sorted(unknown))
    F = int(num_frames)
    colour = d.get('colour')
    if colour is not None:
        if len(colour) != 3:
            raise ValueError('degrade: colour is (alpha, delta, sat)')
        colour = (_finite_in('alpha', colour[0], 0.0, _ALPHA_MAX), _finite_in('delta', colour[1], -_DELTA_MAX, _DELTA_MAX),
                  _finite_in('sat', colour[2], 0.0, _SAT_MAX))
    blur = d.get('blur')
    blur = [None] * F if blur is None else list(blur)
    if len(blur) != F:
        raise ValueError('degrade: %d blur entries for %d frames' % (len(blur), F))
    for f, b in enumerate(blur):
        if b is None:
            continue
        if len(b) != 3:
            raise ValueError('degrade: a blur entry is (taps, length, angle)')
        taps = b[0]
        if taps != int(taps) or not 1 <= int(taps) <= 15 or int(taps) % 2 == 0:
            raise ValueError('degrade: taps = %r: an odd number in 1..15 expected' % (taps,))
        length = _finite_in('blur length', b[1], 0.0, _LENGTH_MAX)
        if length <= 0.0:
            raise ValueError('degrade: blur length must be positive')
        blur[f] = (int(taps), length, _finite_in('blur angle', b[2], -1e6, 1e6))
    occ = d.get('occluders')
    occ = [[] for _ in range(F)] if occ is None else [list(o) if o is not None else [] for o in occ]
    if len(occ) != F:
        raise ValueError('degrade: %d occluder lists for %d frames' % (len(occ), F))
    for f, rects in enumerate(occ):
        if len(rects) > 4:
            raise ValueError('degrade: %d rectangles on frame %d, at most 4' % (len(rects), f))
        for q, r in enumerate(rects):
            if len(r) != 5:
                raise ValueError('degrade: a rectangle is (x0, y0, x1, y1, fill)')
            xy = []
            for v in r[:4]:
                if not np.isfinite(v) or v != int(v) or abs(int(v)) > _RECT_MAX:
                    raise ValueError('degrade: rectangle coordinate %r: an integer of magnitude <= 2^20 expected' % (v,))
                xy.append(int(v))
            fill = r[4]
            if not (isinstance(fill, str) and fill == 'noise'):
                if isinstance(fill, str) or len(fill) != 3 or any(v != int(v) or not 0 <= int(v) <= 255 for v in fill):
                    raise ValueError("degrade: fill %r: 'noise' or three bytes expected" % (fill,))
                fill = tuple(int(v) for v in fill)
            rects[q] = (*xy, fill)
    seed = d.get('seed', 0)
    if seed != int(seed) or not 0 <= int(seed) < 1 << 32:
        raise ValueError('degrade: seed %r outside 0 .. 2^32 - 1' % (seed,))
    return colour, blur, occ, int(seed)


def degrade_records(d, num_frames, mi, out=None):
    """A per-clip degradation dict (or None: every flag off) -> num_frames fami_degrade_frame_t records (structured
    numpy array, written into `out` when given).  mi: the clip's inverse transform, for the blur steps.  A stage that has
    nothing to do on a frame keeps its flag off (the kernel skips it): no colour, no blur entry, no rectangles."""
    F = int(num_frames)
    rec = np.zeros(F, _DEGRADE_REC) if out is None else out
    rec[...] = np.zeros((), _DEGRADE_REC)
    if d is None:
        return rec
    colour, blur, occ, seed = check_degradation(d, F)
    for f in range(F):
        flags = 0
        if blur[f] is not None:
            taps, length, angle = blur[f]
            rec[f]['taps'] = taps
            rec[f]['step_x'], rec[f]['step_y'] = blur_steps(taps, length, angle, mi)
            flags |= DEGRADE_BLUR
        if colour is not None:
            rec[f]['alpha'], rec[f]['delta'], rec[f]['sat'] = colour
            flags |= DEGRADE_COLOUR
        if occ[f]:
            rec[f]['n_rect'], rec[f]['seed'] = len(occ[f]), seed
            for q, (x0, y0, x1, y1, fill) in enumerate(occ[f]):
                noise = isinstance(fill, str)
                rec[f]['rect'][q] = (x0, y0, x1, y1, (0, 0, 0) if noise else fill, int(noise))
            flags |= DEGRADE_OCCLUDE
        rec[f]['flags'] = flags
    return rec


def _range_option(o, name, lo, hi, integer=False):
    r = o[name]
    if len(r) != 2:
        raise ValueError('draw_degradation: %s is a (low, high) pair' % name)
    a, b = (int(r[0]), int(r[1])) if integer else (float(r[0]), float(r[1]))
    if (integer and (a != r[0] or b != r[1])) or not (np.isfinite(a) and np.isfinite(b) and lo <= a <= b <= hi):
        raise ValueError('draw_degradation: %s = %r outside %g <= low <= high <= %g' % (name, tuple(r), lo, hi))
    return a, b


def draw_degradation(num_frames, image_size, options, rng, trans=None):
    """The random draws of one clip's degradation -> the per-clip dict ClipBatcher.prepare reads from a sample's
    optional `degrade` field (check_degradation documents it).  The reference has no such augmentation: rule and
    distributions are this project's, and the defaults (DEGRADE_DEFAULTS) are STARTING VALUES, not tuned -- no dataset
    was available.  Joints and visibilities are not touched: an occluded joint stays supervised, which is the point.

    options: a dict over DEGRADE_DEFAULTS (None: the defaults); an unknown key is an error.
      photo_prob; alpha_range, delta_range, sat_range   colour, with probability photo_prob, ONE draw per clip for all
                   its frames: t = u * alpha + delta, then saturation g + sat * (t - g) about the luma g (fami.h)
      occlude_prob; occlude_count (inclusive integers, high <= 4); occlude_area (fraction of the crop's area);
      occlude_aspect (width / height, drawn log-uniformly); occlude_frames 'key' (rectangles on the key frame only) |
                   'all' (the same rectangles on every frame) | 'independent' (count and rectangles drawn per frame);
                   occlude_fill 'mean' (the bytes of MEAN * 255 rounded) | 'noise'.  The centre of a rectangle is uniform
                   over the crop, so rectangles hang over its edges.
      blur_prob_key, blur_prob_sup; blur_length (crop pixels, low >= 1)   per frame; the angle is uniform in [0, 180)
                   degrees and taps = blur_taps(length), the largest odd number <= min(15, length)
    rng: a numpy.random.Generator or RandomState the caller hands in; only rng.uniform(low, high) is called, one scalar
    per call.  numpy.random's global state and Python's `random` are never touched, so draw_augmentation's order (the
    reference's) stays intact.  Consumption order, normative -- the same seeded generator gives the same dict:
      1. colour: u; if u < photo_prob: alpha, delta, sat.
      2. occluders: u; if u < occlude_prob: for the clip ('key', 'all') or for each frame in order ('independent'):
         count (floor of uniform(low, high + 1)), then per rectangle: area fraction, log aspect, centre x, centre y.
      3. seed: one uniform(0, 2^32), always.
      4. blur: for each frame, key first: u; if u < the frame's probability: length, angle.
    A u is drawn even where its probability is 0 or 1.
    trans: the clip's 2x3 crop transform, if known: the blur steps are then checked against fami.h's bound here
    (ValueError) and not only in ClipBatcher.prepare, which always derives them from the sample's own transform.
    Refusals (ValueError): probabilities outside [0, 1], non-finite or out-of-range ranges, a count above 4, unknown
    modes or keys; and check_degradation's on the result."""
    o = dict(DEGRADE_DEFAULTS)
    unknown = set(options or {}) - set(o)
    if unknown:
        raise ValueError('draw_degradation: unknown options %s' % sorted(unknown))
    o.update(options or {})
    F, (W, H) = int(num_frames), (int(image_size[0]), int(image_size[1]))
    if F < 1 or W < 1 or H < 1:
        raise ValueError('draw_degradation: num_frames and image_size must be >= 1')
    for name in ('photo_prob', 'occlude_prob', 'blur_prob_key', 'blur_prob_sup'):
        p = float(o[name])
        if not (np.isfinite(p) and 0.0 <= p <= 1.0):
            raise ValueError('draw_degradation: %s = %r outside [0, 1]' % (name, o[name]))
    alpha_r = _range_option(o, 'alpha_range', 0.0, _ALPHA_MAX)
    delta_r = _range_option(o, 'delta_range', -_DELTA_MAX, _DELTA_MAX)
    sat_r = _range_option(o, 'sat_range', 0.0, _SAT_MAX)
    count_r = _range_option(o, 'occlude_count', 0, 4, integer=True)
    area_r = _range_option(o, 'occlude_area', 0.0, 1.0)
    aspect_r = _range_option(o, 'occlude_aspect', 1.0 / 64, 64.0)
    length_r = _range_option(o, 'blur_length', 1.0, _LENGTH_MAX)
    if o['occlude_frames'] not in ('key', 'all', 'independent'):
        raise ValueError("draw_degradation: occlude_frames %r: 'key', 'all' or 'independent'" % (o['occlude_frames'],))
    if o['occlude_fill'] not in ('mean', 'noise'):
        raise ValueError("draw_degradation: occlude_fill %r: 'mean' or 'noise'" % (o['occlude_fill'],))
    fill = MEAN_FILL if o['occlude_fill'] == 'mean' else 'noise'

    def u(lo=0.0, hi=1.0):
        return float(rng.uniform(lo, hi))

    def rectangles():
        rects = []
        for _ in range(min(int(np.floor(u(count_r[0], count_r[1] + 1))), count_r[1])):
            area = u(*area_r) * W * H
            aspect = float(np.exp(u(np.log(aspect_r[0]), np.log(aspect_r[1]))))
            cx, cy = u(0.0, W), u(0.0, H)
            w, h = max(1, int(round(np.sqrt(area * aspect)))), max(1, int(round(np.sqrt(area / aspect))))
            x0, y0 = int(np.floor(cx - w / 2)), int(np.floor(cy - h / 2))
            rects.append((x0, y0, x0 + w, y0 + h, fill))
        return rects

    colour = None
    if u() < o['photo_prob']:
        colour = (u(*alpha_r), u(*delta_r), u(*sat_r))
    occ = [[] for _ in range(F)]
    if u() < o['occlude_prob']:
        if o['occlude_frames'] == 'independent':
            occ = [rectangles() for _ in range(F)]
        else:
            rects = rectangles()
            occ = [list(rects) if f == 0 or o['occlude_frames'] == 'all' else [] for f in range(F)]
    seed = min(int(u(0.0, 4294967296.0)), 4294967295)
    blur = [None] * F
    for f in range(F):
        if u() < (o['blur_prob_key'] if f == 0 else o['blur_prob_sup']):
            length, angle = u(*length_r), u(0.0, 180.0)
            blur[f] = (blur_taps(length), length, angle)
    d = {'colour': colour, 'blur': blur, 'occluders': occ, 'seed': seed}
    check_degradation(d, F)
    if trans is not None:
        mi = invert_affine(trans)
        for b in blur:
            if b is not None:
                blur_steps(b[0], b[1], b[2], mi)
    return d


class ClipBatcher:
    """A minibatch of annotated persons -> the tensors Trainer(targets_from_joints=True).step takes, with ONE async
    host-to-device copy and ONE kernel launch (fami_warp_normalize_batch_u8) per batch instead of 2 B launches, 2 B
    ctypes calls and a copy per joints array.

    Owns the batch tensors kf_x [B,3,H,W], sup_x [B,3S,H,W] (S = num_frames - 1), joints [B,J,2], vis [B,J] (fp32,
    device), one pinned host staging buffer and its device twin: the descriptor table of the launch (fami.h) followed
    by the joints and the visibilities; `joints` and `vis` are views of the device twin.

    prepare(clips): clips is a list of n <= B samples, each a dict (or object with these attributes) holding
      frames      list of num_frames uint8 device tensors [Hs,Ws,3], contiguous, key frame first; all frames of one
                  clip have one size, clips may differ; the same tensor may appear in many samples (evaluation: many
                  person boxes on the same five frames)
      joints, joints_vis   [J,3] numpy, image coordinates
      center, scale, rot, flip   after the draws (draw_augmentation); center is the UNMIRRORED one, as for prepare_clip
      degrade     OPTIONAL: the per-clip dict of draw_degradation / check_degradation, or None
    Per sample it does prepare_clip's host arithmetic (flip bookkeeping, dark_get_affine_transform, invert_affine,
    transform_joints), writes everything into the staging buffer, issues the copy and the launch on the current stream
    and returns (kf_x[:n], sup_x[:n], joints[:n], vis[:n], trans [n,2,3], center [n,2], scale [n,2]): four device views
    and three float64 numpy arrays; center is the one the transform used (mirrored where flip, the reference's
    meta['center']), and center / scale are what evaluate.predict takes.  The crops are bit for bit prepare_clip's.

    Degradation: if NO sample of the batch carries `degrade`, prepare issues exactly the copy and the launch above, and
    nothing is ever allocated for it.  Otherwise one fami_degrade_frame_t per (sample, frame) goes into the same staging
    buffer behind the joints (still one copy; the buffer grows once, at the first such batch), samples without the field
    get all-flags-off records, the blur steps come from the sample's own inverse transform (blur_steps), and
    fami_warp_degrade_batch_u8 runs in place of the plain launch.  The return tuple is the same; joints and
    visibilities are NOT touched by occluders.  The per-clip path (crop_clip / prepare_clip) stays as it is.

    Rows n.. of the four batch tensors are left alone when n < B.  (joints / vis: the staging buffer mirrors its device
    twin and is copied whole, so those rows keep what the batcher last put there.)

    The staging buffer is reused: an event is recorded behind the copy and the next prepare waits for it on the host
    before it overwrites the buffer.  Nothing else synchronises: the returned views are overwritten by the next
    prepare, in stream order; and the CALLER keeps the source frames alive (and unchanged) until the stream has passed
    the launch.  Use one batcher from one stream."""

    def __init__(self, batch_size, num_frames, image_size, num_joints=17, bgr=False, device='cuda'):
        B, F, J = int(batch_size), int(num_frames), int(num_joints)
        if B < 1 or F < 1 or J < 1:
            raise ValueError('ClipBatcher: batch_size, num_frames and num_joints must be >= 1')
        self.B, self.F, self.J, self.bgr = B, F, J, bool(bgr)
        self.image_size = (int(image_size[0]), int(image_size[1]))
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('ClipBatcher: a CUDA device expected (HIP path only, no CPU fallback)')
        self._table_bytes = lib().call('fami_warp_batch_table_bytes', B, F)
        if self._table_bytes != B * _CLIP_REC.itemsize + 8 * B * F:
            raise RuntimeError('fami_warp_clip_t layout differs between data.py and libfami_hip.so')
        self._degrade_bytes = lib().call('fami_degrade_table_bytes', B, F)
        if self._degrade_bytes != B * F * _DEGRADE_REC.itemsize:
            raise RuntimeError('fami_degrade_frame_t layout differs between data.py and libfami_hip.so')
        self._bufs = None                        # allocated at the first use: constructing needs no device
        self._copied = None                      # event behind the last copy out of the staging buffer

    def _buffers(self):
        if self._bufs is None:
            B, F, J, (W, H) = self.B, self.F, self.J, self.image_size
            if self.device.index is None:
                self.device = torch.device('cuda', torch.cuda.current_device())
            o1 = self._table_bytes
            o2 = o1 + 4 * B * J * 2
            host = torch.zeros(o2 + 4 * B * J, dtype=torch.uint8).pin_memory()
            dev = torch.zeros(o2 + 4 * B * J, dtype=torch.uint8, device=self.device)
            h = host.numpy()
            self._bufs = {
                'host': host, 'dev': dev, 'h_table': h[:o1],
                'h_joints': h[o1:o2].view(np.float32).reshape(B, J, 2), 'h_vis': h[o2:].view(np.float32).reshape(B, J),
                'joints': dev[o1:o2].view(torch.float32).view(B, J, 2), 'vis': dev[o2:].view(torch.float32).view(B, J),
                'kf_x': torch.zeros(B, 3, H, W, device=self.device),
                'sup_x': torch.zeros(B, 3 * (F - 1), H, W, device=self.device), 'plain_bytes': o2 + 4 * B * J}
        return self._bufs

    def _degrade_buffers(self):
        """The staging buffer and its device twin grown ONCE, at the first batch that carries a `degrade` field, by the
        degradation table behind the joints and the visibilities (16-byte aligned), so that the upload stays one copy.
        The host contents move over; joints / vis become views of the new twin (views handed out before stay valid and
        keep their values, but are no longer written).  A batcher that never degrades never allocates this."""
        bufs = self._buffers()
        if 'h_degrade' not in bufs:
            if self._copied is not None:
                self._copied.synchronize()
            B, J = self.B, self.J
            o1, o3 = self._table_bytes, bufs['plain_bytes']
            o2, o4 = o1 + 4 * B * J * 2, (o3 + 15) // 16 * 16
            host = torch.zeros(o4 + self._degrade_bytes, dtype=torch.uint8).pin_memory()
            dev = torch.zeros(o4 + self._degrade_bytes, dtype=torch.uint8, device=self.device)
            host[:o3].copy_(bufs['host'])
            dev[:o3].copy_(bufs['dev'])
            h = host.numpy()
            bufs.update({
                'host': host, 'dev': dev, 'h_table': h[:o1],
                'h_joints': h[o1:o2].view(np.float32).reshape(B, J, 2), 'h_vis': h[o2:o3].view(np.float32).reshape(B, J),
                'joints': dev[o1:o2].view(torch.float32).view(B, J, 2), 'vis': dev[o2:o3].view(torch.float32).view(B, J),
                'h_degrade': h[o4:].view(_DEGRADE_REC).reshape(B, self.F), 'degrade_offset': o4})
        return bufs

    kf_x = property(lambda self: self._buffers()['kf_x'])
    sup_x = property(lambda self: self._buffers()['sup_x'])
    joints = property(lambda self: self._buffers()['joints'])
    vis = property(lambda self: self._buffers()['vis'])

    @staticmethod
    def _field(sample, name):
        return sample[name] if isinstance(sample, dict) else getattr(sample, name)

    @staticmethod
    def _degrade_of(sample):
        """the optional per-sample field `degrade`: a dict (check_degradation), or None / absent"""
        return sample.get('degrade') if isinstance(sample, dict) else getattr(sample, 'degrade', None)

    def _host_arithmetic(self, c, Hs, Ws):
        """prepare_clip's host side for one sample -> (trans, inverse, flip, center, scale, joints, joints_vis)"""
        joints, joints_vis = self._field(c, 'joints'), self._field(c, 'joints_vis')
        flip = bool(self._field(c, 'flip'))
        center = np.asarray(self._field(c, 'center'), np.float64).copy()
        scale = self._field(c, 'scale')
        if flip:                                              # prepare_clip's bookkeeping
            joints, joints_vis = fliplr_joints(joints, joints_vis, Ws)
            center[0] = Ws - center[0] - 1
        trans = dark_get_affine_transform(center, scale, self._field(c, 'rot'), self.image_size)
        joints, joints_vis = transform_joints(joints, joints_vis, trans, self.image_size)
        return trans, invert_affine(trans), flip, center, np.asarray(scale, np.float64), joints, joints_vis

    def _check(self, clips):
        """Every refusal that needs no device, in an order that needs none either: counts (and the values of a `degrade`
        field), then kind and shape of the frames, then where they live -> per clip (Hs, Ws)."""
        if len(clips) < 1 or len(clips) > self.B:
            raise ValueError('ClipBatcher.prepare: %d samples for a batch of %d' % (len(clips), self.B))
        sizes = []
        for k, c in enumerate(clips):
            frames = self._field(c, 'frames')
            if len(frames) != self.F:
                raise ValueError('ClipBatcher.prepare: sample %d has %d frames, %d expected' % (k, len(frames), self.F))
            if self._degrade_of(c) is not None:          # counts and values of the optional field, before any tensor
                check_degradation(self._degrade_of(c), self.F)
            for f in frames:
                if not (torch.is_tensor(f) and f.dtype == torch.uint8):
                    raise RuntimeError('ClipBatcher.prepare: sample %d: uint8 tensors expected' % k)
                if f.dim() != 3 or f.shape[2] != 3:
                    raise ValueError('ClipBatcher.prepare: sample %d: [Hs,Ws,3] frames expected' % k)
                if f.shape != frames[0].shape:
                    raise ValueError('ClipBatcher.prepare: sample %d mixes frame sizes %s and %s' %
                                     (k, tuple(frames[0].shape), tuple(f.shape)))
            Hs, Ws = int(frames[0].shape[0]), int(frames[0].shape[1])
            if not (0 < Hs < 32768 and 0 < Ws < 32768):
                raise ValueError('ClipBatcher.prepare: sample %d: frame size %dx%d outside 1..32767' % (k, Hs, Ws))
            for f in frames:
                if not f.is_cuda:
                    raise RuntimeError('ClipBatcher.prepare: uint8 CUDA frames expected (HIP path only, no CPU fallback)')
                if not f.is_contiguous() or f.data_ptr() == 0:
                    raise ValueError('ClipBatcher.prepare: sample %d: contiguous, non-empty frames expected' % k)
            sizes.append((Hs, Ws))
        return sizes

    def prepare(self, clips):
        sizes = self._check(clips)
        n, F = len(clips), self.F
        # host arithmetic first: its refusals (a blur step beyond fami.h's bound among them) need no device either
        pre = [self._host_arithmetic(c, Hs, Ws) for c, (Hs, Ws) in zip(clips, sizes)]
        degrade = [self._degrade_of(c) for c in clips]
        records = None
        if any(d is not None for d in degrade):
            records = [degrade_records(d, F, p[1]) for d, p in zip(degrade, pre)]
        bufs = self._buffers()
        for k, c in enumerate(clips):
            for f in self._field(c, 'frames'):
                if f.device != self.device:
                    raise RuntimeError('ClipBatcher.prepare: sample %d has a frame on %s, not %s' % (k, f.device, self.device))
        if records is not None:
            bufs = self._degrade_buffers()
        if self._copied is not None:
            self._copied.synchronize()           # the last copy has read the staging buffer
        # the table of THIS launch: n records, then n * F pointers (fami.h)
        h_clips = bufs['h_table'][:n * _CLIP_REC.itemsize].view(_CLIP_REC)
        h_ptrs = bufs['h_table'][n * _CLIP_REC.itemsize:n * (_CLIP_REC.itemsize + 8 * F)].view(np.uint64).reshape(n, F)
        trans_all, center_all, scale_all = np.zeros((n, 2, 3)), np.zeros((n, 2)), np.zeros((n, 2))
        for k, (c, (Hs, Ws)) in enumerate(zip(clips, sizes)):
            trans, mi, flip, center, scale, joints, joints_vis = pre[k]
            h_clips[k] = (mi.reshape(6), int(flip), Hs, Ws, 0)
            h_ptrs[k] = [t.data_ptr() for t in self._field(c, 'frames')]
            bufs['h_joints'][k] = joints[:, :2]
            bufs['h_vis'][k] = joints_vis[:, 0]
            trans_all[k], center_all[k], scale_all[k] = trans, center, scale
            if records is not None:              # samples without the field: all-flags-off records
                bufs['h_degrade'][k] = records[k]
        stream = torch.cuda.current_stream(self.device)
        W, H = self.image_size
        out = (bufs['kf_x'].data_ptr(), bufs['sup_x'].data_ptr() if F > 1 else None, n, F, H, W, int(self.bgr), *MEAN, *STD,
               stream.cuda_stream)
        if records is None and 'h_degrade' in bufs:      # a plain batch after a degraded one: today's bytes only
            bufs['dev'][:bufs['plain_bytes']].copy_(bufs['host'][:bufs['plain_bytes']], non_blocking=True)
        else:
            bufs['dev'].copy_(bufs['host'], non_blocking=True)
        if self._copied is None:
            self._copied = torch.cuda.Event()
        self._copied.record(stream)
        if records is None:
            lib().call('fami_warp_normalize_batch_u8', bufs['dev'].data_ptr(), *out)
        else:
            lib().call('fami_warp_degrade_batch_u8', bufs['dev'].data_ptr(),
                       bufs['dev'].data_ptr() + bufs['degrade_offset'], *out)
        return (bufs['kf_x'][:n], bufs['sup_x'][:n], bufs['joints'][:n], bufs['vis'][:n], trans_all, center_all,
                scale_all)
