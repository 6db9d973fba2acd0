"""Input pipeline on the device: what the reference's DataLoader workers do per clip with cv2 and
torchvision -- one affine crop shared by the key frame and its supporting frames, optional flip, ToTensor + Normalize,
joint transform, visibility rule (datasets/zoo/posetrack/PoseTrack_Alignment.py:380-440,
datasets/process/affine_transform.py:45-82, datasets/process/pose_process.py:12-26,
datasets/transforms/build.py:12-23) -- as host arithmetic on 2x3 matrices plus ONE kernel launch per clip
(`fami_warp_normalize_u8`, twice: key frame, supporting frames) or ONE per batch (`ClipBatcher`,
`fami_warp_normalize_batch_u8`).  crop_clip / prepare_clip / ClipBatcher.prepare are deterministic given the draws of
the augmentation (half body / scale / rotation / flip); `draw_augmentation` restates those draws in the reference's
order on generators the caller hands in.  HIP path only: there is no CPU fallback."""
import random

import numpy as np
import torch

from ._lib import lib

MEAN = (0.485, 0.456, 0.406)      # datasets/transforms/build.py:13-14 (RGB)
STD = (0.229, 0.224, 0.225)
FLIP_PAIRS = ((3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16))   # PoseTrack_Alignment.py:40
JOINTS_WEIGHT = (1., 1., 1., 1., 1., 1., 1., 1.2, 1.2, 1.5, 1.5, 1., 1., 1.2, 1.2, 1.5, 1.5)    # PoseTrack_Alignment.py:41-43
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
    transform for the joints.  center is the caller's (already flipped if flip, PoseTrack_Alignment.py:414)."""
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
    Per sample it does prepare_clip's host arithmetic (flip bookkeeping, dark_get_affine_transform, invert_affine,
    transform_joints), writes everything into the staging buffer, issues the copy and the launch on the current stream
    and returns (kf_x[:n], sup_x[:n], joints[:n], vis[:n], trans [n,2,3], center [n,2], scale [n,2]): four device views
    and three float64 numpy arrays; center is the one the transform used (mirrored where flip, the reference's
    meta['center']), and center / scale are what evaluate.predict takes.  The crops are bit for bit prepare_clip's.

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
                'sup_x': torch.zeros(B, 3 * (F - 1), H, W, device=self.device)}
        return self._bufs

    kf_x = property(lambda self: self._buffers()['kf_x'])
    sup_x = property(lambda self: self._buffers()['sup_x'])
    joints = property(lambda self: self._buffers()['joints'])
    vis = property(lambda self: self._buffers()['vis'])

    @staticmethod
    def _field(sample, name):
        return sample[name] if isinstance(sample, dict) else getattr(sample, name)

    def _check(self, clips):
        """Every refusal that needs no device, in an order that needs none either: counts, then kind and shape of the
        frames, then where they live -> per clip (Hs, Ws)."""
        if len(clips) < 1 or len(clips) > self.B:
            raise ValueError('ClipBatcher.prepare: %d samples for a batch of %d' % (len(clips), self.B))
        sizes = []
        for k, c in enumerate(clips):
            frames = self._field(c, 'frames')
            if len(frames) != self.F:
                raise ValueError('ClipBatcher.prepare: sample %d has %d frames, %d expected' % (k, len(frames), self.F))
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
        n, F, bufs = len(clips), self.F, self._buffers()
        for k, c in enumerate(clips):
            for f in self._field(c, 'frames'):
                if f.device != self.device:
                    raise RuntimeError('ClipBatcher.prepare: sample %d has a frame on %s, not %s' % (k, f.device, self.device))
        if self._copied is not None:
            self._copied.synchronize()           # the last copy has read the staging buffer
        # the table of THIS launch: n records, then n * F pointers (fami.h)
        h_clips = bufs['h_table'][:n * _CLIP_REC.itemsize].view(_CLIP_REC)
        h_ptrs = bufs['h_table'][n * _CLIP_REC.itemsize:n * (_CLIP_REC.itemsize + 8 * F)].view(np.uint64).reshape(n, F)
        trans_all, center_all, scale_all = np.zeros((n, 2, 3)), np.zeros((n, 2)), np.zeros((n, 2))
        for k, (c, (Hs, Ws)) in enumerate(zip(clips, sizes)):
            joints, joints_vis = self._field(c, 'joints'), self._field(c, 'joints_vis')
            flip = bool(self._field(c, 'flip'))
            center = np.asarray(self._field(c, 'center'), np.float64).copy()
            scale = self._field(c, 'scale')
            if flip:                                              # prepare_clip's bookkeeping
                joints, joints_vis = fliplr_joints(joints, joints_vis, Ws)
                center[0] = Ws - center[0] - 1
            trans = dark_get_affine_transform(center, scale, self._field(c, 'rot'), self.image_size)
            joints, joints_vis = transform_joints(joints, joints_vis, trans, self.image_size)
            h_clips[k] = (invert_affine(trans).reshape(6), int(flip), Hs, Ws, 0)
            h_ptrs[k] = [t.data_ptr() for t in self._field(c, 'frames')]
            bufs['h_joints'][k] = joints[:, :2]
            bufs['h_vis'][k] = joints_vis[:, 0]
            trans_all[k], center_all[k], scale_all[k] = trans, center, np.asarray(scale, np.float64)
        stream = torch.cuda.current_stream(self.device)
        bufs['dev'].copy_(bufs['host'], non_blocking=True)
        if self._copied is None:
            self._copied = torch.cuda.Event()
        self._copied.record(stream)
        W, H = self.image_size
        lib().call('fami_warp_normalize_batch_u8', bufs['dev'].data_ptr(), bufs['kf_x'].data_ptr(),
                   bufs['sup_x'].data_ptr() if F > 1 else None, n, F, H, W, int(self.bgr), *MEAN, *STD,
                   stream.cuda_stream)
        return (bufs['kf_x'][:n], bufs['sup_x'][:n], bufs['joints'][:n], bufs['vis'][:n], trans_all, center_all,
                scale_all)
