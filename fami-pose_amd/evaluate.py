"""Evaluation driver of the hot path.

* `predict` -- one inference step: what the reference's eval loop does per batch
  (engine/core/functions/alignment_mi_function_term6_1.py:256-276): `model(kf, sup) -> (pred, kf_bb)` under
  `torch.no_grad()`, then `get_final_preds(pred, center, scale)` -- with the decode on device, so only [B,J,2]
  coordinates and [B,J,1] confidences leave the GPU instead of two full heatmap stacks.
* `mirror_cat` / `flip_merge` / `flip_perm` -- flip testing, the protocol every HRNet-family number is reported with
  (the reference declares VAL.FLIP_VAL, TEST.FLIP_TEST and the two SHIFT_HEATMAP switches,
  posetimation/config/mppe_config.py:322-346, and ships `flip_back`, datasets/process/pose_process.py:29-42, but its
  released eval function never calls it): the clip and its horizontal mirror go through ONE forward as a doubled batch,
  the mirrored half's heatmaps are mirrored back with the left/right joint channels swapped, optionally shifted by one
  column, and averaged with the plain half -- one HIP launch per input in front of the forward and one per merged head
  behind it (csrc/flip.hip), nothing extra on the bus.  `predict(..., flip=True)` and `evaluate_loop(..., flip=True)` use it; `flip_test_options(cfg, phase)` reads the
  switches.  The doubled batch doubles the activation memory of the forward: halve VAL.BATCH_SIZE_PER_GPU /
  TEST.BATCH_SIZE_PER_GPU where that does not fit (there is no two-pass mode).
* `decode='dark'` on `predict` / `evaluate_loop` -- the distribution-aware decode the reference ships and exports
  (`dark_get_final_preds`, datasets/process/heatmaps_process.py:84-143; datasets/process/__init__.py:14) and that DARK-trained
  weights are meant to be read with: a `blur_kernel` x `blur_kernel` Gaussian blur of every map, log, one Newton step at the
  argmax -- one HIP launch per head (csrc/decode.hip, `loss.dark_get_final_preds`) in place of the quarter-pixel shift; with
  flip=True it runs on the merged maps.  The reference has no cfg switch for it, so there is none here; PCK stays on the
  argmax.  The default decode='standard' is `get_final_preds` as before.
* `EvalAccumulator` + `evaluate_loop` -- the loop around it (:222-328): per-batch PCK of both heatmap outputs (on
  device), `all_preds` / `all_bb` / `all_boxes` / `filenames_map` accumulation exactly as the reference lays them out.
* `pose_nms` / `EvalAccumulator.pose_nms` / `pose_nms_options` -- the third step of that protocol, between the loop and
  the writer: every detection is rescored by its keypoint confidences (box score x mean confidence of the joints above
  IN_VIS_THRE) and the duplicate poses of one frame are suppressed by object-keypoint-similarity NMS, hard
  (`oks_nms`) or soft (`soft_oks_nms`).  The reference ships the four functions (datasets/process/nms.py:51-192),
  declares VAL/TEST.IN_VIS_THRE, OKS_THRE and SOFT_NMS (mppe_config.py:325-330, 342-348), sets them in
  configs/Alignment/Base_PoseTrack17.yaml and reads them at PoseTrack_Alignment.py:68-72 -- and never uses the values.
  Here it is one upload, ONE launch for the whole validation set with one workgroup per frame (csrc/nms.hip,
  `fami_pose_nms_f32`) and one download; `all_boxes` already carries what it needs (column 4 the box area, column 5 the
  box score).  There is no "run NMS" switch in the reference, so there is none here: the step runs when it is called,
  and `evaluate_loop`, `predict` and `write_posetrack_results` are unchanged.  Box-IoU NMS (nms.py:9-48, NMS_THRE) is a
  detector-stage step and stays out.
* `pose_track` / `EvalAccumulator.pose_track` -- person identities, between `pose_nms` and the writer.  The reference declares
  EVAL_TRACKING / TRACKING_THRESHOLD (posetimation/config/defaults.py:34-36), carries `eval_tracking` through
  `convert_data_to_annorect_struct`, and writes track_id = position of the pose in its frame (PoseTrack_Alignment.py:998):
  it has no association rule, so the rule is this project's (include/fami.h): per video, frames by ascending frame
  number, every detection in list order takes the live track with the largest OKS (the arithmetic of `pose_nms`) if that
  exceeds oks_thre, else starts a new one; a track unseen for more than max_gap frame numbers is retired.  One upload, ONE
  launch with one workgroup per video (csrc/track.hip, `fami_pose_track_f32`), one download.  No cfg switch: the live
  config tree has no tracking key.  `write_posetrack_results(..., tracks=)` carries the ids into the JSON; with
  tracks=None it writes what it always wrote.
* `track_refine` / `EvalAccumulator.track_refine` -- the first consumer of those ids, between `pose_track` and the writer:
  gaps of at most max_fill frame numbers inside a track are filled by linear interpolation (new rows, new keys where a
  frame had none), x and y are filtered along the track with confidence-weighted Gaussian weights, box scores can become
  the track's mean, tracks shorter than min_len leave the lists.  The reference has no tracker and no such step: the rule
  is this project's (include/fami.h), its defaults starting values, not tuned.  One upload, at most three launches
  (csrc/track_refine.hip: fill, smooth, score), one download; with every stage off it returns copies and launches nothing.
* `write_posetrack_results` -- the PoseTrack JSON writer of
  datasets/zoo/posetrack/PoseTrack_Alignment.py:883-1017 (`evaluate` up to the poseval call): COCO->PoseTrack joint
  conversion (datasets/process/structure/keypoints_ord.py:14-73), the annorect structure
  (datasets/process/structure/data_format.py:12-49), empty frames filled in, one `{'annolist': [...]}` file per video
  named after the annotation file (posetrack_utils.py:13-56).

* `pack_posetrack_frames` / `load_posetrack_dirs` / `posetrack_ap` / `evaluate_posetrack_ap` -- the pose half of the
  vendored poseval (`evaluate_simple.evaluate(gt_dir, pred_dir, eval_track=False)`, posetrack_utils/poseval/py/
  evaluate_simple.py:13-50): per frame the greedy PCKh matching of predicted to annotated poses (assignGTmulti,
  eval_helpers.py:453-668), per joint one precision / recall curve over the set and its VOC AP (computeRPC / VOCap
  :192-228, computeMetrics evaluateAP.py:8-47), the summary row of getCum (:133-147).  In-process, in fp64 on the device:
  one workgroup per frame for the matching and one per joint for the curve (csrc/posetrack_ap.hip), a stable
  `torch.sort` between them; one upload, one download.  The ignore-region point filter, for which the reference needs
  shapely, is an even-odd crossing test in the first kernel.  The files `write_posetrack_results` wrote are its input.

* `posetrack_mota` / `evaluate_posetrack_mota` / `evaluate_posetrack` -- the tracking half of the same tool
  (`evaluate_simple.evaluate(gt_dir, pred_dir)[1]`; evaluateTracking.py:13-222, the `mot` lists of assignGTmulti,
  py-motmetrics/motmetrics/mot.py:90-229 MOTAccumulator.update, the counts of metrics.py:196-218): per sequence and joint
  one accumulator that remembers which predicted track every annotated track was matched to, per frame a carry-forward
  step and a minimum-cost assignment, MISS / SWITCH / FP / MATCH counts, MOTA / MOTP / Prec / Rec.  On the device, one
  wavefront per (sequence, joint) (csrc/posetrack_mot.hip), on the masks the AP's assign launch filtered; it scores the
  ids `pose_track` writes.  `evaluate_posetrack` runs both halves on one pack, one upload and one assign launch.

* `pack_coco_keypoints` / `coco_keypoint_ap` / `load_coco_keypoints` / `evaluate_coco_keypoints` /
  `coco_keypoint_results` / `EvalAccumulator.coco_results` -- the fourth step of the HRNet protocol, the number it reports:
  pycocotools' `COCOeval(gt, dt, 'keypoints')` (AP, AP50, AP75, AP-medium, AP-large and the five ARs) for one category.
  pycocotools is no part of the reference tree (oracle/ref_harness.py stubs it), so include/fami.h restates the definition
  in full.  In-process, in fp64 on the device: one workgroup per image ranks and cuts the detections, fills the OKS matrix
  and runs the 30 greedy walks (10 thresholds x 3 area ranges); one workgroup per (range, threshold) reads the curve at the
  101 recall thresholds (csrc/coco_ap.hip); a stable `torch.sort` between them, one upload, one download.  It scores what
  `pose_nms` keeps by the similarity `pose_nms` uses.  Box / segm IoU types, several categories, COCOeval's `scores` and
  `evalImgs` and COCO dataset indexing are out of scope.

`_Words` is the one upload of all of these: a list of named fields -> ONE buffer of 4-byte words, pointers, views and the one
download.

Out of scope: motmetrics' other metrics (MT / ML, fragmentations), per-sequence metric files, motion models and
appearance re-identification, the PoseTrack18 `images` / `annotations` file layout (poseval's convert.py) and PCKh
(evaluatePCKh.py).

The reference imports its joint-name lists from modules that are missing from the released tree
(`datasets.zoo.coco`, `datasets.zoo.posetrack.pose_topology`, keypoints_ord.py:10-11); COCO_JOINT / POSETRACK_JOINT
below are the standard COCO-17 and PoseTrack-15 orders of DCPose / Detect-and-Track, which the README defers to.
"""
import json
import math
import os
import os.path as osp

import numpy as np
import torch

from ._lib import lib
from .data import FLIP_PAIRS
from .loss import (_need_cuda, _p, _stream, check_blur_kernel, check_integral_options, dark_get_final_preds,
                   get_final_preds, integral_get_final_preds)
from .zoo.registry import TEST_PHASE, VAL_PHASE

COCO_JOINT = ['nose', 'left_eye', 'right_eye', 'left_ear', 'right_ear', 'left_shoulder', 'right_shoulder',
              'left_elbow', 'right_elbow', 'left_wrist', 'right_wrist', 'left_hip', 'right_hip', 'left_knee',
              'right_knee', 'left_ankle', 'right_ankle']
# the per-joint OKS constants of COCO-17, datasets/process/nms.py:66-69 (float64, as the reference holds them)
COCO_SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
NMS_MAX_PER_IMAGE = 256         # csrc/nms.hip: one thread per detection of an image
NMS_MAX_JOINTS = 32             # ... and one mask bit per joint
AP_JOINTS = 15                  # csrc/posetrack_ap.hip: the PoseTrack joints, one mask bit each
AP_MAX_PRED = 256               # ... one thread per predicted pose of a frame
AP_MAX_GT = 64                  # ... the annotated poses of a frame are LDS-resident
AP_MAX_SET = 458752             # ... one label bit per predicted pose of the set in 56 KiB of LDS
AP_MIN_SCORE = -9999            # eval_helpers.MIN_SCORE: a predicted point without a score
REFINE_MAX = 16                 # csrc/track_refine.hip: the largest max_fill and smooth_radius (33 neighbour reads per thread)
MOT_MAX_TRACKS = 256            # csrc/posetrack_mot.hip: annotated tracks of a sequence (the map m is LDS-resident)
MOT_COUNTS = ('num_misses', 'num_switches', 'num_false_positives', 'num_detections', 'num_objects')
POSETRACK_JOINT = ['right_ankle', 'right_knee', 'right_hip', 'left_hip', 'left_knee', 'left_ankle', 'right_wrist',
                   'right_elbow', 'right_shoulder', 'left_shoulder', 'left_elbow', 'left_wrist', 'neck', 'nose',
                   'head_top']


# ---------------------------------------------------------------------------------------- host plumbing of the set kernels
class _Words:
    """The ONE buffer of 4-byte words a set kernel's arrays travel in: declared as an ordered list of fields
    (name, 'f32' | 'f64' | 'i32', shape[, host array or fill value]) -- zeros without the last --, laid out in that order with
    every f64 field on an even word (8-byte aligned), and uploaded once.  `ptr` is a field's device address, `view` its
    device-side tensor, `download` ONE copy to the host of everything from a field to the end.  The alignment rule holds for an
    EMPTY f64 field too: behind an odd word count it still costs a padding word."""
    TYPES = {'f32': (np.float32, torch.float32), 'f64': (np.float64, torch.float64), 'i32': (np.int32, torch.int32)}

    def __init__(self, dev, fields):
        self.fields, filled, words = {}, [], 0
        for name, dt, shape, *init in fields:
            shape = shape if isinstance(shape, tuple) else (int(shape),)
            at = words + (words & 1 if dt == 'f64' else 0)
            words = at + math.prod(shape) * (2 if dt == 'f64' else 1)
            self.fields[name] = (at, words, dt, shape)
            filled += [(name, init[0])] if init else []
        buf = np.zeros(words, dtype=np.int32)
        for name, init in filled:
            at, to, dt, _ = self.fields[name]
            buf[at:to].view(self.TYPES[dt][0])[:] = np.reshape(init, -1)
        self.d = torch.from_numpy(buf).to(dev)

    def ptr(self, name):
        return self.d.data_ptr() + 4 * self.fields[name][0]

    def view(self, name):
        at, to, dt, shape = self.fields[name]
        return self.d[at:to].view(self.TYPES[dt][1]).view(shape)

    def download(self, first):
        """-> {name: numpy array of the field's dtype and shape} for `first` and every field behind it (views of one array)"""
        names = list(self.fields)
        start = self.fields[first][0]
        out = self.d[start:].cpu().numpy()
        res = {}
        for name in names[names.index(first):]:
            at, to, dt, shape = self.fields[name]
            res[name] = out[at - start:to - start].view(self.TYPES[dt][0]).reshape(shape)
        return res


def _hip_device(who, device):
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise RuntimeError('%s runs on the HIP path only (device is %s)' % (who, dev))
    return dev


def _int_option(who, text, value, lo, hi, *names):
    """ValueError '<who>: <text % names>, got <value>' unless `value` is an integer (no bool) in lo .. hi"""
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or not lo <= value <= hi:
        raise ValueError('%s: %s, got %r' % (who, text % names, value))


def _sigmas(who, J, sigmas, holder, dtype):
    """The per-joint OKS constants as a flat `dtype` array: default COCO_SIGMAS for J = 17, else J finite positive values
    (judged after the rounding to `dtype`, which is what the kernel reads)."""
    if sigmas is None:
        if J != len(COCO_SIGMAS):
            raise ValueError('%s: COCO_SIGMAS has %d joints, %s has %d: pass sigmas' % (who, len(COCO_SIGMAS), holder, J))
        sigmas = COCO_SIGMAS
    sig = np.asarray(sigmas, dtype=np.float64).reshape(-1).astype(dtype)
    if sig.shape != (J,) or not np.isfinite(sig).all() or not (sig > 0).all():
        raise ValueError('%s: sigmas must be %d finite positive values' % (who, J))
    return sig


def _pose_set(who, preds, boxes, sigmas):
    """The pose set of `pose_nms` / `pose_track`: preds [N,J,3] and boxes [N,6] with J in range -> (preds, boxes, N, J, sigmas
    fp32 [J])."""
    preds, boxes, N, J = _pose_shapes(who, preds, boxes)
    return preds, boxes, N, J, _sigmas(who, J, sigmas, 'preds', np.float32)


def _pose_shapes(who, preds, boxes):
    """preds [N,J,3] and boxes [N,6] with J in range -> (preds, boxes, N, J)"""
    preds, boxes = np.asarray(preds), np.asarray(boxes)
    if preds.ndim != 3 or preds.shape[2] != 3 or boxes.ndim != 2 or boxes.shape[1] != 6 or boxes.shape[0] != preds.shape[0]:
        raise ValueError('%s expects preds [N,J,3] and boxes [N,6], got %s and %s' % (who, preds.shape, boxes.shape))
    N, J = preds.shape[:2]
    if not 1 <= J <= NMS_MAX_JOINTS:
        raise ValueError('%s: J = %d joints, supported 1 .. %d' % (who, J, NMS_MAX_JOINTS))
    return preds, boxes, N, J


def _fp32(who, what, *arrays):
    """`arrays` rounded to fp32 as they are uploaded (a value beyond fp32 becomes inf) -> list; ValueError if not finite then"""
    with np.errstate(over='ignore'):
        out = [np.ascontiguousarray(a, dtype=np.float32) for a in arrays]
    if not all(np.isfinite(a).all() for a in out):
        raise ValueError('%s: %s must be finite (in fp32)' % (who, what))
    return out


def _index_range(who, N, J):
    if N * J * 3 > 0x7fffffff:
        raise ValueError('%s: N * J * 3 = %d exceeds 2^31 - 1' % (who, N * J * 3))


def _ascends(seg, n):
    """seg [groups + 1] ascends from 0 to n?"""
    return len(seg) >= 2 and seg[0] == 0 and seg[-1] == n and not (np.diff(seg) < 0).any()


def _first_over(counts_a, cap_a, counts_b, cap_b):
    """-> the first group with more than cap_a of the one kind or more than cap_b of the other, None if there is none"""
    if counts_a.max() > cap_a or counts_b.max() > cap_b:
        return int(np.argmax((counts_a > cap_a) | (counts_b > cap_b)))
    return None


# ---------------------------------------------------------------------------------------- flip testing
def flip_perm(num_joints, pairs=FLIP_PAIRS):
    """-> list of J ints: perm[a] = b and perm[b] = a for every (a, b) of `pairs`, identity elsewhere (the channel
    exchange of flip_back, pose_process.py:37-40, as one gather)."""
    J = int(num_joints)
    perm = list(range(J))
    seen = set()
    for a, b in pairs:
        a, b = int(a), int(b)
        if not (0 <= a < J and 0 <= b < J):
            raise ValueError('flip pair (%d, %d) outside [0, %d)' % (a, b, J))
        if a == b:
            raise ValueError('flip pair (%d, %d) pairs a joint with itself' % (a, b))
        if a in seen or b in seen:
            raise ValueError('flip pair (%d, %d): a joint occurs twice' % (a, b))
        seen.update((a, b))
        perm[a], perm[b] = b, a
    return perm


_PERM_CACHE = {}


def _perm_on(dev, J, pairs):
    """flip_perm(J, pairs) as a device int32 tensor; one upload per (device, J, pairs)."""
    key = (str(dev), J, tuple((int(a), int(b)) for a, b in pairs))
    t = _PERM_CACHE.get(key)
    if t is None:
        t = _PERM_CACHE[key] = torch.tensor(flip_perm(J, key[2]), dtype=torch.int32, device=dev)
    return t


def mirror_cat(x):
    """x [B,C,H,W] (device) -> [2B,C,H,W] fp32: x, then x mirrored along W -- the doubled batch of a flip-test forward,
    one launch, values copied bit for bit."""
    _need_cuda(x)
    if x.dim() != 4:
        raise ValueError('mirror_cat expects [B,C,H,W], got %s' % (tuple(x.shape),))
    x = x.float().contiguous()
    B, C, H, W = x.shape
    out = torch.empty(2 * B, C, H, W, device=x.device)
    lib().call('fami_mirror_cat_f32', _p(x), _p(out), B * C * H, W, _stream(x))
    return out


def flip_merge(hm2, pairs=FLIP_PAIRS, shift=False):
    """hm2 [2B,J,H,W] (device): heatmaps of a clip batch, then of its mirror -> [B,J,H,W] =
    (hm2[:B] + flip_back(hm2[B:], pairs)) * 0.5; with `shift` the mirrored-back half moves one column to the right first
    (HRNet's SHIFT_HEATMAP: flipped[..., 1:] = flipped[..., :-1], column 0 keeps its value)."""
    _need_cuda(hm2)
    if hm2.dim() != 4 or hm2.shape[0] % 2:
        raise ValueError('flip_merge expects [2B,J,H,W], got %s' % (tuple(hm2.shape),))
    hm2 = hm2.float().contiguous()
    B, J, H, W = hm2.shape[0] // 2, hm2.shape[1], hm2.shape[2], hm2.shape[3]
    perm = _perm_on(hm2.device, J, pairs)
    out = torch.empty(B, J, H, W, device=hm2.device)
    lib().call('fami_flip_merge_f32', _p(hm2), _p(perm), _p(out), B, J, H, W, 1 if shift else 0, _stream(hm2))
    return out


def flip_test_options(cfg, phase):
    """-> {'flip': bool, 'shift_heatmap': bool} for `predict` / `evaluate_loop` from the reference's switches:
    VAL.FLIP_VAL / VAL.SHIFT_HEATMAP in the validation phase, TEST.FLIP_TEST / TEST.SHIFT_HEATMAP in the test phase
    (mppe_config.py:322,329,340,346); False where the node or the key is absent."""
    if phase == VAL_PHASE:
        node, key = 'VAL', 'FLIP_VAL'
    elif phase == TEST_PHASE:
        node, key = 'TEST', 'FLIP_TEST'
    else:
        raise ValueError('flip testing is an evaluation option: phase %r has none' % (phase,))
    sub = cfg.get(node) if hasattr(cfg, 'get') else None
    sub = sub if hasattr(sub, 'get') else {}
    return {'flip': bool(sub.get(key, False)), 'shift_heatmap': bool(sub.get('SHIFT_HEATMAP', False))}


def _flip_forward(model, kf_x, sup_x):
    """ONE forward on the doubled batch [x ; mirror(x)] (the channel-packed supporting frames mirror along W like any
    other channel).  Needs eval mode: with running statistics BatchNorm does not mix the two halves."""
    if model.training:
        raise RuntimeError('flip testing needs model.eval(): batch statistics would mix the clip and its mirror')
    return model(mirror_cat(kf_x), mirror_cat(sup_x))


def _decoder(decode, blur_kernel, integral_beta=20.0):
    """-> f(heatmaps, center, scale) for decode = 'standard' (get_final_preds: quarter-pixel shift), 'dark'
    (dark_get_final_preds with a blur_kernel x blur_kernel Gaussian) or 'integral' (integral_get_final_preds: the soft-argmax
    at integral_beta); ValueError for anything else, before any device work.  Each decode ignores the other's keyword."""
    if decode == 'standard':
        return get_final_preds
    if decode == 'dark':
        k = check_blur_kernel(blur_kernel)
        return lambda hm, center, scale: dark_get_final_preds(hm, center, scale, k)
    if decode == 'integral':
        _, beta = check_integral_options(1.0, integral_beta)
        return lambda hm, center, scale: integral_get_final_preds(hm, center, scale, beta)
    raise ValueError("decode must be 'standard', 'dark' or 'integral', got %r" % (decode,))


@torch.no_grad()
def predict(model, kf_x, sup_x, center, scale, flip=False, shift_heatmap=False, flip_pairs=FLIP_PAIRS, decode='standard',
            blur_kernel=11, integral_beta=20.0):
    """-> (preds [B,J,2] image coordinates, maxvals [B,J,1], final_hm [B,J,H/4,W/4]) as device tensors.
    `model` is a val/test-phase Alignment_V15 (2-tuple forward) or a train-phase one (3-tuple; MI terms ignored).
    flip=True: flip testing -- one forward on the doubled batch, final_hm is the merged map and the decode runs on it.
    decode='dark': the distribution-aware decode (blur_kernel: odd, 9..17) instead of the quarter-pixel shift.
    decode='integral': the soft-argmax of the map at integral_beta (loss.integral_get_final_preds)."""
    final_preds = _decoder(decode, blur_kernel, integral_beta)
    if flip:
        final_hm = flip_merge(_flip_forward(model, kf_x, sup_x)[0], flip_pairs, shift_heatmap)
        preds, maxvals = final_preds(final_hm, center, scale)
        return preds, maxvals, final_hm
    out = model(kf_x, sup_x)
    final_hm = out[0]
    preds, maxvals = final_preds(final_hm, center, scale)
    return preds, maxvals, final_hm


# ---------------------------------------------------------------------------------------- accumulation (core fn :236-309)
class EvalAccumulator:
    """The arrays the reference's eval loop fills batch by batch (core fn :238-247, :283-309)."""

    def __init__(self, num_samples, num_joints=17):
        self.all_preds = np.zeros((num_samples, num_joints, 3), dtype=np.float64)
        self.all_bb = np.zeros((num_samples, num_joints, 3), dtype=np.float64)
        self.all_boxes = np.zeros((num_samples, 6))
        self.filenames_map = {}
        self.image_path = []
        self.idx = 0
        self._counter = 0
        self.acc_sum = [0.0, 0.0]         # AverageMeter.update(avg_acc, cnt) of final_hm / kf_bb_hm (:266-270)
        self.acc_cnt = [0, 0]

    def add_images(self, names):
        for nm in names:                                        # :283-289
            self.filenames_map.setdefault(nm, []).append(self._counter)
            self._counter += 1
        self.image_path.extend(names)

    def add(self, pred_coord, pred_maxvals, bb_coord, bb_maxvals, center, scale, score, names):
        """One batch: decoded coordinates / confidences of final_hm and kf_bb_hm (host arrays), box meta."""
        n = len(names)
        self.add_images(names)
        i = self.idx
        self.all_preds[i:i + n, :, :2] = pred_coord             # :296-302
        self.all_preds[i:i + n, :, 2:3] = pred_maxvals
        self.all_bb[i:i + n, :, :2] = bb_coord
        self.all_bb[i:i + n, :, 2:3] = bb_maxvals
        center, scale = np.asarray(center), np.asarray(scale)
        self.all_boxes[i:i + n, 0:2] = center[:, 0:2]           # :304-307
        self.all_boxes[i:i + n, 2:4] = scale[:, 0:2]
        self.all_boxes[i:i + n, 4] = np.prod(scale * 200, 1)
        self.all_boxes[i:i + n, 5] = np.asarray(score)
        self.idx += n

    def add_accuracy(self, k, avg_acc, cnt):
        self.acc_sum[k] += avg_acc * cnt
        self.acc_cnt[k] += cnt

    def accuracy(self, k=0):
        return self.acc_sum[k] / self.acc_cnt[k] if self.acc_cnt[k] else 0.0

    def pose_nms(self, **kw):
        """Rescoring and OKS-NMS of everything accumulated so far (module-level `pose_nms`, same keywords) ->
        (boxes2, filenames_map2): a copy of all_boxes[:idx] with column 5 replaced by the rescored value, and
        filenames_map with each frame's list reduced to the kept detections in pick order -- the `boxes` and
        `filenames_map` arguments of `write_posetrack_results`.  The accumulator itself is not modified."""
        boxes2 = self.all_boxes[:self.idx].copy()
        scores, keep_map = pose_nms(self.all_preds[:self.idx], boxes2, self.filenames_map, **kw)
        boxes2[:, 5] = scores
        return boxes2, keep_map

    def pose_track(self, filenames_map=None, **kw):
        """Track ids for everything accumulated so far (module-level `pose_track`, same keywords) -> (tracks [idx] int32,
        num_tracks {video: int}).  `filenames_map`: the frames to track, typically the keep_map of `pose_nms` (duplicates
        removed, each frame in pick order); default the accumulator's own map.  `tracks` is the `tracks=` argument of
        `write_posetrack_results`.  The accumulator itself is not modified."""
        fmap = self.filenames_map if filenames_map is None else filenames_map
        return pose_track(self.all_preds[:self.idx], self.all_boxes[:self.idx], fmap, **kw)

    def track_refine(self, tracks, filenames_map=None, boxes=None, **kw):
        """Gap filling, smoothing, rescoring and pruning of the tracks of everything accumulated so far (module-level
        `track_refine`, same keywords) -> (preds2, boxes2, filenames_map2, tracks2), the arguments of
        `write_posetrack_results(..., tracks=tracks2)`.  `tracks`: what `pose_track` returned; `filenames_map`: the map it
        was given (default the accumulator's own); `boxes`: the rescored copy `pose_nms` returned (default all_boxes, the
        detector's box scores).  The accumulator itself is not modified."""
        fmap = self.filenames_map if filenames_map is None else filenames_map
        boxes = self.all_boxes[:self.idx] if boxes is None else boxes
        return track_refine(self.all_preds[:self.idx], boxes, fmap, tracks, **kw)

    def coco_results(self, image_ids, keep=None, boxes=None, category_id=1):
        """Everything accumulated so far as COCO result dicts (module-level `coco_keypoint_results`): image_ids [idx] the
        COCO image id of every row, keep the keep map of `pose_nms` (or a flat list of rows), boxes the rescored copy it
        returned (default: all_boxes, the detector's box scores) -- so pose_nms -> coco_results -> pack_coco_keypoints ->
        coco_keypoint_ap runs without a file.  The accumulator itself is not modified."""
        boxes = self.all_boxes[:self.idx] if boxes is None else boxes
        return coco_keypoint_results(self.all_preds[:self.idx], boxes, image_ids, keep=keep, category_id=category_id)


@torch.no_grad()
def evaluate_loop(model, batches, num_samples, num_joints=17, flip=False, shift_heatmap=False, flip_pairs=FLIP_PAIRS,
                  decode='standard', blur_kernel=11, integral_beta=20.0):
    """The reference's validation loop (core fn :256-309) on the HIP path.  `batches` yields
    (kf_x, sup_x, target_heatmaps | None, meta) with meta = {'image': [names], 'center': [B,2], 'scale': [B,2],
    'score': [B]}; tensors may live on the host (they are moved to the model's device).  -> EvalAccumulator.
    flip=True: flip testing -- both heads (final_hm, kf_bb_hm) are merged from one doubled-batch forward; decode and
    PCK run on the merged maps.  decode='dark': both heads are decoded with dark_get_final_preds (blur_kernel: odd, 9..17);
    decode='integral': both with integral_get_final_preds at integral_beta.  PCK stays on the argmax."""
    final_preds = _decoder(decode, blur_kernel, integral_beta)
    dev = next(model.parameters()).device
    acc = EvalAccumulator(num_samples, num_joints)
    model.eval()
    for kf_x, sup_x, target, meta in batches:
        kf_x, sup_x = kf_x.to(dev), sup_x.to(dev)
        if flip:
            out = _flip_forward(model, kf_x, sup_x)
            pred_hm, kf_bb_hm = (flip_merge(o, flip_pairs, shift_heatmap) for o in out[:2])
        else:
            out = model(kf_x, sup_x)
            pred_hm, kf_bb_hm = out[0], out[1]
        center = np.asarray(meta['center'], dtype=np.float32)
        scale = np.asarray(meta['scale'], dtype=np.float32)
        pc, pm = final_preds(pred_hm, center, scale)
        bc, bm = final_preds(kf_bb_hm, center, scale)
        if target is not None:
            B, J, H, W = pred_hm.shape
            target = target.to(dev).float().contiguous()
            rows = torch.empty(2, J + 3, device=dev)
            iws = torch.empty(2 * B * J, dtype=torch.int64, device=dev)
            mws = torch.empty(2 * B * J, device=dev)
            s = torch.cuda.current_stream(dev).cuda_stream
            for k, hm in enumerate((pred_hm, kf_bb_hm)):
                lib().call('fami_pck_accuracy_f32', hm.data_ptr(), target.data_ptr(), rows[k].data_ptr(), iws.data_ptr(),
                           mws.data_ptr(), B, J, H, W, 0.5, s)
            r = rows.cpu().numpy()
            for k in range(2):
                acc.add_accuracy(k, float(r[k, J + 1]), int(r[k, J + 2]))
        acc.add(pc.cpu().numpy(), pm.cpu().numpy(), bc.cpu().numpy(), bm.cpu().numpy(), center, scale,
                np.asarray(meta['score']), list(meta['image']))
    return acc


# ---------------------------------------------------------------------------------------- rescoring + OKS-NMS
def pose_nms_options(cfg, phase):
    """-> {'in_vis_thre', 'oks_thre', 'soft'} for `pose_nms` from the reference's switches: VAL.IN_VIS_THRE / OKS_THRE /
    SOFT_NMS in the validation phase, the same keys of TEST in the test phase (mppe_config.py:326-330, 343-347); where
    the node or a key is absent, the reference's defaults 0.0 / 0.5 / False."""
    if phase == VAL_PHASE:
        node = 'VAL'
    elif phase == TEST_PHASE:
        node = 'TEST'
    else:
        raise ValueError('pose NMS is an evaluation option: phase %r has none' % (phase,))
    sub = cfg.get(node) if hasattr(cfg, 'get') else None
    sub = sub if hasattr(sub, 'get') else {}
    return {'in_vis_thre': float(sub.get('IN_VIS_THRE', 0.0)), 'oks_thre': float(sub.get('OKS_THRE', 0.5)),
            'soft': bool(sub.get('SOFT_NMS', False))}


def _nms_lists(filenames_map, N, who='pose_nms'):
    """-> (index [n] int32, seg [M+1] int32) of the lists of `filenames_map` in its order; ValueError for a list longer
    than the kernel's cap, an index outside [0, N), a non-integer index, or an index used twice.  The lists are checked
    as one array (a validation set has tens of thousands of them); the offending image is looked up only to be named."""
    lists = [list(v) for v in filenames_map.values()]
    seg = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(v) for v in lists], out=seg[1:])

    def image_of(pos):
        return list(filenames_map)[int(np.searchsorted(seg, pos, side='right')) - 1]

    if len(lists) and np.diff(seg).max() > NMS_MAX_PER_IMAGE:
        m = int(np.diff(seg).argmax())
        raise ValueError(who + ': image %r has %d detections, the limit is %d per image'
                         % (list(filenames_map)[m], len(lists[m]), NMS_MAX_PER_IMAGE))
    flat = np.asarray([i for v in lists for i in v])
    if flat.size == 0:
        return np.zeros(0, dtype=np.int32), seg.astype(np.int32)
    if flat.ndim != 1 or flat.dtype.kind not in 'iu':
        raise ValueError(who + ': the lists of filenames_map must hold integer row indices (got %s)' % flat.dtype)
    bad = np.flatnonzero((flat < 0) | (flat >= N))
    if bad.size:
        raise ValueError(who + ': image %r lists row %d outside [0, %d)' % (image_of(bad[0]), flat[bad[0]], N))
    count = np.bincount(flat, minlength=N)
    if count.max() > 1:
        raise ValueError(who + ': row %d is listed %d times' % (int(count.argmax()), int(count.max())))
    return flat.astype(np.int32), seg.astype(np.int32)


def pose_nms(preds, boxes, filenames_map, in_vis_thre=0.0, oks_thre=0.5, soft=False, max_dets=20, vis_thre=None,
             sigmas=None, device='cuda'):
    """Rescoring and OKS-NMS of a whole evaluation set in one launch (csrc/nms.hip; include/fami.h has the arithmetic).
    preds [N,J,3] (x, y, confidence in image pixels) and boxes [N,6] (column 4 the box area, column 5 the box score) are
    host arrays as `EvalAccumulator` holds them; filenames_map {image -> [row indices]} groups them into frames.
    -> (scores [N] float64, keep_map): scores[i] = box score x mean confidence of the joints of i with confidence >
    in_vis_thre (0 when none passes; also 0 for a row that no image lists), computed in fp64 and rounded to fp32 once;
    keep_map has the keys of filenames_map in its order, each value the list of kept row indices in pick order
    (descending score; equal scores: the one listed first).
    soft=False is the reference's `oks_nms`: a kept pose suppresses every lower-scored one of its frame with OKS >
    oks_thre.  soft=True is `soft_oks_nms` with the Gaussian `_rescore`: the pose with the highest working score is
    kept, the others' working scores are multiplied by exp(-OKS^2 / oks_thre), at most max_dets (the reference's default
    20) per frame; the returned scores stay the rescored values, as the reference returns only indices.
    vis_thre=None counts all joints in an OKS; with a value, the joints whose confidence in the COMPARED (lower-scored)
    pose exceeds it -- the picked pose's visibility is not read: the reference's `list(vg > t) and list(vd > t)`
    evaluates to its second operand, and that is kept here (an empty mask gives OKS 0: nothing is suppressed).
    sigmas: the per-joint OKS constants, default COCO_SIGMAS for J = 17 (any other J needs its own).
    The inputs are rounded to fp32 on upload (the pipeline's own values are fp32 already); the arithmetic on them is
    fp64.  One upload, one launch, one download.  ValueError before any device work for: J != 17 without sigmas, J > 32,
    non-finite inputs, an image with more than 256 detections, a row index outside [0, N) or used twice, max_dets < 1,
    oks_thre <= 0 with soft=True."""
    preds, boxes, N, J, sig32 = _pose_set('pose_nms', preds, boxes, sigmas)
    _int_option('pose_nms', 'max_dets must be an integer >= 1', max_dets, 1, math.inf)
    in_vis_thre, oks_thre = float(in_vis_thre), float(oks_thre)
    vis = None if vis_thre is None else float(vis_thre)
    if not (np.isfinite(in_vis_thre) and np.isfinite(oks_thre) and (vis is None or np.isfinite(vis))):
        raise ValueError('pose_nms: thresholds must be finite')
    if soft and not oks_thre > 0:
        raise ValueError('pose_nms: soft mode divides by oks_thre, which must be > 0 (got %r)' % oks_thre)
    k32, a32, b32 = _fp32('pose_nms', 'preds, box areas and box scores', preds, boxes[:, 4], boxes[:, 5])
    index, seg = _nms_lists(filenames_map, N)
    dev = _hip_device('pose_nms', device)
    M, n = len(seg) - 1, int(index.size)
    keys = list(filenames_map.keys())
    if N == 0 or M == 0:
        return np.zeros(N, dtype=np.float64), {k: [] for k in keys}
    _index_range('pose_nms', N, J)
    # the six inputs (index holds n <= N rows, zeros behind them), then the three outputs with their initial values (score 0
    # and rank -1 for rows that no image lists): the outputs come back in one download
    w = _Words(dev, [('kpts', 'f32', (N, J, 3), k32), ('area', 'f32', N, a32), ('box_score', 'f32', N, b32),
                     ('sigmas', 'f32', J, sig32), ('index', 'i32', N, np.pad(index, (0, N - n))), ('seg', 'i32', M + 1, seg),
                     ('score', 'f32', N), ('rank', 'i32', N, -1), ('kept', 'i32', M)])
    with torch.cuda.device(dev):
        lib().call('fami_pose_nms_f32', w.ptr('kpts'), w.ptr('area'), w.ptr('box_score'), w.ptr('sigmas'), w.ptr('index'),
                   w.ptr('seg'), N, J, M, in_vis_thre, oks_thre, 1 if soft else 0, int(max_dets), 0.0 if vis is None else vis,
                   0 if vis is None else 1, w.ptr('score'), w.ptr('rank'), w.ptr('kept'),
                   torch.cuda.current_stream(dev).cuda_stream)
    out = w.download('score')
    scores, rank, kept = out['score'].astype(np.float64), out['rank'], out['kept']
    if (kept < 0).any():
        raise RuntimeError('pose_nms: the kernel refused image %r' % (keys[int(np.argmax(kept < 0))],))
    # the kept rows of all images, ordered by (image, rank), then cut at the per-image counts
    r = rank[index]
    sel = np.flatnonzero(r >= 0)
    image = np.repeat(np.arange(M), np.diff(seg))[sel]
    rows = index[sel][np.lexsort((r[sel], image))].tolist()
    cut = np.concatenate([[0], np.cumsum(kept)]).tolist()
    keep_map = {key: rows[cut[m]:cut[m + 1]] for m, key in enumerate(keys)}
    return scores, keep_map


# ---------------------------------------------------------------------------------------- OKS pose tracking
def posetrack_frame_of(key):
    """The writer's own rule (`write_posetrack_results`): '.../<a>/<b>/<number>.<ext>' -> ('<a>/<b>', number)."""
    parts = str(key).split('/')
    try:
        if len(parts) < 3:
            raise ValueError
        return parts[-3] + '/' + parts[-2], int(osp.splitext(parts[-1])[0])
    except ValueError:
        raise ValueError("pose_track: cannot read a video and a frame number from %r (expected '.../<video>/<number>.jpg'): "
                         'pass frame_of' % (key,)) from None


def _track_tables(filenames_map, N, frame_of=None):
    """-> (index [n], fseg [M+1], fnum [M], vseg [V+1] int32, videos): the rows of `filenames_map` grouped by frame (each
    list in its own order), the frames grouped by video (videos in the order of their first key) in ascending frame
    number.  ValueError for what `_nms_lists` refuses, a key `frame_of` cannot place, a frame number that is no int32, and
    two keys with the same (video, frame number)."""
    index, seg = _nms_lists(filenames_map, N, 'pose_track')
    frame_of = posetrack_frame_of if frame_of is None else frame_of
    videos, vid, num, seen = {}, [], [], {}
    for key in filenames_map:
        where = frame_of(key)
        if not isinstance(where, tuple) or len(where) != 2:
            raise ValueError('pose_track: frame_of(%r) must return (video, frame_number), got %r' % (key, where))
        video, f = where
        _int_option('pose_track', 'the frame number of %r must be an integer that fits int32', f, -2 ** 31, 2 ** 31 - 1, key)
        if (video, int(f)) in seen:
            raise ValueError('pose_track: %r and %r are both frame %d of video %r' % (seen[(video, int(f))], key, f, video))
        seen[(video, int(f))] = key
        vid.append(videos.setdefault(video, len(videos)))
        num.append(int(f))
    M = len(vid)
    vid, num = np.asarray(vid, dtype=np.int64), np.asarray(num, dtype=np.int64)
    order = np.lexsort((num, vid))
    lens = np.diff(seg.astype(np.int64))[order]
    fseg = np.zeros(M + 1, dtype=np.int64)
    np.cumsum(lens, out=fseg[1:])
    take = np.repeat(seg[:-1].astype(np.int64)[order] - fseg[:-1], lens) + np.arange(int(fseg[-1]))
    vseg = np.zeros(len(videos) + 1, dtype=np.int64)
    np.cumsum(np.bincount(vid, minlength=len(videos)), out=vseg[1:])
    return (index[take].astype(np.int32), fseg.astype(np.int32), num[order].astype(np.int32), vseg.astype(np.int32),
            list(videos))


def pose_track(preds, boxes, filenames_map, oks_thre=0.3, max_gap=3, vis_thre=None, sigmas=None, frame_of=None,
               device='cuda'):
    """Person identities for a whole evaluation set in one launch (csrc/track.hip; include/fami.h has the rule, which is
    this project's: the reference declares EVAL_TRACKING and writes the position in the frame as track_id).
    preds [N,J,3], boxes [N,6] (column 4 the box area) and filenames_map {image -> [row indices]} as for `pose_nms`,
    typically its keep_map: duplicates removed, each frame in pick order.  frame_of(key) -> (video, frame_number);
    default the writer's rule, video = parts[-3] + '/' + parts[-2] and number = int(stem of parts[-1]) of key.split('/').
    -> (tracks [N] int32, num_tracks {video: ids handed out}); tracks is -1 for a row that no image lists.
    Per video, frames in ascending frame NUMBER (their order in filenames_map does not matter; frames without a
    detection are simply absent).  A live track holds an id and the pose, box area and frame number of the last
    detection matched to it.  Before frame f every track with f - last_frame > max_gap is retired (max_gap = 1:
    consecutive frame numbers only).  The detections of f are walked in the order of filenames_map[image]: a detection
    takes the live track with the largest OKS -- tracks already matched in this frame and tracks created in it do not
    compete; equal OKS: the lowest id -- if that OKS is > oks_thre, receives its id, and the track takes its pose, area and
    frame number; otherwise it is new.  After the walk the new detections get the next ids in list order and become
    live.  Ids start at 0 in every video and are never reused.
    OKS(track q, detection d) = mean_j exp(-(dx^2 + dy^2) / (2 sigma_j)^2 / ((a_q + a_d) / 2 + 2^-52) / 2), the arithmetic
    of `pose_nms` (fp64 on the inputs rounded to fp32), over all joints, or with vis_thre over the joints whose
    confidence in d exceeds it (an empty mask gives OKS 0).  sigmas: default COCO_SIGMAS for J = 17.
    oks_thre = 0.3 and max_gap = 3 are STARTING VALUES, NOT TUNED: no PoseTrack data was available where this was built.
    One upload, one launch (one workgroup per video), one download.  ValueError before any device work for: shape
    errors, J outside 1 .. 32, J != 17 without sigmas, non-finite or non-positive sigmas, non-finite inputs or thresholds,
    max_gap no integer >= 1, a key frame_of cannot place, two keys with the same (video, frame number), a frame with more
    than 256 rows, a row outside [0, N) or listed twice.  ValueError naming the video after the download if it had more
    than 256 live tracks at once (the other videos of the call are computed as if alone, but nothing is returned)."""
    preds, boxes, N, J, sig32 = _pose_set('pose_track', preds, boxes, sigmas)
    _int_option('pose_track', 'max_gap must be an integer >= 1', max_gap, 1, 2 ** 31 - 1)
    oks_thre = float(oks_thre)
    vis = None if vis_thre is None else float(vis_thre)
    if not (np.isfinite(oks_thre) and (vis is None or np.isfinite(vis))):
        raise ValueError('pose_track: thresholds must be finite')
    k32, a32 = _fp32('pose_track', 'preds and box areas', preds, boxes[:, 4])
    index, fseg, fnum, vseg, videos = _track_tables(filenames_map, N, frame_of)
    dev = _hip_device('pose_track', device)
    M, V, n = len(fnum), len(videos), int(index.size)
    if N == 0 or M == 0:
        return np.full(N, -1, dtype=np.int32), {}
    _index_range('pose_track', N, J)
    # the seven inputs, then the two outputs (track pre-filled with -1 for the rows that no image lists), which come back in
    # one download
    w = _Words(dev, [('kpts', 'f32', (N, J, 3), k32), ('area', 'f32', N, a32), ('sigmas', 'f32', J, sig32),
                     ('index', 'i32', n, index), ('fseg', 'i32', M + 1, fseg), ('fnum', 'i32', M, fnum),
                     ('vseg', 'i32', V + 1, vseg), ('track', 'i32', N, -1), ('ntracks', 'i32', V)])
    with torch.cuda.device(dev):
        lib().call('fami_pose_track_f32', w.ptr('kpts'), w.ptr('area'), w.ptr('sigmas'), w.ptr('index'), w.ptr('fseg'),
                   w.ptr('fnum'), w.ptr('vseg'), N, J, n, M, V, oks_thre, int(max_gap), 0.0 if vis is None else vis,
                   0 if vis is None else 1, w.ptr('track'), w.ptr('ntracks'), torch.cuda.current_stream(dev).cuda_stream)
    out = w.download('track')
    tracks, count = out['track'].copy(), out['ntracks']
    if (count < 0).any():
        raise ValueError('pose_track: video %r has more than %d live tracks at once (the limit of one workgroup)'
                         % (videos[int(np.argmax(count < 0))], NMS_MAX_PER_IMAGE))
    return tracks, {video: int(c) for video, c in zip(videos, count)}


# ---------------------------------------------------------------------------------------- track refinement
def posetrack_key_of(video, frame_number, sibling_key):
    """The key of a frame that had none, after a frame of the same video: the sibling's directory, the number zero-padded to
    the width of the sibling's stem, the sibling's extension ('.../000001_bonn/00000007.jpg', 9 -> '.../000001_bonn/00000009.jpg')."""
    head, name = osp.split(str(sibling_key))
    stem, ext = osp.splitext(name)
    return osp.join(head, '%0*d%s' % (len(stem), frame_number, ext))


def _refine_options(max_fill, fill_conf, smooth_radius, smooth_sigma, conf_thre, min_len):
    """-> (fill_conf, smooth_sigma as floats, conf_thre as np.float32) or ValueError"""
    _int_option('track_refine', 'max_fill must be an integer in 0 .. %d', max_fill, 0, REFINE_MAX, REFINE_MAX)
    _int_option('track_refine', 'smooth_radius must be an integer in 0 .. %d', smooth_radius, 0, REFINE_MAX, REFINE_MAX)
    _int_option('track_refine', 'min_len must be an integer >= 1', min_len, 1, 2 ** 31 - 1)
    fill_conf, sigma, thre = float(fill_conf), float(smooth_sigma), float(conf_thre)
    with np.errstate(over='ignore'):
        thre32 = np.float32(thre)
    if not (np.isfinite(fill_conf) and np.isfinite(sigma) and np.isfinite(thre32)):
        raise ValueError('track_refine: fill_conf, smooth_sigma and conf_thre must be finite (conf_thre in fp32)')
    if not sigma > 0:
        raise ValueError('track_refine: smooth_sigma must be > 0, got %r' % sigma)
    if not 0 <= fill_conf <= 1:
        raise ValueError('track_refine: fill_conf must be in [0, 1], got %r' % fill_conf)
    if thre32 < 0:
        raise ValueError('track_refine: conf_thre must be >= 0 (a weight is a confidence above it), got %r' % thre)
    return fill_conf, sigma, thre32


def _refine_members(filenames_map, N, tracks, frame_of):
    """The members of all tracks sorted by (video, id, frame) -> (rows, video numbers, ids, frame numbers: int64 [n] each,
    videos, key_at {(video, frame number): key}).  ValueError for what `_track_tables` refuses, a listed row with a
    negative id, an id twice in one frame."""
    index, fseg, fnum, vseg, videos = _track_tables(filenames_map, N, frame_of)
    frame_of = posetrack_frame_of if frame_of is None else frame_of
    key_at = {}
    for key in filenames_map:
        video, f = frame_of(key)
        key_at[(video, int(f))] = key
    frame = np.repeat(np.arange(len(fnum)), np.diff(fseg))              # of every position of index
    rows, f = index.astype(np.int64), fnum.astype(np.int64)[frame]
    vid = np.repeat(np.arange(len(videos)), np.diff(vseg))[frame]
    ids = tracks[rows].astype(np.int64)
    if (ids < 0).any():
        r = int(rows[np.argmax(ids < 0)])
        raise ValueError('track_refine: row %d is listed by an image and has track id %d' % (r, tracks[r]))
    order = np.lexsort((f, ids, vid))
    rows, vid, ids, f = rows[order], vid[order], ids[order], f[order]
    twice = (vid[1:] == vid[:-1]) & (ids[1:] == ids[:-1]) & (f[1:] == f[:-1])
    if twice.any():
        i = int(np.argmax(twice))
        raise ValueError('track_refine: track id %d occurs twice in frame %d of video %r (rows %d and %d)'
                         % (ids[i], f[i], videos[vid[i]], rows[i], rows[i + 1]))
    return rows, vid, ids, f, videos, key_at


def _refine_tables(mrow, mvid, mid, mf, max_fill, N):
    """The members sorted by (video, id, frame) -> (fill [G,5]: the end rows a and b, the frame number and the ends' frame
    numbers of every new row, in (video, id, frame) order -- they get the rows N, N + 1, ...; their video numbers and ids;
    the members after the fill sorted the same way: rows [Mm], frame numbers [Mm], track of each [Mm], tseg [T+1])."""
    same = (mvid[1:] == mvid[:-1]) & (mid[1:] == mid[:-1])
    gap = mf[1:] - mf[:-1] - 1
    pa = np.flatnonzero(same & (gap >= 1) & (gap <= max_fill))
    cnt = gap[pa]
    G = int(cnt.sum())
    g_f = np.repeat(mf[pa], cnt) + np.arange(G) - np.repeat(np.cumsum(cnt) - cnt, cnt) + 1
    fill = np.stack([np.repeat(mrow[pa], cnt), np.repeat(mrow[pa + 1], cnt), g_f, np.repeat(mf[pa], cnt),
                     np.repeat(mf[pa + 1], cnt)], axis=1)
    g_vid, g_id = np.repeat(mvid[pa], cnt), np.repeat(mid[pa], cnt)
    avid, aid, af = np.concatenate([mvid, g_vid]), np.concatenate([mid, g_id]), np.concatenate([mf, g_f])
    order = np.lexsort((af, aid, avid))
    srow, svid, sid = np.concatenate([mrow, N + np.arange(G)])[order], avid[order], aid[order]
    start = np.ones(len(srow), dtype=bool)
    start[1:] = (svid[1:] != svid[:-1]) | (sid[1:] != sid[:-1])
    return fill, g_vid, g_id, srow, af[order], np.cumsum(start) - 1, np.concatenate([np.flatnonzero(start), [len(srow)]])


def track_refine(preds, boxes, filenames_map, tracks, max_fill=2, fill_conf=1.0, smooth_radius=2, smooth_sigma=1.0,
                 conf_thre=0.0, rescore=False, min_len=1, frame_of=None, key_of=None, device='cuda'):
    """Refinement of the tracks `pose_track` handed out, between it and the writer (csrc/track_refine.hip; include/fami.h
    has the rule, which is this project's: the reference has no tracker).  preds [N,J,3], boxes [N,6], filenames_map and
    frame_of as for `pose_track`; tracks [N] integer, its output.
    -> (preds2 [N+G,J,3] float32, boxes2 [N+G,6] float64, filenames_map2, tracks2 [N+G] int32): the arguments of
    `write_posetrack_results(preds2, boxes2, filenames_map2, ..., tracks=tracks2)`.  The first N rows keep their numbers; G
    rows are new.  The members of a track are the listed rows of one (video, id), by ascending frame number.
    1. Fill (max_fill >= 1): consecutive members a, b of a track with 1 <= f_b - f_a - 1 <= max_fill get a new row for every
       frame number between them: x, y and box columns 0 .. 4 are v_a + (v_b - v_a) * t with t = (f - f_a) / (f_b - f_a), the
       confidences and box column 5 are min(of a, of b) * fill_conf.  New rows are numbered N, N + 1, ... in (video, id,
       frame) order and appended to the list of their frame's key; a frame without a key gets key_of(video, frame_number,
       sibling_key) -- default `posetrack_key_of`; the sibling is the key of end a of the first new row of that frame --
       behind all existing keys, in (video, frame) order.  A longer gap is left alone.
    2. Smooth (smooth_radius >= 1): x, y of joint j of member i with confidence > conf_thre become the mean of the members
       within smooth_radius frame numbers whose joint j passes conf_thre too, weighted with exp(-d^2 / (2 smooth_sigma^2))
       times the confidence; copied bit for bit if no other member contributes.  Always from unsmoothed neighbours;
       confidences do not change.
    3. rescore=True: box column 5 of every member becomes the mean score of its track (after the fill).
    4. Prune (min_len >= 2): tracks with fewer members (after the fill) leave the lists of filenames_map2 (the keys stay)
       and get tracks2 = -1.
    Arithmetic: fp64 on the inputs rounded to fp32, one rounding per operation, results rounded to fp32 once; preds2 is the
    fp32 set, boxes2 holds the input's values in its first N rows except where a stage wrote.  Rows that no image lists
    are carried through.  With max_fill=0, smooth_radius=0, rescore=False, min_len=1 nothing is rounded and nothing
    launched: the four results are copies of the inputs (tracks as int32).
    The defaults are STARTING VALUES, NOT TUNED: no PoseTrack data was available where this was built.
    One upload, at most three launches (fill, smooth, score), one download.  ValueError before any device work for:
    everything `pose_track` refuses about shapes, J and the map; tracks not [N] integer (int32 range); a listed row with a
    negative id; an id twice in one frame of a video; non-finite inputs or options; max_fill or smooth_radius outside
    0 .. 16; smooth_sigma <= 0; fill_conf outside [0, 1]; conf_thre < 0; min_len < 1; a key_of whose key frame_of does not
    place at (video, frame_number) or that exists already; a frame with more than 256 rows after the fill.  The inputs are
    not modified."""
    who = 'track_refine'
    preds, boxes, N, J = _pose_shapes(who, preds, boxes)
    tracks = np.asarray(tracks)
    if tracks.ndim != 1 or tracks.dtype.kind not in 'iu' or len(tracks) != N:
        raise ValueError('%s: tracks must be an integer array of %d entries, got %s %s' % (who, N, tracks.dtype, tracks.shape))
    if N and (tracks.min() < -2 ** 31 or tracks.max() > 2 ** 31 - 1):
        raise ValueError('%s: track ids must fit int32' % who)
    fill_conf, sigma, thre32 = _refine_options(max_fill, fill_conf, smooth_radius, smooth_sigma, conf_thre, min_len)
    k32, b32 = _fp32(who, 'preds and boxes', preds, boxes)
    mrow, mvid, mid, mf, videos, key_at = _refine_members(filenames_map, N, tracks, frame_of)
    fmap2 = {key: [int(r) for r in rows] for key, rows in filenames_map.items()}
    if max_fill == 0 and smooth_radius == 0 and not rescore and min_len == 1:
        return preds.copy(), boxes.copy(), fmap2, tracks.astype(np.int32)
    fill, g_vid, g_id, srow, sf, mtrk, tseg = _refine_tables(mrow, mvid, mid, mf, int(max_fill), N)
    G = len(fill)
    R = N + G
    _index_range(who, R, J)
    _refine_keys(fmap2, key_at, videos, g_vid, fill, N, frame_of, key_of)
    Mm, T, radius = len(srow), len(tseg) - 1, int(smooth_radius)
    dev = _hip_device(who, device)
    preds2, boxes2 = np.concatenate([k32, np.zeros((G, J, 3), np.float32)]), np.concatenate([boxes.astype(np.float64), np.zeros((G, 6))])
    tracks2 = np.concatenate([tracks.astype(np.int32), g_id.astype(np.int32)])
    if Mm and (G or radius or rescore):
        d = np.arange(radius + 1, dtype=np.float64)
        # the tables, the inputs with room for the new rows behind them, then the outputs, which come back in one download
        w = _Words(dev, [('gauss', 'f64', radius + 1, np.exp(-(d * d) / (2.0 * sigma * sigma))), ('fill', 'i32', (G, 5), fill),
                         ('mrow', 'i32', Mm, srow), ('mfr', 'i32', Mm, sf), ('mtrk', 'i32', Mm, mtrk), ('tseg', 'i32', T + 1, tseg),
                         ('kpts', 'f32', (N, J, 3), k32), ('kpts_new', 'f32', (G, J, 3)), ('boxes', 'f32', (N, 6), b32),
                         ('boxes_new', 'f32', (G, 6)), ('out', 'f32', (R if radius else 0, J, 3)),
                         ('score', 'f32', T if rescore else 0), ('flag', 'i32', 3)])
        with torch.cuda.device(dev):
            s = torch.cuda.current_stream(dev).cuda_stream
            if G:
                lib().call('fami_track_fill_f32', w.ptr('kpts'), w.ptr('boxes'), w.ptr('fill'), N, J, G, fill_conf,
                           w.ptr('kpts_new'), w.ptr('boxes_new'), w.ptr('flag'), s)
            if radius:
                lib().call('fami_track_smooth_f32', w.ptr('kpts'), w.ptr('mrow'), w.ptr('mfr'), w.ptr('mtrk'), w.ptr('tseg'),
                           w.ptr('gauss'), R, J, Mm, T, radius, float(thre32), w.ptr('out'), w.ptr('flag') + 4, s)
            if rescore:
                lib().call('fami_track_score_f32', w.ptr('boxes'), w.ptr('mrow'), w.ptr('tseg'), R, Mm, T, w.ptr('score'),
                           w.ptr('flag') + 8, s)
        out = w.download('boxes_new' if radius else 'kpts_new')     # (without the filter the new poses come back as filled)
        if out['flag'].any():
            raise RuntimeError('%s: the %s kernel refused its tables' % (who, ('fill', 'smooth', 'score')[int(np.argmax(out['flag'] != 0))]))
        boxes2[N:] = out['boxes_new']
        if radius:
            preds2[srow] = out['out'][srow]
        else:
            preds2[N:] = out['kpts_new']
        if rescore:
            boxes2[srow, 5] = out['score'][mtrk]
    # 4. tracks that are too short leave the lists
    short = (np.diff(tseg) < min_len)[mtrk]
    if short.any():
        dead = set(srow[short].tolist())
        tracks2[srow[short]] = -1
        for key, rows in fmap2.items():
            fmap2[key] = [r for r in rows if r not in dead]
    return preds2, boxes2, fmap2, tracks2


def _refine_keys(fmap2, key_at, videos, g_vid, fill, N, frame_of, key_of):
    """Appends the new rows N, N + 1, ... (fill [G,5]: end rows, frame number, the ends' frame numbers; g_vid their video
    numbers) to the lists of `fmap2`; a frame without a key gets one from key_of, behind all existing keys in (video, frame)
    order.  ValueError for a key that frame_of does not place there or that exists, and for a list over the cap."""
    frame_of = posetrack_frame_of if frame_of is None else frame_of
    key_of = posetrack_key_of if key_of is None else key_of
    made, key_g = {}, []
    for v, (_, _, f, fa, _) in zip(g_vid.tolist(), fill.tolist()):
        key = key_at.get((videos[v], f), made.get((v, f)))
        if key is None:
            key = made[(v, f)] = key_of(videos[v], f, key_at[(videos[v], fa)])
            where = frame_of(key)
            if not isinstance(where, tuple) or len(where) != 2 or where[0] != videos[v] or where[1] != f:
                raise ValueError('track_refine: key_of(%r, %d, ...) gave %r, which frame_of places at %r'
                                 % (videos[v], f, key, where))
            if key in fmap2:
                raise ValueError('track_refine: key_of(%r, %d, ...) gave %r, which exists already' % (videos[v], f, key))
        key_g.append(key)
    for where in sorted(made):
        fmap2[made[where]] = []
    for g, key in enumerate(key_g):
        fmap2[key].append(N + g)
        if len(fmap2[key]) > NMS_MAX_PER_IMAGE:
            raise ValueError('track_refine: image %r would list more than %d rows after the fill' % (key, NMS_MAX_PER_IMAGE))


# ---------------------------------------------------------------------------------------- PoseTrack JSON writer
def coco2posetrack_ord(preds, global_score=1):
    """keypoints_ord.py:14-73.  preds: 4x17 (x, y, score, score) in COCO order -> list of 15 PoseTrack points."""
    data = []
    src, dst = COCO_JOINT, POSETRACK_JOINT
    global_score = float(global_score)
    rsho, lsho, nose = src.index('right_shoulder'), src.index('left_shoulder'), src.index('nose')
    for k, name in enumerate(dst):
        if name in src:
            ind = src.index(name)
            local_score = (preds[2, ind] + preds[2, ind]) / 2.0
            data.append({'id': [k], 'x': [float(preds[0, ind])], 'y': [float(preds[1, ind])],
                         'score': [local_score * global_score]})
        elif name == 'neck':
            x = (preds[0, rsho] + preds[0, lsho]) / 2.0
            y = (preds[1, rsho] + preds[1, lsho]) / 2.0
            local_score = (preds[2, rsho] + preds[2, lsho]) / 2.0
            data.append({'id': [k], 'x': [float(x)], 'y': [float(y)], 'score': [local_score * global_score]})
        elif name == 'head_top':
            x_msho = (preds[0, rsho] + preds[0, lsho]) / 2.0
            y_msho = (preds[1, rsho] + preds[1, lsho]) / 2.0
            x_nose, y_nose = preds[0, nose], preds[1, nose]
            local_score = (preds[2, rsho] + preds[2, lsho]) / 2.0
            data.append({'id': [k], 'x': [float(x_nose - (x_msho - x_nose))], 'y': [float(y_nose - (y_msho - y_nose))],
                         'score': [local_score]})        # :72: the head-top score is NOT scaled by the box score
    return data


def convert_data_to_annorect_struct(poses, tracks, boxes, eval_tracking=False, tracking_threshold=0):
    """data_format.py:12-49."""
    annorect = []
    for j in range(len(poses)):
        score = boxes[j][0, 5]
        if eval_tracking and score > tracking_threshold:
            continue
        annorect.append({'annopoints': [{'point': coco2posetrack_ord(poses[j], global_score=score)}],
                         'score': [float(score)], 'track_id': [tracks[j]]})
    if len(poses) == 0:      # "MOTA requires each image to have at least one detection": a dummy prediction
        annorect.append({'annopoints': [{'point': [{'id': [0], 'x': [0], 'y': [0], 'score': [-100.0]}]}],
                         'score': [0], 'track_id': [0]})
    return annorect


def video2filenames(annot_dir):
    """posetrack_utils.py:13-56: {video dir -> annotation file name}, {video dir -> number of frames}."""
    files = [f for f in os.listdir(annot_dir) if osp.isfile(osp.join(annot_dir, f))]
    json_files = [f for f in files if '.json' in f]
    mat_files = [f for f in files if '.mat' in f]
    output, L = {}, {}
    if len(json_files) > 1:
        for fname in json_files:
            with open(osp.join(annot_dir, fname)) as fin:
                data = json.load(fin)
            if 'annolist' in data:
                temp = data['annolist'][0]['image'][0]['name']
                num_frames = len(data['annolist'])
            else:
                temp = data['images'][0]['file_name']
                num_frames = data['images'][0]['nframes']
            video = osp.dirname(temp)
            output[video], L[video] = fname, num_frames
    else:
        import scipy.io as sio
        for fname in mat_files:
            data = sio.loadmat(osp.join(annot_dir, fname), squeeze_me=True, struct_as_record=False)
            temp = data['annolist'][0].image.name
            num_frames = len(sio.loadmat(osp.join(annot_dir, fname))['annolist'][0])
            video = osp.dirname(temp)
            output[video], L[video] = fname.replace('.mat', '.json'), num_frames
    return output, L


def write_posetrack_results(preds, boxes, filenames_map, annot_dir, output_dir, is_posetrack18=False, phase='validate',
                            tracks=None):
    """PoseTrack_Alignment.evaluate up to the poseval call (:883-1017).  preds [N,17,3] (x, y, confidence in image
    coordinates), boxes [N,6] (center, scale, area, score), filenames_map {image path -> [row indices]}.
    Writes one JSON file per video under output_dir/{val,test}_set_json_results and returns {file path: video}.
    tracks: None -- every pose gets its position in its frame as track_id, the reference's placeholder (:998) -- or an [N]
    integer array, typically `pose_track`'s: the pose of row i gets tracks[i]; a listed row with a negative id is a
    ValueError, raised before anything is written."""
    if tracks is not None:
        tracks = np.asarray(tracks)
        if tracks.ndim != 1 or tracks.dtype.kind not in 'iu' or len(tracks) != len(preds):
            raise ValueError('write_posetrack_results: tracks must be an integer array of %d entries, got %s %s'
                             % (len(preds), tracks.dtype, tracks.shape))
        for key, rows in filenames_map.items():
            for idx in rows:
                if tracks[idx] < 0:
                    raise ValueError('write_posetrack_results: row %d of image %r has track id %d' % (idx, key, tracks[idx]))
    output_dir = osp.join(output_dir, 'val_set_json_results' if phase == 'validate' else 'test_set_json_results')
    os.makedirs(output_dir, exist_ok=True)
    video_map, vid2frame_map, vid2name_map = {}, {}, {}
    all_preds, all_boxes, all_rows = [], [], []
    cc = 0
    for key in filenames_map:
        parts = key.split('/')
        video_name = parts[-3] + '/' + parts[-2]
        img_sfx = parts[-3] + '/' + parts[-2] + '/' + parts[-1]
        frame_num = int(parts[-1].replace('.jpg', ''))
        video_map.setdefault(video_name, []).append(cc)
        vid2frame_map.setdefault(video_name, []).append(frame_num)
        vid2name_map.setdefault(video_name, []).append(img_sfx)
        pose_list, box_list = [], []
        for idx in filenames_map[key]:
            t = np.zeros((4, 17))
            t[0, :], t[1, :], t[2, :], t[3, :] = preds[idx, :, 0], preds[idx, :, 1], preds[idx, :, 2], preds[idx, :, 2]
            pose_list.append(t)
            b = np.zeros((1, 6))
            b[0, :] = boxes[idx, :]
            box_list.append(b)
        all_preds.append(pose_list)
        all_boxes.append(box_list)
        all_rows.append(list(filenames_map[key]))
        cc += 1

    out_filenames, L = video2filenames(annot_dir)
    out_data = {}
    for vid in video_map:
        cur_length = L['images/' + vid]
        kps_map, box_map, row_map, used = {}, {}, {}, []
        for c, idx in enumerate(video_map[vid]):
            frame_num = vid2frame_map[vid][c]
            used.append(frame_num)
            kps_map[frame_num] = (vid2name_map[vid][c], all_preds[idx])
            box_map[frame_num] = all_boxes[idx]
            row_map[frame_num] = all_rows[idx]
        sid, fid = (1, cur_length + 1) if not is_posetrack18 else (0, cur_length)
        for frame_num in range(sid, fid):
            if frame_num not in used:            # frames without a detection still get an (empty) entry
                arr = vid2name_map[vid][0].split('/')
                img_sfx = arr[0] + '/' + arr[1] + '/' + str(frame_num).zfill(6 if is_posetrack18 else 8) + '.jpg'
                kps, ids, bboxs = [], [], []
            else:
                img_sfx, kps = kps_map[frame_num]
                bboxs = box_map[frame_num]
                ids = list(range(len(kps))) if tracks is None else [int(tracks[i]) for i in row_map[frame_num]]
            out_data.setdefault(vid, []).append({'image': {'name': img_sfx}, 'imgnum': [frame_num],
                                                 'annorect': convert_data_to_annorect_struct(kps, ids, bboxs)})
    written = {}
    for vname, vdata in out_data.items():
        path = osp.join(output_dir, out_filenames[osp.join('images', vname)])
        with open(path, 'w') as f:
            json.dump({'annolist': vdata}, f)
        written[path] = vname
    return written


# ---------------------------------------------------------------------------------------- PoseTrack AP (poseval)
def _rect_has_points(rect):
    """eval_helpers.rectHasPoints (:370-373)."""
    a = rect.get('annopoints')
    return a is not None and len(a) > 0 and len(a[0]) > 0 and 'point' in a[0]


def _num(v, what, where):
    try:
        x = float(v)
    except (TypeError, ValueError):
        raise ValueError('pack_posetrack_frames: %s of %s is not a number (%r)' % (what, where, v))
    if not math.isfinite(x):
        raise ValueError('pack_posetrack_frames: %s of %s is not finite (%r)' % (what, where, v))
    return x


def _pack_points(points, where, with_score, unique_ids):
    """-> (row: 15 x (x, y, score) as a flat list; has mask).  The first occurrence of a joint id counts (getPointGTbyID,
    :72-79).  Plain lists: a numpy store per point would double the time of the pack."""
    row = [0.0] * (AP_JOINTS * 3)
    has = 0
    for pt in points:
        pid = pt.get('id')
        if pid is None:
            continue
        j = pid[0]
        if isinstance(j, (bool, np.bool_)) or not isinstance(j, (int, np.integer)) or not 0 <= j < AP_JOINTS:
            raise ValueError('pack_posetrack_frames: joint id %r of %s is outside 0 .. %d' % (j, where, AP_JOINTS - 1))
        x, y = _num(pt['x'][0], 'x', where), _num(pt['y'][0], 'y', where)
        sc = _num(pt['score'][0], 'score', where) if with_score and 'score' in pt else float(AP_MIN_SCORE)
        if (has >> j) & 1:
            if unique_ids:
                raise ValueError('pack_posetrack_frames: joint id %d is listed twice in %s, a frame with ignore regions '
                                 '(the reference filters before it picks the first)' % (j, where))
            continue
        has |= 1 << j
        row[3 * j:3 * j + 3] = (x, y, sc)
    return row, has


def pack_posetrack_frames(gt_annolists, pr_annolists, seq_ids=None):
    """The frames of an evaluation set as the flat fp64 / int32 arrays `posetrack_ap` uploads.  gt_annolists and
    pr_annolists are the `annolist` frames of all sequences, one entry per frame, in the same order (what
    `load_posetrack_dirs` returns).  Frame selection is the reference's (eval_helpers.load_data_dir -> cleanupData ->
    removeIgnoredPoints, :305-367, 442-444): a ground-truth frame with an empty `annorect` is dropped with its
    predictions; a rect without a `point` list is dropped; a frame's `ignore_regions` become its polygons (the point
    filter itself runs on the device).  The first occurrence of a joint id in a point list counts; a prediction without a
    `score` gets MIN_SCORE = -9999.
    -> dict: pr_xys [P,15,3] (x, y, score), pr_has [P], gt_xy [G,15,2], gt_has [G], gt_head [G,4] (x1, y1, x2, y2),
    pr_seg / gt_seg / poly_seg [F+1], vert_seg [NP+1], verts [NV,2], frame_index [F] (the position of every kept frame
    in the inputs).  A rect that the ignore filter empties stays in the arrays with an empty mask -- it matches nothing,
    which is what removing it does in the reference -- so `assigned` of `posetrack_ap` counts the annotated poses as
    packed here.
    ValueError for: unequal frame counts, a joint id outside 0 .. 14, non-finite coordinates or scores, more than 256
    predicted or 64 annotated poses in a frame (the frame is named), an annotated pose without its head rectangle, an
    ignore region of fewer than three points, and a joint id listed twice in a frame WITH ignore regions (the reference
    filters first and then takes the first that is left; that order is not restated).  Neither input is modified (the
    reference's assignGTmulti filters its prediction frames in place).
    seq_ids (one entry per input frame, what `load_posetrack_dirs(with_seq=True)` returns; any hashable) adds what
    `posetrack_mota` needs: gt_track [G] / pr_track [P] int32 (the `track_id` of every packed pose, renumbered from 0 in
    order of appearance within its sequence, annotated and predicted ids apart), frame_seq [F] int32 (the sequence of
    every kept frame, numbered in order of appearance) and seq_seg [S+1] int32 (sequence s owns the kept frames
    seq_seg[s] .. seq_seg[s+1); a sequence may own none).  Then also ValueError for: a pose with points but no
    `track_id`, a track id listed twice among one frame's annotated or among its predicted poses, a sequence whose
    frames are not contiguous, more than 256 ground-truth tracks in a sequence.  Without seq_ids the dict has exactly the
    keys above and no `track_id` is read."""
    if len(gt_annolists) != len(pr_annolists):
        raise ValueError('pack_posetrack_frames: %d ground-truth frames, %d prediction frames'
                         % (len(gt_annolists), len(pr_annolists)))
    if seq_ids is not None and len(seq_ids) != len(gt_annolists):
        raise ValueError('pack_posetrack_frames: %d frames, %d seq_ids' % (len(gt_annolists), len(seq_ids)))
    pr_rows, pr_has, gt_rows, gt_has, gt_head = [], [], [], [], []
    pr_seg, gt_seg, poly_seg, vert_seg, verts, kept = [0], [0], [0], [0], [], []
    gt_track, pr_track, frame_seq, seen, maps = [], [], [], {}, ({}, {})
    for idx, (gf, pf) in enumerate(zip(gt_annolists, pr_annolists)):
        if seq_ids is not None:
            sid = seq_ids[idx]
            if sid not in seen:
                seen[sid] = len(seen)
                maps = ({}, {})                                   # track ids are per sequence: renumbered from 0
            elif sid != seq_ids[idx - 1]:
                raise ValueError('pack_posetrack_frames: the frames of sequence %r are not contiguous (frame %d)' % (sid, idx))
        if len(gf['annorect']) == 0:
            continue
        where = 'frame %d' % idx
        regions = gf.get('ignore_regions') or []
        for reg in regions:
            pts = reg['point']
            if len(pts) < 3:
                raise ValueError('pack_posetrack_frames: an ignore region of %s has %d points, a polygon needs 3'
                                 % (where, len(pts)))
            verts.extend((_num(p['x'][0], 'ignore-region x', where), _num(p['y'][0], 'ignore-region y', where)) for p in pts)
            vert_seg.append(len(verts))
        g_rects = [r for r in gf['annorect'] if _rect_has_points(r)]
        p_rects = [r for r in pf['annorect'] if _rect_has_points(r)]
        if len(p_rects) > AP_MAX_PRED or len(g_rects) > AP_MAX_GT:
            raise ValueError('pack_posetrack_frames: %s has %d predicted and %d annotated poses, the limits are %d and %d'
                             % (where, len(p_rects), len(g_rects), AP_MAX_PRED, AP_MAX_GT))
        for r in g_rects:
            row, has = _pack_points(r['annopoints'][0]['point'], where + ' (ground truth)', False, bool(regions))
            try:
                head = [_num(r[k][0], k, where) for k in ('x1', 'y1', 'x2', 'y2')]
            except KeyError as e:
                raise ValueError('pack_posetrack_frames: an annotated pose of %s has no %s (head rectangle)' % (where, e))
            gt_rows.append(row)
            gt_has.append(has)
            gt_head.append(head)
        for r in p_rects:
            row, has = _pack_points(r['annopoints'][0]['point'], where + ' (prediction)', True, bool(regions))
            pr_rows.append(row)
            pr_has.append(has)
        if seq_ids is not None:
            for rects, ids, out, side in ((g_rects, maps[0], gt_track, 'annotated'), (p_rects, maps[1], pr_track, 'predicted')):
                here = set()
                for r in rects:
                    tid = r.get('track_id')
                    if tid is None or len(tid) == 0:
                        raise ValueError('pack_posetrack_frames: a %s pose of %s has points but no track_id' % (side, where))
                    tid = tid[0]
                    if tid in here:
                        raise ValueError('pack_posetrack_frames: track id %r is listed twice among the %s poses of %s'
                                         % (tid, side, where))
                    here.add(tid)
                    out.append(ids.setdefault(tid, len(ids)))
            if len(maps[0]) > MOT_MAX_TRACKS:
                raise ValueError('pack_posetrack_frames: sequence %r has more than %d ground-truth tracks (at %s)'
                                 % (seq_ids[idx], MOT_MAX_TRACKS, where))
            frame_seq.append(seen[seq_ids[idx]])
        pr_seg.append(len(pr_rows))
        gt_seg.append(len(gt_rows))
        poly_seg.append(len(vert_seg) - 1)
        kept.append(idx)
    i32 = lambda a: np.asarray(a, dtype=np.int32)  # noqa: E731
    out = {'pr_xys': np.asarray(pr_rows, dtype=np.float64).reshape(-1, AP_JOINTS, 3), 'pr_has': i32(pr_has),
            'gt_xy': np.ascontiguousarray(np.asarray(gt_rows, dtype=np.float64).reshape(-1, AP_JOINTS, 3)[:, :, :2]),
            'gt_has': i32(gt_has),
            'gt_head': np.asarray(gt_head, dtype=np.float64).reshape(-1, 4), 'pr_seg': i32(pr_seg), 'gt_seg': i32(gt_seg),
            'poly_seg': i32(poly_seg), 'vert_seg': i32(vert_seg), 'verts': np.asarray(verts, dtype=np.float64).reshape(-1, 2),
            'frame_index': np.asarray(kept, dtype=np.int64)}
    if seq_ids is not None:
        frame_seq = i32(frame_seq)
        out.update({'gt_track': i32(gt_track), 'pr_track': i32(pr_track), 'frame_seq': frame_seq,
                    'seq_seg': i32(np.searchsorted(frame_seq, np.arange(len(seen) + 1)))})
    return out


def load_posetrack_dirs(gt_dir, pred_dir, with_seq=False):
    """-> (gt_annolists, pr_annolists) for `pack_posetrack_frames`: the `annolist` frames of every *.json file of gt_dir
    (sorted by name; the reference takes glob's order) and of the file of the same base name in pred_dir
    (eval_helpers.load_data_dir, :385-440).  IOError for a missing prediction file and ValueError for a prediction file
    with another number of frames, as the reference raises; ValueError for a file in the PoseTrack18 `images` /
    `annotations` layout: its conversion (poseval's convert.py) is out of scope.
    with_seq=True: -> (gt_annolists, pr_annolists, seq_ids), seq_ids the index of the file every frame came from (the
    reference's `seq_id`, load_data_dir :404): the third argument of `pack_posetrack_frames` for `posetrack_mota`."""
    gt_frames, pr_frames, seq_ids = [], [], []
    for seq, name in enumerate(sorted(f for f in os.listdir(gt_dir) if f.endswith('.json'))):
        pair = []
        for d in (gt_dir, pred_dir):
            path = osp.join(d, name)
            if not osp.exists(path):
                raise IOError('Prediction file ' + path + ' does not exist')
            with open(path) as fin:
                data = json.load(fin)
            if 'annolist' not in data:
                raise ValueError('load_posetrack_dirs: %s is not in the annolist layout; converting the PoseTrack18 '
                                 'images / annotations layout is out of scope' % path)
            pair.append(data['annolist'])
        if len(pair[0]) != len(pair[1]):
            raise ValueError('# prediction frames %d != # GT frames %d for %s'
                             % (len(pair[1]), len(pair[0]), osp.join(pred_dir, name)))
        seq_ids += [seq] * len(pair[0])
        gt_frames += pair[0]
        pr_frames += pair[1]
    return (gt_frames, pr_frames, seq_ids) if with_seq else (gt_frames, pr_frames)


def _get_cum(vals):
    """eval_helpers.getCum (:133-147): Head = mean(head_top, neck, nose), Shou, Elb, Wri, Hip, Knee, Ankl, Total."""
    groups = ((14, 12, 13), (8, 9), (7, 10), (6, 11), (2, 3), (1, 4), (0, 5))
    return [float(vals[list(g)].mean()) for g in groups] + [float(vals[AP_JOINTS])]


def posetrack_ap(frames, dist_thresh=0.5, device='cuda'):
    """PoseTrack AP of a packed set (`pack_posetrack_frames`) on the device: poseval's assignGTmulti + computeMetrics
    (csrc/posetrack_ap.hip; include/fami.h has the arithmetic).  Per frame the predicted poses are matched greedily to
    the annotated ones by PCKh at dist_thresh (after the ignore-region filter), per joint one precision / recall curve
    over the whole set gives the VOC AP.  All arithmetic is fp64.  Equal scores keep frame order, then pose order within
    the frame (a stable descending sort; the reference's `argsort()[::-1]` leaves them open).
    -> dict: 'ap', 'pre', 'rec' float64 [16] (per joint in PoseTrack order, x 100; entry 15 the mean over the non-NaN
    joints; a joint nobody predicts gives 0 and counts in the mean, one predicted but never annotated gives NaN and does
    not -- both as in the reference), 'names' [16], 'cum' (the 8 values of getCum of `ap`: Head, Shou, Elb, Wri, Hip,
    Knee, Ankl, Total), and for inspection 'label' [P] (bit j: joint j of the pose counts as a true positive), 'assigned'
    [P] (frame-local index of the annotated pose it took, -1 for none), 'ngt' [15], 'pr_has' [P] / 'gt_has' [G] (the masks
    left by the ignore-region filter).  One upload, two entry-point calls with one stable `torch.sort` between them, one
    download.  An empty set returns the reference's values (all zeros) without device work.  ValueError for more than
    458752 predicted poses in the set (the curve kernel's cap)."""
    F = len(frames['pr_seg']) - 1
    if F <= 0:
        return _ap_empty()
    dist_thresh, dev = _posetrack_check('posetrack_ap', frames, dist_thresh, device, ap=True, mot=False)
    return _ap_result(_posetrack_run('posetrack_ap', frames, dist_thresh, dev, ap=True, mot=False))


def _ap_empty():
    z = np.zeros(AP_JOINTS + 1)
    return {'ap': z.copy(), 'pre': z.copy(), 'rec': z.copy(), 'names': POSETRACK_JOINT + ['total'], 'cum': _get_cum(z),
            'label': np.zeros(0, np.int32), 'assigned': np.zeros(0, np.int32), 'ngt': np.zeros(AP_JOINTS, np.int32),
            'pr_has': np.zeros(0, np.int32), 'gt_has': np.zeros(0, np.int32)}


def _ap_result(raw):
    res = raw['res']
    return {'ap': res[0].copy(), 'pre': res[1].copy(), 'rec': res[2].copy(), 'names': POSETRACK_JOINT + ['total'],
            'cum': _get_cum(res[0]), 'label': raw['label'], 'assigned': raw['assigned'], 'ngt': raw['ngt'],
            'pr_has': raw['pr_has'], 'gt_has': raw['gt_has']}


def _posetrack_check(who, frames, dist_thresh, device, ap, mot):
    """What `posetrack_ap` / `posetrack_mota` refuse before any device work -> (dist_thresh, torch device)."""
    F, P, G = len(frames['pr_seg']) - 1, len(frames['pr_has']), len(frames['gt_has'])
    dist_thresh = float(dist_thresh)
    if not np.isfinite(dist_thresh):
        raise ValueError('%s: dist_thresh must be finite' % who)
    if ap and P > AP_MAX_SET:
        raise ValueError('%s: %d predicted poses, the limit is %d per set' % (who, P, AP_MAX_SET))
    n_pr, n_gt = np.diff(frames['pr_seg']), np.diff(frames['gt_seg'])
    m = _first_over(n_pr, AP_MAX_PRED, n_gt, AP_MAX_GT)
    if m is not None:
        raise ValueError('%s: kept frame %d has %d predicted and %d annotated poses, the limits are %d and %d'
                         % (who, m, n_pr[m], n_gt[m], AP_MAX_PRED, AP_MAX_GT))
    if mot:
        gt_track, pr_track = frames['gt_track'], frames['pr_track']
        if not _ascends(frames['seq_seg'], F):
            raise ValueError('%s: seq_seg must ascend from 0 to the %d kept frames' % (who, F))
        if len(gt_track) != G or len(pr_track) != P:
            raise ValueError('%s: gt_track / pr_track must have one entry per pose' % who)
        if G and (gt_track.min() < 0 or gt_track.max() >= MOT_MAX_TRACKS):
            raise ValueError('%s: annotated track ids must be in 0 .. %d (renumbered per sequence)' % (who, MOT_MAX_TRACKS - 1))
        if P and pr_track.min() < 0:
            raise ValueError('%s: predicted track ids must be >= 0' % who)
    return dist_thresh, _hip_device(who, device)


def _posetrack_run(who, frames, dist_thresh, dev, ap, mot):
    """One upload, fami_posetrack_assign_f64, then the curve (ap) and / or the MOT launches (mot) on what it wrote, one
    download -> the raw outputs."""
    F, P, G = len(frames['pr_seg']) - 1, len(frames['pr_has']), len(frames['gt_has'])
    NP, NV = len(frames['vert_seg']) - 1, len(frames['verts'])
    S = len(frames['seq_seg']) - 1 if mot else 0
    # the fp64 inputs, the int inputs, the int outputs, [the MOT step's int inputs and outputs,] then ap / pre / rec [and the MOT
    # step's fp64 outputs]; everything from the first output on comes back in one download
    fields = [(k, 'f64', frames[k].shape, frames[k]) for k in ('pr_xys', 'gt_xy', 'gt_head', 'verts')]
    fields += [(k, 'i32', frames[k].shape, frames[k]) for k in ('pr_has', 'gt_has', 'pr_seg', 'gt_seg', 'poly_seg', 'vert_seg')]
    fields += [('pr_has_out', 'i32', P), ('gt_has_out', 'i32', G), ('label', 'i32', P), ('assigned', 'i32', P),
               ('ngt_frame', 'i32', (F, AP_JOINTS)), ('ngt', 'i32', AP_JOINTS)]
    if mot:
        fields += [(k, 'i32', frames[k].shape, frames[k]) for k in ('pr_track', 'gt_track', 'seq_seg')]
        fields += [('counts', 'i32', (S, AP_JOINTS, 5)), ('status', 'i32', S), ('totals', 'i32', (AP_JOINTS, 5))]
    fields += [('res', 'f64', (3, AP_JOINTS + 1))]
    if mot:
        fields += [('sumd', 'f64', (S, AP_JOINTS)), ('sumd_tot', 'f64', AP_JOINTS), ('table', 'f64', (4, AP_JOINTS + 1))]
    w = _Words(dev, fields)
    with torch.cuda.device(dev):
        s = torch.cuda.current_stream(dev).cuda_stream
        lib().call('fami_posetrack_assign_f64', w.ptr('pr_xys'), w.ptr('pr_has'), w.ptr('gt_xy'), w.ptr('gt_has'),
                   w.ptr('gt_head'), w.ptr('pr_seg'), w.ptr('gt_seg'), w.ptr('poly_seg'), w.ptr('vert_seg'), w.ptr('verts'),
                   P, G, F, NP, NV, dist_thresh, w.ptr('pr_has_out'), w.ptr('gt_has_out'), w.ptr('label'), w.ptr('assigned'),
                   w.ptr('ngt_frame'), s)
        if ap:
            # plumbing between the two kernels: per joint, the predictions that still have it, by descending score
            if P:
                bits = torch.arange(AP_JOINTS, dtype=torch.int32, device=dev)[:, None]
                has_out, label = w.view('pr_has_out'), w.view('label')
                present = ((has_out[None, :] >> bits) & 1).bool()
                score = w.view('pr_xys').view(P, AP_JOINTS, 3)[:, :, 2].t()
                order = torch.sort(torch.where(present, score, score.new_tensor(float('-inf'))), dim=1, descending=True,
                                   stable=True).indices
                lab = ((label[order] >> bits) & 1).to(torch.uint8).contiguous()
                n_valid = present.sum(1, dtype=torch.int32).contiguous()
            else:                                                        # annotated poses only: 15 empty lists
                lab = torch.zeros(AP_JOINTS, dtype=torch.uint8, device=dev)
                n_valid = torch.zeros(AP_JOINTS, dtype=torch.int32, device=dev)
            lib().call('fami_posetrack_curve_f64', lab.data_ptr(), n_valid.data_ptr(), w.ptr('ngt_frame'), P, F, w.ptr('res'),
                       w.ptr('ngt'), s)
        if mot:
            # on the masks the assign launch wrote: the ignore filter runs once, and MOTA and AP see the same points
            lib().call('fami_posetrack_mot_f64', w.ptr('pr_xys'), w.ptr('pr_has_out'), w.ptr('gt_xy'), w.ptr('gt_has_out'),
                       w.ptr('gt_head'), w.ptr('pr_seg'), w.ptr('gt_seg'), w.ptr('poly_seg'), w.ptr('pr_track'),
                       w.ptr('gt_track'), w.ptr('seq_seg'), P, G, F, S, dist_thresh, w.ptr('counts'), w.ptr('sumd'),
                       w.ptr('status'), s)
            lib().call('fami_posetrack_mot_final_f64', w.ptr('counts'), w.ptr('sumd'), w.ptr('status'), S, w.ptr('totals'),
                       w.ptr('sumd_tot'), w.ptr('table'), s)
    out = w.download('pr_has_out')
    if (out['ngt_frame'] < 0).any():
        raise RuntimeError('%s: the kernel refused kept frame %d' % (who, int(np.argmax((out['ngt_frame'] < 0).any(1)))))
    if mot and out['status'].any():
        raise RuntimeError('%s: the kernel refused sequence %d' % (who, int(np.argmax(out['status'] != 0))))
    taken = ('pr_has_out', 'gt_has_out', 'label', 'assigned', 'ngt', 'res')
    if mot:
        taken += ('counts', 'totals', 'sumd', 'sumd_tot', 'table')
    raw = {k: out[k].copy() for k in taken}                                 # (copies: nothing returned holds the download)
    raw['pr_has'], raw['gt_has'] = raw.pop('pr_has_out'), raw.pop('gt_has_out')
    return raw


def evaluate_posetrack_ap(gt_dir, pred_dir, device='cuda'):
    """-> the 8 AP values Head, Shou, Elb, Wri, Hip, Knee, Ankl, Total: what the reference's
    `evaluate_simple.evaluate(gt_dir, pred_dir, eval_track=False)[0]` returns, in-process.  gt_dir holds the annolist
    ground-truth files, pred_dir the files of the same names -- the directory `write_posetrack_results` wrote to."""
    return posetrack_ap(pack_posetrack_frames(*load_posetrack_dirs(gt_dir, pred_dir)), device=device)['cum']


# ---------------------------------------------------------------------------------------- PoseTrack MOTA (poseval)
def _get_cum_mot(table):
    """printTable(metrics, motHeader=True) of evaluate_simple.py:33-47: the seven group means of MOTA, then the totals of
    MOTA, MOTP, Prec, Rec."""
    return _get_cum(table[0]) + [float(table[r][AP_JOINTS]) for r in (1, 2, 3)]


def _mot_result(table, totals, sumd_tot, per_seq):
    res = {k: table[r].copy() for r, k in enumerate(('mota', 'motp', 'pre', 'rec'))}
    res.update({k: totals[:, i].astype(np.int64) for i, k in enumerate(MOT_COUNTS)})
    res.update({'sum_d': sumd_tot, 'per_seq': per_seq, 'names': POSETRACK_JOINT + ['total'], 'cum': _get_cum_mot(table)})
    return res


def _mot_empty(S):
    nan, z = np.full(AP_JOINTS + 1, np.nan), np.zeros(AP_JOINTS + 1)
    return _mot_result(np.stack([nan, z, nan, nan]), np.zeros((AP_JOINTS, 5), np.int32), np.zeros(AP_JOINTS),
                       np.zeros((S, AP_JOINTS, 5), np.int32))


def _mot_keys(who, frames):
    if not all(k in frames for k in ('gt_track', 'pr_track', 'seq_seg')):
        raise ValueError('%s: the frames carry no track ids; pack them with pack_posetrack_frames(gt, pr, seq_ids)' % who)


def posetrack_mota(frames, dist_thresh=0.5, device='cuda'):
    """PoseTrack MOTA of a set packed WITH seq_ids (`pack_posetrack_frames(gt, pr, seq_ids)`) on the device: poseval's
    evaluateTracking -- the `mot` lists of assignGTmulti, motmetrics' MOTAccumulator.update per (sequence, joint), the
    five counts, computeMetrics (csrc/posetrack_mot.hip; include/fami.h has the rule).  Per sequence and joint the
    annotated poses (objects) are matched to the predicted ones (hypotheses) frame after frame at dist <= dist_thresh
    head sizes: an object first keeps the hypothesis it had, the rest is a minimum-cost assignment; a pair that
    contradicts the object's memory is a SWITCH, objects left are MISSes, hypotheses left FPs.  The last kept frame of
    every sequence is not evaluated (the reference's `imgidxs[:-1]`); a sequence with ONE kept frame, for which the
    reference raises IndexError, contributes nothing, like one with none.  A kept frame without a predicted or without
    an annotated rect counts one MISS, one FP and one object for every joint (the reference's dummy lists).  Where
    several assignments of a frame have equal cost (exact fp64 ties), which one is taken depends on the input alone and
    is otherwise unspecified, as the reference's is.
    -> dict: 'mota', 'motp', 'pre', 'rec' float64 [16] (per joint in PoseTrack order, x 100, entry 15 the mean over the
    non-NaN joints; a joint without objects has NaN mota and rec, one without detections motp 0), 'num_misses',
    'num_switches', 'num_false_positives', 'num_detections', 'num_objects' int64 [15], 'sum_d' float64 [15], 'per_seq'
    int32 [S,15,5] (the five counts in that order, per sequence), 'names' [16], 'cum' (the 11 values of the reference's
    MOT table: MOTA of Head, Shou, Elb, Wri, Hip, Knee, Ankl, then the totals of MOTA, MOTP, Prec, Rec).  One upload,
    the assign launch of `posetrack_ap` (for the ignore filter), the two MOT launches, one download.  An empty set
    returns the reference's values (NaN, motp 0) without device work.  ValueError for frames packed without seq_ids."""
    _mot_keys('posetrack_mota', frames)
    if len(frames['pr_seg']) - 1 <= 0:
        return _mot_empty(max(len(frames['seq_seg']) - 1, 0))
    dist_thresh, dev = _posetrack_check('posetrack_mota', frames, dist_thresh, device, ap=False, mot=True)
    raw = _posetrack_run('posetrack_mota', frames, dist_thresh, dev, ap=False, mot=True)
    return _mot_result(raw['table'], raw['totals'], raw['sumd_tot'], raw['counts'])


def evaluate_posetrack_mota(gt_dir, pred_dir, device='cuda'):
    """-> the 11 values of the reference's MOT table (`evaluate_simple.evaluate(gt_dir, pred_dir)[1]`), in-process; the
    directories as for `evaluate_posetrack_ap`, the predictions written with `write_posetrack_results(tracks=...)`."""
    gt, pr, seq = load_posetrack_dirs(gt_dir, pred_dir, with_seq=True)
    return posetrack_mota(pack_posetrack_frames(gt, pr, seq), device=device)['cum']


def evaluate_posetrack(gt_dir, pred_dir, eval_pose=True, eval_track=True, device='cuda'):
    """The drop-in for the reference's `evaluate_simple.evaluate(gt_dir, pred_dir, eval_pose, eval_track)` -> (cum,
    track_cum): the 8 AP values (NaN with eval_pose=False, as the reference prints them) and the 11 MOT values (None
    with eval_track=False).  One load, one pack, one upload, ONE assign launch shared by both halves, one download."""
    nan = [float('nan')] * 8
    if not eval_pose and not eval_track:
        return nan, None
    loaded = load_posetrack_dirs(gt_dir, pred_dir, with_seq=eval_track)
    frames = pack_posetrack_frames(*loaded)
    if len(frames['pr_seg']) - 1 <= 0:
        return (_ap_empty()['cum'] if eval_pose else nan), (_mot_empty(0)['cum'] if eval_track else None)
    dist_thresh, dev = _posetrack_check('evaluate_posetrack', frames, 0.5, device, ap=eval_pose, mot=eval_track)
    raw = _posetrack_run('evaluate_posetrack', frames, dist_thresh, dev, ap=eval_pose, mot=eval_track)
    return (_get_cum(raw['res'][0]) if eval_pose else nan), (_get_cum_mot(raw['table']) if eval_track else None)


# ---------------------------------------------------------------------------------------- COCO keypoint AP / AR (pycocotools)
COCO_IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)     # Params.setKpParams
COCO_REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
COCO_AREA_RNGS = np.array([[0 ** 2, 1e5 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]], dtype=np.float64)  # all, medium, large
COCO_MAX_DETS = 20
COCO_MAX_PER_IMAGE = 256        # csrc/coco_ap.hip: one thread per detection of an image (before the cut)
COCO_MAX_GT = 128               # ... the annotations of an image are LDS-resident
COCO_MAX_KEPT = 64              # ... the largest max_dets
COCO_MAX_SET = 229376           # ... two bits per kept detection of the set in 56 KiB of LDS
COCO_STAT_NAMES = ['AP', 'AP50', 'AP75', 'AP_M', 'AP_L', 'AR', 'AR50', 'AR75', 'AR_M', 'AR_L']


def _coco_rows(anns, what, J):
    """The keypoint lists of `anns` as one [n,J,3] float64 array (J: None = taken from the first list) -> (array, J)."""
    rows = []
    for i, a in enumerate(anns):
        k = a.get('keypoints')
        if k is None or not hasattr(k, '__len__'):
            raise ValueError('pack_coco_keypoints: %s %d has no keypoint list' % (what, i))
        if J is None:
            J = len(k) // 3
            if len(k) != 3 * J or not 1 <= J <= NMS_MAX_JOINTS:
                raise ValueError('pack_coco_keypoints: %s %d has %d keypoint values; 3 x J with J in 1 .. %d is supported'
                                 % (what, i, len(k), NMS_MAX_JOINTS))
        if len(k) != 3 * J:
            raise ValueError('pack_coco_keypoints: %s %d has %d keypoint values, not 3 x %d' % (what, i, len(k), J))
        rows.append(k)
    try:
        arr = np.asarray(rows, dtype=np.float64).reshape(-1, J or 1, 3)
    except (TypeError, ValueError):
        raise ValueError('pack_coco_keypoints: the keypoints of a %s are not numbers' % what)
    if not np.isfinite(arr).all():
        raise ValueError('pack_coco_keypoints: %s %d has a non-finite keypoint value'
                         % (what, int(np.argmax(~np.isfinite(arr).all(axis=(1, 2))))))
    return arr, J


def _coco_column(anns, key, what, width=None):
    """Field `key` of every dict as a float64 array ([n] or [n,width]); ValueError when missing, malformed or non-finite."""
    vals = []
    for i, a in enumerate(anns):
        if key not in a:
            raise ValueError('pack_coco_keypoints: %s %d has no %r' % (what, i, key))
        vals.append(a[key])
    try:
        arr = np.asarray(vals, dtype=np.float64).reshape((-1,) if width is None else (-1, width))
    except (TypeError, ValueError):
        raise ValueError('pack_coco_keypoints: %r of a %s is not %s' % (key, what, 'a number' if width is None else '%d numbers' % width))
    if len(arr) != len(anns) or not np.isfinite(arr).all():
        raise ValueError('pack_coco_keypoints: %r of a %s is not finite' % (key, what))
    return arr


def pack_coco_keypoints(gt_anns, dt_anns, img_ids=None):
    """A COCO keypoint evaluation set as the flat fp64 / int32 arrays `coco_keypoint_ap` uploads.  gt_anns: COCO annotation
    dicts (`image_id`, `keypoints` [3 J: x, y, v], `area`, `bbox` [x, y, w, h]; optional `iscrowd`, `num_keypoints`,
    `category_id`); dt_anns: result dicts (`image_id`, `keypoints` [3 J: x, y, confidence], `score`; optional
    `category_id`).  What pycocotools' loadRes / _prepare do to them is done here: ignore = iscrowd or num_keypoints == 0
    (a missing `iscrowd` counts as 0, a missing `num_keypoints` is the number of v > 0; an `ignore` field of the input is
    not read, as _prepare overwrites it); a detection's area is that of the bounding box of its J (x, y) pairs, in float64.
    Images are taken in ascending `image_id`; img_ids (default: every id that occurs) names the images to evaluate --
    annotations and detections of other images are left out, an id without either is legal.
    -> dict: gt_kpts [G,J,3], gt_area [G], gt_bbox [G,4], gt_flags [G] int32 (bit 0 ignore, bit 1 iscrowd), dt_kpts [D,J,3],
    dt_score [D], dt_area [D], gt_seg / dt_seg [M+1] int32 (image m owns the rows seg[m] .. seg[m+1), list order kept),
    image_ids [M], gt_index [G] / dt_index [D] (the position of every packed row in the inputs), num_joints.
    ValueError for: a keypoint list that is not 3 J long (J from the first list, 1 .. 32), non-finite keypoints, scores,
    areas or boxes, a missing `area` / `bbox` on an annotation, a missing `score` or `image_id`, more than one distinct
    `category_id`, more than 128 annotations or 256 detections in an image.  Neither input is modified."""
    gt_anns, dt_anns = list(gt_anns), list(dt_anns)
    for what, anns in (('annotation', gt_anns), ('detection', dt_anns)):
        for i, a in enumerate(anns):
            if 'image_id' not in a:
                raise ValueError('pack_coco_keypoints: %s %d has no image_id' % (what, i))
    cats = {a['category_id'] for a in gt_anns + dt_anns if 'category_id' in a}
    if len(cats) > 1:
        raise ValueError('pack_coco_keypoints: one category is supported, the set names %d (%s)'
                         % (len(cats), ', '.join(sorted(map(repr, cats))[:4])))
    ids = sorted({a['image_id'] for a in gt_anns + dt_anns}) if img_ids is None else sorted(set(img_ids))
    number = {v: i for i, v in enumerate(ids)}
    M = len(ids)

    def group(anns):
        """-> (positions of the listed images' dicts, grouped by image in list order; seg [M+1])"""
        img = np.asarray([number.get(a['image_id'], -1) for a in anns], dtype=np.int64)
        pos = np.flatnonzero(img >= 0)
        pos = pos[np.argsort(img[pos], kind='stable')]
        return pos, np.searchsorted(img[pos], np.arange(M + 1)).astype(np.int32)

    gpos, gt_seg = group(gt_anns)
    dpos, dt_seg = group(dt_anns)
    gts, dts = [gt_anns[i] for i in gpos], [dt_anns[i] for i in dpos]
    for seg, cap, what in ((gt_seg, COCO_MAX_GT, 'annotations'), (dt_seg, COCO_MAX_PER_IMAGE, 'detections')):
        n = np.diff(seg)
        if M and n.max() > cap:
            raise ValueError('pack_coco_keypoints: image %r has %d %s, the limit is %d per image'
                             % (ids[int(n.argmax())], n.max(), what, cap))
    gt_kpts, J = _coco_rows(gts, 'annotation', None)
    dt_kpts, J = _coco_rows(dts, 'detection', J)
    J = J or len(COCO_SIGMAS)
    gt_kpts, dt_kpts = gt_kpts.reshape(-1, J, 3), dt_kpts.reshape(-1, J, 3)
    gt_area, gt_bbox = _coco_column(gts, 'area', 'annotation'), _coco_column(gts, 'bbox', 'annotation', 4)
    dt_score = _coco_column(dts, 'score', 'detection')
    crowd = np.asarray([bool(g.get('iscrowd', 0)) for g in gts], dtype=bool)
    labelled = (gt_kpts[:, :, 2] > 0).sum(1)
    nk = np.asarray([g['num_keypoints'] if 'num_keypoints' in g else int(labelled[i]) for i, g in enumerate(gts)], dtype=np.float64)
    ignore = crowd | (nk.reshape(-1) == 0)
    x, y = dt_kpts[:, :, 0], dt_kpts[:, :, 1]
    dt_area = (x.max(1) - x.min(1)) * (y.max(1) - y.min(1)) if len(dts) else np.zeros(0)
    return {'gt_kpts': gt_kpts, 'gt_area': gt_area, 'gt_bbox': gt_bbox,
            'gt_flags': (ignore.astype(np.int32) | (crowd.astype(np.int32) << 1)).astype(np.int32),
            'dt_kpts': dt_kpts, 'dt_score': dt_score, 'dt_area': np.ascontiguousarray(dt_area, dtype=np.float64),
            'gt_seg': gt_seg, 'dt_seg': dt_seg, 'image_ids': ids, 'gt_index': gpos, 'dt_index': dpos, 'num_joints': J}


def _coco_summarize(precision, recall, iou_thrs):
    """COCOeval.summarize for keypoints (_summarizeKps): means over the entries > -1, -1 where there is none."""
    def one(s, thr, a):
        if a >= s.shape[-1]:
            return -1.0
        if thr is not None:
            s = s[np.where(thr == iou_thrs)[0]]
        s = s[..., a]
        s = s[s > -1]
        return -1.0 if s.size == 0 else float(np.mean(s))
    return np.array([one(s, thr, a) for s in (precision, recall)
                     for thr, a in ((None, 0), (.5, 0), (.75, 0), (None, 1), (None, 2))], dtype=np.float64)


def _coco_thresholds(J, max_dets, sigmas, iou_thrs, rec_thrs, area_rngs):
    who = 'coco_keypoint_ap'
    _int_option(who, 'max_dets must be an integer in 1 .. %d' % COCO_MAX_KEPT, max_dets, 1, COCO_MAX_KEPT)
    sig = _sigmas(who, J, sigmas, 'the set', np.float64)
    iou = np.ascontiguousarray(COCO_IOU_THRS if iou_thrs is None else iou_thrs, dtype=np.float64).reshape(-1)
    rec = np.ascontiguousarray(COCO_REC_THRS if rec_thrs is None else rec_thrs, dtype=np.float64).reshape(-1)
    rng = np.ascontiguousarray(COCO_AREA_RNGS if area_rngs is None else area_rngs, dtype=np.float64)
    if not 1 <= iou.size <= 32 or not 1 <= rec.size <= 256 or rng.ndim != 2 or rng.shape[1] != 2 or not 1 <= rng.shape[0] <= 8:
        raise ValueError('%s: 1 .. 32 iou_thrs, 1 .. 256 rec_thrs and 1 .. 8 area_rngs [A,2] are supported' % who)
    if not (np.isfinite(iou).all() and np.isfinite(rec).all() and np.isfinite(rng).all()):
        raise ValueError('%s: thresholds must be finite' % who)
    return int(max_dets), np.ascontiguousarray((sig * 2) ** 2), iou, rec, rng


def _coco_result(precision, recall, iou, num_kept):
    return {'stats': _coco_summarize(precision, recall, iou), 'names': list(COCO_STAT_NAMES), 'precision': precision,
            'recall': recall, 'num_kept': num_kept}


def coco_keypoint_ap(packed, max_dets=COCO_MAX_DETS, sigmas=None, iou_thrs=None, rec_thrs=None, area_rngs=None, device='cuda'):
    """COCO keypoint AP / AR of a packed set (`pack_coco_keypoints`) on the device: pycocotools'
    `COCOeval(gt, dt, 'keypoints')` evaluate + accumulate + summarize for one category (csrc/coco_ap.hip; include/fami.h
    restates the definition in full).  Per image the detections are ranked by score (equal scores keep list order), the
    first max_dets kept and matched greedily to the annotations by OKS, once per area range and OKS threshold, with
    pycocotools' crowd / ignore rules; per (range, threshold) one precision / recall curve over the set, read at the recall
    thresholds.  All arithmetic is fp64.  Defaults: COCO_SIGMAS (J = 17; any other J needs its own sigmas), COCO_IOU_THRS
    (.5 : .05 : .95), COCO_REC_THRS (0 : .01 : 1), COCO_AREA_RNGS (all, medium, large), max_dets 20 -- the threshold arrays
    are numpy's, handed down as they are.
    -> dict: 'stats' float64 [10] (AP, AP50, AP75, AP_M, AP_L, AR, AR50, AR75, AR_M, AR_L: COCOeval.stats; -1 where
    nothing counts, e.g. no annotation of that size, a threshold .5 / .75 that iou_thrs does not hold, or fewer than three
    area ranges), 'names', 'precision' [T,R,A], 'recall' [T,A] (-1 where a range holds no annotation that counts),
    'num_kept' (detections after the cut).  pycocotools' `scores` array is not produced, and "matched" is a flag, not the
    annotation's id (pycocotools never counts a match to an annotation with id 0).
    One upload, the match launch, one stable `torch.sort` plus gather, the curve launch, one download.  An empty set (no
    image, or neither annotations nor detections) returns all -1 without device work.  ValueError before any device work
    for max_dets outside 1 .. 64, sigmas that do not fit, non-finite or too many thresholds, an image over a cap, more
    than 229376 kept detections in the set."""
    J = int(packed['num_joints'])
    K, var, iou, rec, rng = _coco_thresholds(J, max_dets, sigmas, iou_thrs, rec_thrs, area_rngs)
    T, R, A = iou.size, rec.size, rng.shape[0]
    gt_seg, dt_seg = np.asarray(packed['gt_seg'], dtype=np.int32), np.asarray(packed['dt_seg'], dtype=np.int32)
    M, G, D = len(gt_seg) - 1, len(packed['gt_flags']), len(packed['dt_score'])
    if M <= 0 or G + D == 0:
        return _coco_result(-np.ones((T, R, A)), -np.ones((T, A)), iou, 0)
    if len(dt_seg) != M + 1 or not _ascends(gt_seg, G) or not _ascends(dt_seg, D):
        raise ValueError('coco_keypoint_ap: gt_seg / dt_seg must ascend from 0 to the %d annotations / %d detections' % (G, D))
    n_gt, n_dt = np.diff(gt_seg), np.diff(dt_seg)
    m = _first_over(n_gt, COCO_MAX_GT, n_dt, COCO_MAX_PER_IMAGE)
    if m is not None:
        raise ValueError('coco_keypoint_ap: image %d has %d annotations and %d detections, the limits are %d and %d'
                         % (m, n_gt[m], n_dt[m], COCO_MAX_GT, COCO_MAX_PER_IMAGE))
    kept = np.minimum(n_dt, K)
    N = int(kept.sum())
    if N > COCO_MAX_SET:
        raise ValueError('coco_keypoint_ap: %d detections after the cut, the limit is %d per set' % (N, COCO_MAX_SET))
    if M * K * A * T > 0x7fffffff or max(G, D) * J * 3 > 0x7fffffff:
        raise ValueError('coco_keypoint_ap: the set is too large for 32-bit indices')
    dev = _hip_device('coco_keypoint_ap', device)
    # the kept slots of every image, as the match launch lays them out: m * K + k for k < min(detections of m, K)
    first = np.concatenate([[0], np.cumsum(kept)[:-1]])
    slots = (np.repeat(np.arange(M, dtype=np.int64) * K - first, kept) + np.arange(N, dtype=np.int64)).astype(np.int32)
    f64 = {k: np.ascontiguousarray(packed[k], dtype=np.float64).reshape(-1)
           for k in ('gt_kpts', 'gt_area', 'gt_bbox', 'dt_kpts', 'dt_score', 'dt_area')}
    gt_flags = np.ascontiguousarray(packed['gt_flags'], dtype=np.int32).reshape(-1)
    if [a.size for a in f64.values()] != [G * J * 3, G, G * 4, D * J * 3, D, D]:
        raise ValueError('coco_keypoint_ap: the packed arrays do not fit %d annotations and %d detections of %d joints' % (G, D, J))
    if not all(np.isfinite(a).all() for a in f64.values()):
        raise ValueError('coco_keypoint_ap: the packed arrays must be finite')
    # the fp64 inputs, then the int inputs: inputs only (the outputs are torch.empty tensors of their own: in here they would be
    # megabytes of uploaded zeros).  Two spare words have always followed `slots`; the pinned buffer length keeps them.
    w = _Words(dev, [(k, 'f64', a.size, a) for k, a in f64.items()] +
               [('gt_flags', 'i32', gt_flags.size, gt_flags), ('gt_seg', 'i32', M + 1, gt_seg), ('dt_seg', 'i32', M + 1, dt_seg),
                ('slots', 'i32', N, slots), ('spare', 'i32', 2)])
    with torch.cuda.device(dev):
        s = torch.cuda.current_stream(dev).cuda_stream
        out_score = torch.empty(M * K, dtype=torch.float64, device=dev)
        out_row = torch.empty(M * K, dtype=torch.int32, device=dev)
        out_flags = torch.empty(M * K, A * T, dtype=torch.uint8, device=dev)
        npig = torch.empty(M * A, dtype=torch.int32, device=dev)
        res = torch.empty(T * R * A + T * A + 1, dtype=torch.float64, device=dev)
        lib().call('fami_coco_kpt_match_f64', w.ptr('gt_kpts'), w.ptr('gt_area'), w.ptr('gt_bbox'), w.ptr('gt_flags'),
                   w.ptr('dt_kpts'), w.ptr('dt_score'), w.ptr('dt_area'), w.ptr('gt_seg'), w.ptr('dt_seg'), var.ctypes.data,
                   iou.ctypes.data, rng.ctypes.data, G, D, M, J, T, A, K, out_score.data_ptr(), out_row.data_ptr(),
                   out_flags.data_ptr(), npig.data_ptr(), s)
        # plumbing between the two kernels: the kept detections of the whole set by descending score, images in order
        slot = w.view('slots').long()
        order = torch.sort(out_score[slot], descending=True, stable=True).indices
        flags = out_flags[slot[order]].t().contiguous()
        lib().call('fami_coco_kpt_curve_f64', flags.data_ptr() if N else None, npig.data_ptr(), rec.ctypes.data, N, M, T, A, R,
                   res.data_ptr(), res.data_ptr() + 8 * T * R * A, s)
        res[-1:] = npig.min().to(torch.float64)                   # the refusal marker rides in the one download
    out = res.cpu().numpy()
    if out[-1] < 0:
        raise RuntimeError('coco_keypoint_ap: the kernel refused an image')
    return _coco_result(out[:T * R * A].reshape(T, R, A).copy(), out[T * R * A:T * R * A + T * A].reshape(T, A).copy(), iou, N)


def load_coco_keypoints(gt_json, dt_json):
    """-> (gt_anns, dt_anns, img_ids), the arguments of `pack_coco_keypoints`: the `annotations` of an instances-style
    ground-truth file (person_keypoints_*.json) with the ids of its `images` (None when the file lists none: then every
    id that occurs is evaluated), and the list a results file holds.  As COCO.loadRes, ValueError for a results file that
    is not a list or that names an image the ground truth does not list."""
    with open(gt_json) as f:
        gt = json.load(f)
    with open(dt_json) as f:
        dt = json.load(f)
    if not isinstance(gt, dict) or 'annotations' not in gt:
        raise ValueError('load_coco_keypoints: %s has no `annotations`' % gt_json)
    if not isinstance(dt, list):
        raise ValueError('load_coco_keypoints: %s is not a list of results' % dt_json)
    img_ids = [im['id'] for im in gt['images']] if 'images' in gt else None
    if img_ids is not None:
        extra = {r.get('image_id') for r in dt} - set(img_ids)
        if extra:
            raise ValueError('load_coco_keypoints: results name %d images the ground truth does not list (e.g. %r)'
                             % (len(extra), sorted(extra, key=repr)[0]))
    return gt['annotations'], dt, img_ids


def evaluate_coco_keypoints(gt_json, dt_json, device='cuda', **kw):
    """-> the 10 values of `COCOeval(cocoGt, cocoGt.loadRes(dt_json), 'keypoints')` after evaluate / accumulate /
    summarize (`.stats`: AP, AP50, AP75, AP_M, AP_L, AR, AR50, AR75, AR_M, AR_L), in-process; keywords as for
    `coco_keypoint_ap`."""
    return coco_keypoint_ap(pack_coco_keypoints(*load_coco_keypoints(gt_json, dt_json)), device=device, **kw)['stats']


def coco_keypoint_results(preds, boxes, image_ids, keep=None, category_id=1):
    """The result dicts HRNet's COCO evaluation writes, for `pack_coco_keypoints` or `json.dump`: preds [N,J,3] (x, y,
    confidence in image pixels) and boxes [N,6] (column 5 the score: rescored by `pose_nms` where that ran) as
    `EvalAccumulator` holds them, image_ids [N] the COCO image id of every row.  keep: the rows to write, in that order --
    the keep map of `pose_nms` (its lists are flattened in its order) or a flat list of row indices; default every row.
    -> [{'image_id', 'category_id', 'keypoints': [x, y, confidence] x J, 'score'}]."""
    preds, boxes = np.asarray(preds, dtype=np.float64), np.asarray(boxes, dtype=np.float64)
    if preds.ndim != 3 or preds.shape[2] != 3 or boxes.ndim != 2 or boxes.shape[1] != 6 or boxes.shape[0] != preds.shape[0]:
        raise ValueError('coco_keypoint_results expects preds [N,J,3] and boxes [N,6], got %s and %s' % (preds.shape, boxes.shape))
    image_ids = list(image_ids)
    if len(image_ids) != len(preds):
        raise ValueError('coco_keypoint_results: %d rows, %d image_ids' % (len(preds), len(image_ids)))
    if keep is None:
        rows = range(len(preds))
    else:
        rows = [int(i) for v in keep.values() for i in v] if hasattr(keep, 'values') else [int(i) for i in keep]
        if rows and not (0 <= min(rows) and max(rows) < len(preds)):
            raise ValueError('coco_keypoint_results: keep names a row outside [0, %d)' % len(preds))
    ids = [i.item() if isinstance(i, np.generic) else i for i in image_ids]
    return [{'image_id': ids[i], 'category_id': category_id, 'keypoints': preds[i].reshape(-1).tolist(),
             'score': float(boxes[i, 5])} for i in rows]
