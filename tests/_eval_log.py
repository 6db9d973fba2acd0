"""A record of the library launches one public function of fami_pose_amd.evaluate makes, in a form two source trees can
be compared by: the entry points in order, every argument, and where in the ONE uploaded word buffer each pointer lands.

The recorder depends only on what every tree has.  `lib().call` is wrapped on the instance and `torch.from_numpy` on the
module while the function runs.  The word buffer is the largest array handed to `torch.from_numpy` inside the call, and the
first pointer argument of the first launch is its first byte (true of pose_nms, pose_track, the PoseTrack run and
coco_keypoint_ap alike).  One record is {'words': length of the buffer in 4-byte words, 'calls': [[name, [arguments],
stream]]}:
* integers exactly, floats as float.hex();
* pointers as symbols: 'NULL', 'buf+<byte offset>' for a pointer into the word buffer, 'other' for anything else (torch
  temporaries, the host threshold arrays of the COCO match launch);
* the stream (the last argument of an entry point whose prototype ends in fami_stream_t) as 'current' or 'other'.

CASES holds the small seeded inputs of tests/test_eval_launches_gpu.py, built from the makers the evaluation tests already
have; each is a function (ev, dev, tmp_path) -> None that makes exactly one public call."""
import contextlib
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ap_ref as ar  # noqa: E402
import _coco_ref as cr  # noqa: E402
import _mota_ref as mr  # noqa: E402
import _nms_ref as nr  # noqa: E402
import _track_ref as tr  # noqa: E402
from _launch_log import _with_stream  # noqa: E402


@contextlib.contextmanager
def recording(dev):
    """-> a dict that holds the record of everything launched inside the block once the block has ended."""
    from fami_pose_amd._lib import lib
    L, raw, words, streamed, rec = lib(), [], [0], _with_stream(), {}
    call, from_numpy = L.call, torch.from_numpy

    def note(name, args):
        types = L.protos[name][1]
        assert len(types) == len(args), name
        stream = None
        if name in streamed:
            stream = 'current' if (args[-1] or 0) == torch.cuda.current_stream(dev).cuda_stream else 'other'
            args, types = args[:-1], types[:-1]
        raw.append((name, list(zip(args, types)), stream))

    def uploaded(a):
        words[0] = max(words[0], a.nbytes // 4)
        return from_numpy(a)

    L.call = lambda name, *a: (note(name, a), call(name, *a))[1]
    torch.from_numpy = uploaded
    try:
        yield rec
    finally:
        del L.call
        torch.from_numpy = from_numpy
    base = next((a for a, t in raw[0][1] if t is ctypes.c_void_p), None) if raw else None

    def symbol(ptr):
        if not ptr:
            return 'NULL'
        if base is not None and base <= ptr < base + 4 * words[0]:
            return 'buf+%d' % (ptr - base)
        return 'other'

    rec['words'] = words[0]
    rec['calls'] = [[name, [symbol(a) if t is ctypes.c_void_p else float(a).hex() if t in (ctypes.c_float, ctypes.c_double)
                            else int(a) for a, t in args], stream] for name, args, stream in raw]


def record(key, dev, tmp_path):
    """the record of case `key`, as json.load would return it"""
    from fami_pose_amd import evaluate as ev
    with recording(dev) as rec:
        CASES[key](ev, dev, str(tmp_path))
    torch.cuda.synchronize(dev)
    return json.loads(json.dumps(rec))


# ---------------------------------------------------------------------------------------- the cases
def _nms_set(J, seed=3):
    """three images of 0, 1 and 4 detections in N = 6 rows: row 5 is listed by no image"""
    rng = np.random.RandomState(seed)
    preds, boxes, fmap, i = rng.uniform(0.3, 1.0, (6, J, 3)), rng.uniform(0.3, 1.0, (6, 6)), {}, 0
    for m, n in enumerate((0, 1, 4)):
        k, a, b = nr.make_dets(rng, n, J=J)
        preds[i:i + n], boxes[i:i + n, 4], boxes[i:i + n, 5] = k, a, b
        fmap['/d/images/val/a/%08d.jpg' % (m + 1)] = list(range(i, i + n))
        i += n
    return preds, boxes, fmap


def _track_set(seed=2):
    """two videos of 2 and 1 frames, 2 and 1 people, N = 6 with one row that no image lists"""
    rng = np.random.RandomState(seed)
    videos = {'val/a': tr.make_video(rng, 2, [4, 5], drop=0, fp_rate=0), 'val/b': tr.make_video(rng, 1, [9], drop=0, fp_rate=0)}
    preds, boxes, fmap = tr.scatter(rng, videos, 17, spare=1)
    assert len(preds) == 6 and len(fmap) == 3
    return preds, boxes, fmap


def _person(rng):
    xy, _, head, size = ar.make_person(rng, 1.0)
    return xy, head, size


def _ap_frames(seed=4, predictions=True, polygon=True):
    """three frames of two annotated people: frame 1 has an ignore polygon (a triangle far from everybody), frame 2 no
    predicted pose; predictions=False: annotated poses only (P = 0); polygon=False: no ignore region, which leaves an odd
    number of 4-byte words in front of the fp64 outputs (the one case with a padding word)"""
    rng = np.random.RandomState(seed)
    gt, pr = [], []
    for f in range(3):
        people = [_person(rng) for _ in range(2)]
        g = {'annorect': [ar.gt_rect(xy, np.ones(ar.J, bool), head, i) for i, (xy, head, _) in enumerate(people)]}
        if f == 1 and polygon:
            g['ignore_regions'] = [{'point': [{'x': [x], 'y': [y]} for x, y in ((5000.0, 5000.0), (5100.0, 5000.0), (5000.0, 5100.0))]}]
        p = [ar.pr_rect(*ar.make_prediction(rng, xy, size, 0.2, 1.0), track_id=i) for i, (xy, _, size) in enumerate(people)]
        gt.append(g)
        pr.append({'annorect': p if predictions and f != 2 else []})
    return gt, pr


def _mota_set(seed=5):
    """two sequences of 3 and 1 kept frames"""
    gt, pr, seq = mr.make_sequences(np.random.RandomState(seed), 2, (3, 1), p_unannotated=0.0)
    for g in gt:                                                   # (a person who has left must not empty a frame)
        assert any(r['annopoints'] for r in g['annorect'])
    return gt, pr, seq


def _coco_set(seed=6, detections=True):
    """three images: 1 has two people and three detections, 2 one person and no detection, 3 a detection and no annotation"""
    rng = np.random.default_rng(seed)
    g = [cr.person(rng, 100, 100, 120, image_id=1, area=5000.0), cr.person(rng, 400, 300, 200, image_id=1, area=12000.0),
         cr.person(rng, 300, 200, 120, image_id=2, area=5000.0)]
    d = [cr.det_of(g[0], .9, rng, noise=0.05), cr.det_of(g[1], .8, rng, noise=0.05), cr.det_of(g[0], .4, rng, noise=0.15),
         dict(cr.det_of(g[2], .7, rng, noise=0.05), image_id=3)]
    return g, d if detections else [], [1, 2, 3]


def _nms(J, sigmas=None, **kw):
    def run(ev, dev, tmp):
        ev.pose_nms(*_nms_set(J), sigmas=sigmas, device=dev, **kw)
    return run


def _track(**kw):
    def run(ev, dev, tmp):
        ev.pose_track(*_track_set(), device=dev, **kw)
    return run


def _ap(**kw):
    def run(ev, dev, tmp):
        ev.posetrack_ap(ev.pack_posetrack_frames(*_ap_frames(**kw)), device=dev)
    return run


def _mota(ev, dev, tmp):
    frames = ev.pack_posetrack_frames(*_mota_set())
    assert frames['seq_seg'].tolist() == [0, 3, 4]
    ev.posetrack_mota(frames, device=dev)


def _both(ev, dev, tmp):
    """`evaluate_posetrack` with both halves on, from annolist files: the only path with ap and mot together"""
    gt, pr, seq = _mota_set()
    for d in ('gt', 'pr'):
        os.makedirs(os.path.join(tmp, d))
    for s in sorted(set(seq)):
        for d, frames in (('gt', gt), ('pr', pr)):
            with open(os.path.join(tmp, d, 'seq%02d.json' % s), 'w') as f:
                json.dump({'annolist': [fr for fr, q in zip(frames, seq) if q == s]}, f)
    ev.evaluate_posetrack(os.path.join(tmp, 'gt'), os.path.join(tmp, 'pr'), device=dev)


def _coco(detections=True, **kw):
    def run(ev, dev, tmp):
        ev.coco_keypoint_ap(ev.pack_coco_keypoints(*_coco_set(detections=detections)), device=dev, **kw)
    return run


CASES = {
    'pose_nms-j17-hard': _nms(17),
    'pose_nms-j17-soft': _nms(17, soft=True, max_dets=2, vis_thre=0.1),
    'pose_nms-j5': _nms(5, sigmas=np.array([.26, .35, .79, 1.07, .89]) / 10.0),
    'pose_track': _track(),
    'pose_track-vis': _track(vis_thre=0.3),
    'posetrack_ap': _ap(),
    'posetrack_ap-no-predictions': _ap(predictions=False),
    'posetrack_ap-no-polygon': _ap(polygon=False),
    'posetrack_mota': _mota,
    'evaluate_posetrack': _both,
    'coco_keypoint_ap': _coco(),
    'coco_keypoint_ap-cut': _coco(max_dets=2, iou_thrs=[.5, .75], rec_thrs=[0., .5, 1.], area_rngs=[[0., 1e10]]),
    'coco_keypoint_ap-no-detections': _coco(detections=False),
}


def main(argv):
    """python tests/_eval_log.py --record <commit hash> [fixture path]: record every case on the package this tree holds
    (for the fixture: the named commit's fami-pose_amd/evaluate.py in place) and write tests/golden/eval_launches.json."""
    import tempfile
    if len(argv) < 2 or argv[0] != '--record':
        raise SystemExit(main.__doc__)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = argv[2] if len(argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'eval_launches.json')
    data, dev = {'recorded_on_commit': argv[1], 'cases': {}}, torch.device('cuda:0')
    for key in CASES:
        with tempfile.TemporaryDirectory() as tmp:
            data['cases'][key] = record(key, dev, tmp)
        print(key, 'words', data['cases'][key]['words'])
        for row in data['cases'][key]['calls']:
            print('   ', row)
    with open(out, 'w') as f:
        json.dump(data, f, indent=0, sort_keys=True)
        f.write('\n')
    print('recorded %d cases on %s' % (len(data['cases']), argv[1]))


if __name__ == '__main__':
    main(sys.argv[1:])
