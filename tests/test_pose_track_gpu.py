"""OKS pose tracking on the MI355X (csrc/track.hip: fami_pose_track_f32; evaluate.pose_track / EvalAccumulator.pose_track /
write_posetrack_results(tracks=...)) against the float64 restatement tests/_track_ref.py.

Bounds.  There are none to choose: `tracks` and `num_tracks` must be EQUAL.  What can differ between the kernel and the
restatement is an OKS in its last bits (the device's fp64 exp against numpy's, the order of a sum: ~1e-16 relative), so
equality is demanded of inputs on which no decision is that close: every set is seeded, and the restatement's smallest
decision margin on it is asserted to be >= 1e-4 (tests/test_pose_track_host.py does so on the CPU; the cases are asserted
again here before anything is launched).  The seeds were chosen on the CPU so that this holds.

Shapes (tests/_track_ref.py builds them, the host test asserts what they contain): J = 17 with the default sigmas, J = 15
with its own, J = 1 and J = 32 (more than 64 KiB of LDS); with and without vis_thre; max_gap 1, 2 and 3; frames of 1, 63,
64, 65 and 256 detections (the wave boundary and the cap), a crowd of about 70 over five frames; a video of one frame, a
video whose only list is empty, rows that no image lists; V = 1 and V = 40, videos interleaved and frames out of order in
the map."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _nms_ref as nr  # noqa: E402
import _track_ref as tr  # noqa: E402

from fami_pose_amd import evaluate as ev  # noqa: E402
from fami_pose_amd._lib import lib  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 256
SENT = 0x5a5a5a5a


def _raw(dev, preds, boxes, fmap, sigmas=None, oks_thre=0.3, max_gap=3, vis_thre=None, tables=None):
    """The entry point itself on the tables of `fmap` (or on `tables`, unchecked), the outputs inside poisoned guard
    zones -> (track [N], ntracks [V], guards intact?, videos).  track is NOT pre-filled: unlisted rows keep the poison."""
    N, J = preds.shape[:2]
    index, fseg, fnum, vseg, videos = ev._track_tables(fmap, N) if tables is None else tables
    M, V, n = len(fnum), len(vseg) - 1, len(index)
    sig = ev.COCO_SIGMAS if sigmas is None else sigmas
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)  # noqa: E731
    ins = [up(preds, np.float32), up(boxes[:, 4], np.float32), up(sig, np.float32), up(np.concatenate([index, [0]]), np.int32),
           up(fseg, np.int32), up(fnum, np.int32), up(vseg, np.int32)]
    outs = [torch.full((GUARD + k + GUARD,), SENT, dtype=torch.int32, device=dev) for k in (N, V)]
    lib().call('fami_pose_track_f32', *[t.data_ptr() for t in ins], N, J, n, M, V, float(oks_thre), int(max_gap),
               0.0 if vis_thre is None else float(vis_thre), 0 if vis_thre is None else 1,
               *[t[GUARD:].data_ptr() for t in outs], torch.cuda.current_stream(dev).cuda_stream)
    res = [t.cpu().numpy() for t in outs]
    intact = all((r[:GUARD] == SENT).all() and (r[GUARD + k:] == SENT).all() for r, k in zip(res, (N, V)))
    return res[0][GUARD:GUARD + N], res[1][GUARD:GUARD + V], intact, videos


# ---------------------------------------------------------------------------------------- 1. against float64
@pytest.mark.parametrize('n', range(len(tr.CASE_IDS)), ids=tr.CASE_IDS)
def test_against_the_restatement(dev, n):
    c = tr.cases()[n]
    ref, fmap = c['ref'], c['fmap']
    assert ref['margin'] >= tr.MARGIN
    runs = [ev.pose_track(c['preds'], c['boxes'], fmap, sigmas=c['sigmas'], device=dev, **c['kw']) for _ in range(2)]
    tracks, num = runs[0]
    assert tracks.dtype == np.int32 and tracks.shape == (len(c['preds']),)
    assert num == ref['num_tracks'] and list(num) == list(ref['num_tracks'])          # the videos, by their first key
    assert np.array_equal(tracks, ref['tracks'])
    assert np.array_equal(runs[1][0], tracks) and runs[1][1] == num                   # two runs: bit for bit
    # the raw outputs: words behind `track` and `ntracks` unchanged, rows that no image lists untouched
    listed = np.zeros(len(tracks), bool)
    listed[np.concatenate([np.asarray(v, np.int64) for v in fmap.values()])] = True
    raw, cnt, intact, videos = _raw(dev, c['preds'], c['boxes'], fmap, c['sigmas'], **c['kw'])
    assert intact
    assert np.array_equal(raw[listed], ref['tracks'][listed]) and (raw[~listed] == SENT).all()
    assert [int(x) for x in cnt] == [ref['num_tracks'][v] for v in videos]
    print('%s: %d ids for %d detections in %d videos, margin %.2e, %s' % (c['id'], int(cnt.sum()), int(listed.sum()), len(cnt),
                                                                          ref['margin'], ref['stats']))


# ---------------------------------------------------------------------------------------- 2. more than 256 live tracks
def test_too_many_live_tracks_names_the_video_and_spares_the_others(dev):
    preds, boxes, fmap, name = tr.overflow_set()
    with pytest.raises(ValueError, match=name):
        ev.pose_track(preds, boxes, fmap, device=dev)
    others = {k: v for k, v in fmap.items() if '/over/' not in k}
    ref = tr.pose_track_ref(preds, boxes, others)
    assert ref['margin'] >= tr.MARGIN
    raw, cnt, intact, videos = _raw(dev, preds, boxes, fmap)
    assert intact
    assert [int(x) for x in cnt] == [-1 if v == name else ref['num_tracks'][v] for v in videos] and (cnt < 0).sum() == 1
    rows = np.concatenate([np.asarray(v, np.int64) for v in others.values()])
    assert np.array_equal(raw[rows], ref['tracks'][rows])
    tracks, num = ev.pose_track(preds, boxes, others, device=dev)                     # and without it, through the front door
    assert np.array_equal(tracks, ref['tracks']) and num == ref['num_tracks']


def test_unchecked_tables_never_write_outside_the_outputs(dev):
    """Through the raw entry point, what the Python layer refuses: a frame over the cap, a row outside [0, N), frame
    numbers that do not ascend, a frame segment and a video segment outside their arrays.  Each such video gets -1, the
    video next to it comes out as if alone, the guard zones stay intact."""
    rng = np.random.RandomState(4)
    good = tr.make_video(rng, 3, [1, 2, 3], drop=0, fp_rate=0)
    preds, boxes, fmap = tr.scatter(rng, {'val/good': good, 'val/bad': tr.make_video(rng, 2, [1, 2], drop=0, fp_rate=0)}, 17)
    fmap = {k: fmap[k] for k in sorted(fmap, key=lambda k: '/bad/' in k)}             # the bad video's tables are the last
    N = len(preds)
    ref = tr.pose_track_ref(preds, boxes, {k: v for k, v in fmap.items() if '/good/' in k})
    assert ref['margin'] >= tr.MARGIN
    index, fseg, fnum, vseg, videos = ev._track_tables(fmap, N)
    g, b = videos.index('val/good'), videos.index('val/bad')
    rows_good = np.flatnonzero(ref['tracks'] >= 0)
    fb = int(vseg[b])                                                                 # the first frame of the bad video

    def check(tables):
        raw, cnt, intact, _ = _raw(dev, preds, boxes, None, tables=tables + (videos,))
        assert intact and cnt[b] == -1 and cnt[g] == ref['num_tracks']['val/good']
        assert np.array_equal(raw[rows_good], ref['tracks'][rows_good])

    ix = index.copy()
    ix[fseg[fb]] = N + 7
    check((ix, fseg, fnum, vseg))
    ix[fseg[fb]] = -1
    check((ix, fseg, fnum, vseg))
    fn = fnum.copy()
    fn[fb + 1] = fn[fb]
    check((index, fseg, fn, vseg))
    assert (g, b) == (0, 1)
    fs = fseg.copy()
    fs[-1] = len(index) + 300                                                         # past index, and over the cap
    check((index, fs, fnum, vseg))
    vs = vseg.copy()
    vs[-1] = len(fnum) + 5
    check((index, fseg, fnum, vs))


# ---------------------------------------------------------------------------------------- 3. the front door
def test_accumulator_nms_track_writer(dev, tmp_path):
    """Three small videos through EvalAccumulator.pose_nms -> pose_track -> write_posetrack_results(tracks=...): the files
    carry the restatement's ids for the kept detections."""
    rng = np.random.RandomState(7)
    vids = {'bonn/%06d_bonn' % (i + 1): tr.make_video(rng, n, list(range(1, 7)), fp_rate=0.5) for i, n in enumerate((2, 3, 4))}
    preds, boxes, fmap = tr.scatter(rng, vids, 17)
    N = len(preds)
    boxes[:, 5] = rng.uniform(0.3, 1.0, N)
    dup = fmap[list(fmap)[0]][0]                                                      # a near-duplicate for the NMS to remove
    preds, boxes = np.concatenate([preds, preds[dup:dup + 1]]), np.concatenate([boxes, boxes[dup:dup + 1]])
    preds[N, :, :2] += 0.5
    boxes[N, 5] *= 0.5
    fmap[list(fmap)[0]] = fmap[list(fmap)[0]] + [N]
    acc = ev.EvalAccumulator(N + 1)
    names = [None] * (N + 1)
    for key, rows in fmap.items():
        for r in rows:
            names[r] = key
    scale = np.sqrt(boxes[:, 4])[:, None] / 200.0 * np.ones((1, 2))
    acc.add(preds[:, :, :2], preds[:, :, 2:3], preds[:, :, :2], preds[:, :, 2:3], boxes[:, :2], scale, boxes[:, 5], names)
    nms_kw = dict(in_vis_thre=0.2, oks_thre=0.9)
    boxes2, keep = acc.pose_nms(device=dev, **nms_kw)
    nref = nr.pose_nms_ref(acc.all_preds, acc.all_boxes, acc.filenames_map, **nms_kw)
    assert nref['margin'] >= tr.MARGIN and keep == nref['keep_map']
    kept = sum(len(v) for v in keep.values())
    assert kept <= N and N not in keep[list(fmap)[0]]                                 # the duplicate is gone
    tracks, num = acc.pose_track(keep, device=dev)
    ref = tr.pose_track_ref(acc.all_preds, acc.all_boxes, keep)
    assert ref['margin'] >= tr.MARGIN
    assert np.array_equal(tracks, ref['tracks']) and num == ref['num_tracks'] and len(num) == 3
    assert (tracks < 0).sum() == N + 1 - kept and tracks[N] == -1 and ref['stats']['matched'] > 20   # suppressed: no id
    annot = tmp_path / 'annot'
    annot.mkdir()
    for v in vids:
        (annot / (v.split('/')[1] + '.json')).write_text(json.dumps({'images': [{'file_name': 'images/%s/00000001.jpg' % v, 'nframes': 6}]}))
    written = ev.write_posetrack_results(acc.all_preds, boxes2, keep, str(annot), str(tmp_path / 'res'), tracks=tracks)
    assert sorted(written.values()) == sorted(vids)
    by_key = {tr.default_frame_of(k): rows for k, rows in keep.items()}
    for path, v in written.items():
        for el in json.load(open(path))['annolist']:
            rows = by_key.get((v, el['imgnum'][0]))
            if rows:
                assert [r['track_id'] for r in el['annorect']] == [[int(ref['tracks'][i])] for i in rows]
                assert [r['score'] for r in el['annorect']] == [[float(boxes2[i, 5])] for i in rows]
            else:
                assert el['annorect'][0]['score'] == [0]
