"""OKS pose tracking, the parts that need no device: the float64 restatement tests/_track_ref.py on hand-made cases whose
answer is known without arithmetic, the seeded sets of tests/test_pose_track_gpu.py (their decision margins and what
they exercise), everything `evaluate.pose_track` refuses before it touches a device, its frame tables, and the `tracks=`
argument of `write_posetrack_results`."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _track_ref as tr  # noqa: E402

import fami_pose_amd as fp  # noqa: E402
from fami_pose_amd import evaluate as ev  # noqa: E402

KEY = '/d/images/val/vid/%08d.jpg'
rng0 = np.random.RandomState(0)
SHAPE_A, SHAPE_B = 40.0 * rng0.standard_normal((17, 2)), 40.0 * rng0.standard_normal((17, 2))


def _set(frames):
    """frames: {frame number: [(shape [17,2], centre (x, y), confidence)]} -> preds, boxes, fmap (rows in frame order)."""
    ks, fmap = [], {}
    for f, people in frames.items():
        fmap[KEY % f] = list(range(len(ks), len(ks) + len(people)))
        for shape, c, conf in people:
            k = np.zeros((17, 3))
            k[:, :2], k[:, 2] = shape + np.asarray(c, dtype=np.float64)[None], conf
            ks.append(k)
    preds = np.asarray(ks).reshape(-1, 17, 3)
    boxes = np.zeros((len(preds), 6))
    boxes[:, 4] = 2e4
    return preds, boxes, fmap


def _ids(frames, **kw):
    preds, boxes, fmap = _set(frames)
    ref = tr.pose_track_ref(preds, boxes, fmap, **kw)
    return [[int(ref['tracks'][r]) for r in rows] for rows in fmap.values()], ref


# ---------------------------------------------------------------------------------------- 1. the restatement by hand
def test_two_people_crossing_keep_their_ids():
    """A walks right, B walks left through the same point; they differ in shape, so the ids follow the people although
    the detector lists them in changing order."""
    frames = {}
    for f in range(1, 8):
        a, b = (SHAPE_A, (500 + 6 * (f - 4), 400), 0.9), (SHAPE_B, (500 - 6 * (f - 4), 400), 0.9)
        frames[f] = [a, b] if f % 2 else [b, a]
    ids, ref = _ids(frames)
    assert ids == [[0, 1] if f % 2 else [1, 0] for f in range(1, 8)]
    assert ref['num_tracks'] == {'val/vid': 2} and ref['margin'] > 0.1


def test_gap_shorter_than_max_gap_keeps_the_id_longer_gets_a_new_one():
    """max_gap = 3: seen in frame 1 and again in frame 4 (missing for max_gap - 1 = 2 frames, f - last = 3) keeps the id;
    seen again in frame 5 (missing for max_gap = 3 frames, f - last = 4) is retired and comes back with a new one."""
    p = (SHAPE_A, (300, 300), 0.9)
    ids, ref = _ids({1: [p], 4: [p]}, max_gap=3)
    assert ids == [[0], [0]] and ref['stats']['reid_across_gap'] == 1 and ref['stats']['retired'] == 0
    ids, ref = _ids({1: [p], 5: [p]}, max_gap=3)
    assert ids == [[0], [1]] and ref['stats']['retired'] == 1 and ref['stats']['new_after_retirement'] == 1
    ids, ref = _ids({1: [p], 2: [p], 3: [p]}, max_gap=1)
    assert ids == [[0], [0], [0]]
    ids, ref = _ids({1: [p], 3: [p]}, max_gap=1)                  # max_gap = 1: consecutive frame numbers only
    assert ids == [[0], [1]]


def test_two_detections_contest_one_track():
    """Frame 2 lists two poses near the one track (A, 3 px and 1 px away) and the track B: the first listed takes A
    although the second is closer; the second takes nothing (B is too different) and is new; B keeps its id."""
    a, b = (SHAPE_A, (300, 300), 0.9), (SHAPE_B, (900, 300), 0.9)
    far, near = (SHAPE_A, (303, 300), 0.9), (SHAPE_A, (301, 300), 0.9)
    ids, ref = _ids({1: [a, b], 2: [far, near, b]})
    assert ids == [[0, 1], [0, 2, 1]] and ref['stats']['contested'] == 1
    # ... or its next best: with a second A-shaped track 8 px off, the loser of the contest takes that one
    a2 = (SHAPE_A, (308, 300), 0.9)
    ids, ref = _ids({1: [a, a2], 2: [far, near]}, oks_thre=0.1)
    assert ids == [[0, 1], [0, 1]] and ref['stats']['contested'] == 1
    # equal OKS: the lowest id.  Two identical tracks; the one detection takes id 0
    ids, ref = _ids({1: [a, a], 2: [a]})
    assert ids == [[0, 1], [0]]


def test_empty_mask_matches_nothing():
    seen, unseen = (SHAPE_A, (300, 300), 0.9), (SHAPE_A, (300, 300), 0.1)
    ids, _ = _ids({1: [seen], 2: [unseen], 3: [seen]}, vis_thre=0.2, max_gap=1)
    assert ids == [[0], [1], [1]]                                   # OKS 0 in frame 2: new; frame 3 matches that new track
    ids, _ = _ids({1: [seen], 2: [unseen], 3: [seen]}, max_gap=1)   # without a vis_thre every joint counts
    assert ids == [[0], [0], [0]]


def test_single_frame_video_and_unlisted_rows():
    preds, boxes, fmap = _set({9: [(SHAPE_A, (300, 300), 0.9), (SHAPE_B, (300, 300), 0.9)]})
    preds, boxes = np.concatenate([preds, preds[:1]]), np.concatenate([boxes, boxes[:1]])   # row 2: listed nowhere
    ref = tr.pose_track_ref(preds, boxes, fmap)
    assert list(ref['tracks']) == [0, 1, -1] and ref['num_tracks'] == {'val/vid': 2}


def test_videos_are_independent_and_frames_may_come_in_any_order():
    p, q = (SHAPE_A, (300, 300), 0.9), (SHAPE_B, (600, 300), 0.9)
    preds, boxes, fmap = _set({1: [p], 2: [p, q], 3: [q]})
    keys = list(fmap)
    other = {k.replace('/vid/', '/vid2/'): v for k, v in fmap.items()}
    preds2, boxes2 = np.concatenate([preds, preds]), np.concatenate([boxes, boxes])
    mixed = {}
    for i in (2, 0, 1):                                             # out of order, the two videos interleaved
        mixed[keys[i]] = fmap[keys[i]]
        mixed[keys[i].replace('/vid/', '/vid2/')] = [r + len(preds) for r in other[keys[i].replace('/vid/', '/vid2/')]]
    ref = tr.pose_track_ref(preds2, boxes2, mixed)
    assert list(ref['tracks']) == [0, 0, 1, 1] * 2 and ref['num_tracks'] == {'val/vid': 2, 'val/vid2': 2}


# ---------------------------------------------------------------------------------------- 2. the seeded sets
def test_generated_sets_have_margin_and_exercise_the_rule():
    cases = tr.cases()
    assert [c['fam'] for c in cases] == [fam for fam, _, n in tr.FAMILIES for _ in range(n)] and len(cases) == len(tr.CASE_IDS)
    print('smallest decision margin per case: ' + ', '.join('%s %.2e' % (c['id'], c['ref']['margin']) for c in cases))
    assert min(c['ref']['margin'] for c in cases) >= tr.MARGIN
    for c in cases:
        st = c['ref']['stats']
        assert st['matched'] > 0 and st['retired'] > 0 and st['new_after_retirement'] > 0 and st['max_live'] <= 256, c['id']
    main = [c for c in cases if c['fam'] == 'main']
    for c in main:
        st = c['ref']['stats']
        assert st['contested'] > 0 and st['big_frames'] > 0 and st['max_live'] == 256, c['id']
    assert main[0]['ref']['stats']['reid_across_gap'] > 0                      # max_gap = 3
    assert main[1]['ref']['stats']['reid_across_gap'] == 0                     # max_gap = 1: there is no gap to bridge
    assert main[1]['ref']['stats']['retired'] > main[0]['ref']['stats']['retired']
    assert not np.array_equal(main[0]['ref']['tracks'], main[1]['ref']['tracks'])
    assert not np.array_equal(main[0]['ref']['tracks'], main[2]['ref']['tracks'])
    fmap, ref = main[0]['fmap'], main[0]['ref']
    sizes = {}
    for k, v in fmap.items():
        sizes.setdefault(tr.default_frame_of(k)[0], []).append(len(v))
    assert len(sizes) == 40 == len(ref['num_tracks'])
    assert all(set(sizes['val/n%d' % n]) == {n} for n in (63, 64, 65, 256)) and set(sizes['val/one']) == {1}
    assert sizes['val/single'] == [3] and sizes['val/empty'] == [0] and ref['num_tracks']['val/empty'] == 0
    assert ref['num_tracks']['val/single'] == 3 and ref['num_tracks']['val/one'] == 1
    assert (ref['tracks'] == -1).sum() == 3                                    # the rows no image lists
    keys = list(fmap)
    vids = [tr.default_frame_of(k)[0] for k in keys]
    assert sum(a != b for a, b in zip(vids, vids[1:])) > len(keys) // 2        # videos interleaved in the map
    v0 = [tr.default_frame_of(k)[1] for k in keys if '/v00/' in k]
    assert v0 != sorted(v0) and any(b - a > 1 for a, b in zip(sorted(v0), sorted(v0)[1:]))   # out of order, numbers skip
    assert [c['preds'].shape[1] for c in cases] == [17] * 3 + [15] * 2 + [1] + [32] * 2
    assert len(cases[5]['ref']['num_tracks']) == 1                             # V = 1
    j32 = cases[6]['ref']['stats']
    assert j32['max_live'] > 64 and j32['big_frames'] > 0


def test_overflow_set_is_what_it_claims():
    preds, boxes, fmap, name = tr.overflow_set()
    ref = tr.pose_track_ref(preds, boxes, fmap)
    assert ref['num_tracks'][name] == 300 and max(len(v) for v in fmap.values()) <= 256
    others = tr.pose_track_ref(preds, boxes, {k: v for k, v in fmap.items() if '/over/' not in k})
    assert others['margin'] >= tr.MARGIN and others['stats']['max_live'] < 256


# ---------------------------------------------------------------------------------------- 3. what the host refuses
def _small():
    rng = np.random.RandomState(1)
    return tr.scatter(rng, {'val/a': tr.make_video(rng, 3, [1, 2, 3]), 'val/b': tr.make_video(rng, 2, [4, 5])}, 17, spare=1)


def test_exported():
    assert fp.pose_track is ev.pose_track and 'pose_track' in fp.__all__


@pytest.mark.parametrize('what', ['preds_shape', 'boxes_shape', 'J0', 'J33', 'J15_no_sigmas', 'sigma_nan', 'sigma_zero', 'sigma_len',
                                  'pred_inf', 'area_nan', 'thre_nan', 'vis_inf', 'gap_0', 'gap_float', 'gap_bool', 'key', 'key_number',
                                  'duplicate_frame', 'frame_of_shape', 'frame_of_float', 'cap', 'row_range', 'row_negative',
                                  'row_twice', 'row_float'])
def test_refused_before_any_device_work(what, monkeypatch):
    """Every refusal is a ValueError raised before the library or a device is touched (neither exists for this test)."""
    monkeypatch.setattr(ev, 'lib', None)
    monkeypatch.setattr(ev, 'torch', None)
    preds, boxes, fmap = _small()
    kw = {}
    key0 = list(fmap)[0]
    if what == 'preds_shape':
        preds = preds[:, :, :2]
    elif what == 'boxes_shape':
        boxes = boxes[:-1]
    elif what == 'J0':
        preds = preds[:, :0]
    elif what == 'J33':
        preds, kw = np.ones((len(preds), 33, 3)), {'sigmas': np.ones(33)}
    elif what == 'J15_no_sigmas':
        preds = preds[:, :15]
    elif what in ('sigma_nan', 'sigma_zero'):
        s = tr.COCO_SIGMAS.copy()
        s[3] = np.nan if what == 'sigma_nan' else 0.0
        kw = {'sigmas': s}
    elif what == 'sigma_len':
        kw = {'sigmas': tr.COCO_SIGMAS[:16]}
    elif what == 'pred_inf':
        preds[2, 3, 0] = np.inf
    elif what == 'area_nan':
        boxes[1, 4] = np.nan
    elif what == 'thre_nan':
        kw = {'oks_thre': float('nan')}
    elif what == 'vis_inf':
        kw = {'vis_thre': float('inf')}
    elif what == 'gap_0':
        kw = {'max_gap': 0}
    elif what == 'gap_float':
        kw = {'max_gap': 2.0}
    elif what == 'gap_bool':
        kw = {'max_gap': True}
    elif what == 'key':
        fmap = {'frame7.jpg': fmap.pop(key0), **fmap}
    elif what == 'key_number':
        fmap = {'/d/images/val/a/seven.jpg': fmap.pop(key0), **fmap}
    elif what == 'duplicate_frame':
        video, f = tr.default_frame_of(key0)
        fmap = {**fmap, '/elsewhere/%s/%06d.png' % (video, f): []}
    elif what == 'frame_of_shape':
        kw = {'frame_of': lambda k: 'val/a'}
    elif what == 'frame_of_float':
        kw = {'frame_of': lambda k: ('val/a', 1.5)}
    elif what == 'cap':
        preds, boxes = np.ones((300, 17, 3)), np.ones((300, 6))
        fmap = {key0: list(range(257))}
    elif what == 'row_range':
        fmap[key0] = fmap[key0] + [len(preds)]
    elif what == 'row_negative':
        fmap[key0] = fmap[key0] + [-1]
    elif what == 'row_twice':
        fmap[key0] = fmap[key0] + [fmap[list(fmap)[1]][0]]
    elif what == 'row_float':
        fmap[key0] = [float(r) for r in fmap[key0]]
    with pytest.raises(ValueError, match='pose_track'):
        ev.pose_track(preds, boxes, fmap, **kw)


def test_accumulator_forwards(monkeypatch):
    """EvalAccumulator.pose_track: the accumulated rows only, the given map or its own, the keywords as they are."""
    seen = []
    monkeypatch.setattr(ev, 'pose_track', lambda *a, **kw: seen.append((a, kw)) or 'result')
    acc = ev.EvalAccumulator(5)
    acc.add(np.ones((3, 17, 2)), np.ones((3, 17, 1)), np.ones((3, 17, 2)), np.ones((3, 17, 1)), np.ones((3, 2)), np.ones((3, 2)),
            np.ones(3), [KEY % 1, KEY % 1, KEY % 2])
    assert acc.pose_track(max_gap=2) == 'result' and acc.pose_track({KEY % 1: [1]}, oks_thre=0.5) == 'result'
    (a0, k0), (a1, k1) = seen
    assert a0[0].shape == (3, 17, 3) and a0[1].shape == (3, 6) and a0[2] is acc.filenames_map and k0 == {'max_gap': 2}
    assert a1[2] == {KEY % 1: [1]} and k1 == {'oks_thre': 0.5}


def test_host_device_is_not_a_fallback():
    preds, boxes, fmap = _small()
    with pytest.raises(RuntimeError, match='HIP path only'):
        ev.pose_track(preds, boxes, fmap, device='cpu')


def test_frame_tables():
    """index / fseg / fnum / vseg: rows grouped by frame in list order, frames by video in ascending frame number,
    videos in the order of their first key, whatever the order of the map; an empty list is a frame of its own."""
    fmap = {'/x/v/b/00000007.jpg': [4, 1], '/x/v/a/00000003.jpg': [0], '/x/v/b/00000002.jpg': [5, 2, 3], '/x/v/a/00000001.jpg': [],
            '/x/v/b/00000005.jpg': [6]}
    index, fseg, fnum, vseg, videos = ev._track_tables(fmap, 8)
    assert videos == ['v/b', 'v/a'] and list(vseg) == [0, 3, 5]
    assert list(fnum) == [2, 5, 7, 1, 3] and list(fseg) == [0, 3, 4, 6, 6, 7] and list(index) == [5, 2, 3, 6, 4, 1, 0]
    assert all(a.dtype == np.int32 for a in (index, fseg, fnum, vseg))
    index, fseg, fnum, vseg, videos = ev._track_tables(fmap, 8, frame_of=lambda k: ('all', -int(k[-5])))
    assert videos == ['all'] and list(fnum) == [-7, -5, -3, -2, -1] and list(index) == [4, 1, 6, 0, 5, 2, 3]
    assert ev.posetrack_frame_of('a/b/000012.png') == ('a/b', 12)
    index, fseg, fnum, vseg, videos = ev._track_tables({}, 8)
    assert len(index) == 0 and list(fseg) == [0] and len(fnum) == 0 and list(vseg) == [0] and videos == []


# ---------------------------------------------------------------------------------------- 4. the writer
def _writer_case(tmp_path):
    rng = np.random.RandomState(2)
    names = ['/d/images/bonn/000001_bonn/0000000%d.jpg' % i for i in (1, 1, 2, 2, 2, 4)]
    preds, boxes = rng.uniform(0.1, 1.0, (7, 17, 3)), rng.uniform(0.1, 1.0, (7, 6))
    fmap = {}
    for row, nm in zip((3, 0, 5, 1, 4, 2), names):                                    # row 6 is listed nowhere
        fmap.setdefault(nm, []).append(row)
    annot = tmp_path / 'annot'
    annot.mkdir()
    for nm in ('000001_bonn.json', 'other.json'):
        (annot / nm).write_text(json.dumps({'images': [{'file_name': 'images/bonn/%s/00000001.jpg' % nm[:-5], 'nframes': 4}]}))
    return preds, boxes, fmap, str(annot)


def test_writer_carries_the_track_ids(tmp_path):
    preds, boxes, fmap, annot = _writer_case(tmp_path)
    tracks = np.array([11, 5, 0, 7, 5, 11, -1], dtype=np.int32)                       # row 6: unlisted, may be -1
    (path,) = ev.write_posetrack_results(preds, boxes, fmap, annot, str(tmp_path / 'out'), tracks=tracks)
    data = json.load(open(path))['annolist']
    assert [el['imgnum'][0] for el in data] == [1, 2, 3, 4]
    assert [[r['track_id'] for r in el['annorect']] for el in data] == [[[7], [11]], [[11], [5], [5]], [[0]], [[0]]]
    assert [r['score'] for r in data[1]['annorect']] == [[float(boxes[i, 5])] for i in (5, 1, 4)]
    assert data[2]['annorect'][0]['score'] == [0]                                     # frame 3: the writer's dummy, id 0


def test_writer_without_tracks_is_unchanged(tmp_path):
    """tracks=None and the position-in-frame array write identical files; both carry the reference's placeholder."""
    preds, boxes, fmap, annot = _writer_case(tmp_path)
    (a,) = ev.write_posetrack_results(preds, boxes, fmap, annot, str(tmp_path / 'a'))
    (b,) = ev.write_posetrack_results(preds, boxes, fmap, annot, str(tmp_path / 'b'), tracks=None)
    pos = np.full(7, -1, dtype=np.int64)
    for rows in fmap.values():
        pos[rows] = np.arange(len(rows))
    (c,) = ev.write_posetrack_results(preds, boxes, fmap, annot, str(tmp_path / 'c'), tracks=pos)
    assert open(a, 'rb').read() == open(b, 'rb').read() == open(c, 'rb').read()
    data = json.load(open(a))['annolist']
    assert [[r['track_id'] for r in el['annorect']] for el in data] == [[[0], [1]], [[0], [1], [2]], [[0]], [[0]]]


def test_writer_refuses_bad_tracks(tmp_path):
    preds, boxes, fmap, annot = _writer_case(tmp_path)
    out = tmp_path / 'out'
    for bad in (np.array([0, 1, 2, -1, 4, 5, 6]), np.zeros(6, dtype=np.int32), np.zeros(7), np.zeros((7, 1), dtype=np.int32)):
        with pytest.raises(ValueError, match='track'):
            ev.write_posetrack_results(preds, boxes, fmap, annot, str(out), tracks=bad)
    assert not out.exists()                                                           # refused before anything is written
