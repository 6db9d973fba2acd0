"""Track refinement without a GPU: the float64 restatement (tests/_refine_ref.py) held to hand-derived numbers, and the host
half of evaluate.track_refine -- the refusals, the member and fill tables, the keys of the new frames, the pass-through with
every stage off -- which runs before any device work."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _refine_ref as rr  # noqa: E402

import fami_pose_amd as fp  # noqa: E402
from fami_pose_amd import evaluate as ev  # noqa: E402

KEY = '/d/images/val/vid/%08d.jpg'


def tracks_of(people, J=1):
    """people: [[(frame, x, confidence, box score), ...], ...] -> preds [N,J,3], boxes [N,6], fmap, tracks; person p has id p,
    y = 2 x, box columns 0 .. 4 = x + column."""
    preds, boxes, fmap, tracks = [], [], {}, []
    for p, mem in enumerate(people):
        for f, x, c, s in mem:
            fmap.setdefault(KEY % f, []).append(len(preds))
            preds.append([[x, 2 * x, c]] * J)
            boxes.append([x, x + 1, x + 2, x + 3, x + 4, s])
            tracks.append(p)
    return np.asarray(preds, dtype=np.float64), np.asarray(boxes, dtype=np.float64), fmap, np.asarray(tracks)


OFF = dict(max_fill=0, smooth_radius=0, rescore=False, min_len=1)


# ---------------------------------------------------------------------------------------- the restatement, by hand
def test_three_frames_radius_one():
    preds, boxes, fmap, tracks = tracks_of([[(1, 0.0, 1.0, 1.0), (2, 3.0, 1.0, 1.0), (3, 0.0, 1.0, 1.0)]])
    r = rr.track_refine_ref(preds, boxes, fmap, tracks, max_fill=0, smooth_radius=1, smooth_sigma=1.0)
    g1 = np.exp(-0.5)
    assert r['preds2'][1, 0, 0] == np.float32(3.0 / ((g1 + 1.0) + g1))
    assert abs(float(r['preds2'][1, 0, 0]) - 3.0 / (1.0 + 2.0 * g1)) < 3.0 * 2.0 ** -24
    assert r['preds2'][0, 0, 0] == np.float32(g1 * 3.0 / (1.0 + g1)) == r['preds2'][2, 0, 0]    # the ends: a window of two
    assert np.array_equal(r['preds2'][:, 0, 1], 2 * r['preds2'][:, 0, 0])                      # y = 2 x is linear too
    assert np.array_equal(r['preds2'][:, :, 2], preds[:, :, 2]) and r['fmap2'] == fmap         # confidences, lists: as they were


def test_fill_two_rows_at_thirds():
    preds, boxes, fmap, tracks = tracks_of([[(1, 0.0, 0.5, 0.8), (4, 3.0, 0.25, 0.4)]], J=2)
    r = rr.track_refine_ref(preds, boxes, fmap, tracks, max_fill=2, fill_conf=0.5, smooth_radius=0)
    assert r['preds2'].shape == (4, 2, 3) and r['preds2'].dtype == np.float32 and r['boxes2'].shape == (4, 6)
    assert np.array_equal(r['preds2'][2:, :, 0], np.float32([[3.0 * (1.0 / 3.0)] * 2, [3.0 * (2.0 / 3.0)] * 2]))
    assert np.array_equal(r['preds2'][2:, :, 1], np.float32([[6.0 * (1.0 / 3.0)] * 2, [6.0 * (2.0 / 3.0)] * 2]))
    assert (r['preds2'][2:, :, 2] == np.float32(0.25 * 0.5)).all()
    assert np.array_equal(r['boxes2'][2, :5], np.float32(np.arange(5) + 3.0 * (1.0 / 3.0)).astype(np.float64))
    assert (r['boxes2'][2:, 5] == np.float32(np.float64(np.float32(0.4)) * 0.5)).all()
    assert list(r['tracks2']) == [0, 0, 0, 0] and np.array_equal(r['fill'], [[0, 1, 2, 1, 4], [0, 1, 3, 1, 4]])
    assert r['fmap2'] == {KEY % 1: [0], KEY % 4: [1], KEY % 2: [2], KEY % 3: [3]} and list(r['fmap2']) == [KEY % f for f in (1, 4, 2, 3)]
    assert np.array_equal(r['preds2'][:2], preds.astype(np.float32)) and np.array_equal(r['boxes2'][:2], boxes)


def test_a_gap_of_max_fill_plus_one_is_left_alone():
    preds, boxes, fmap, tracks = tracks_of([[(1, 0.0, 1.0, 1.0), (4, 3.0, 1.0, 1.0), (8, 5.0, 1.0, 1.0)]])
    r = rr.track_refine_ref(preds, boxes, fmap, tracks, max_fill=2, smooth_radius=0)
    assert len(r['preds2']) == 5 and [int(x[2]) for x in r['fill']] == [2, 3]                  # 2 missing: filled; 3 missing: not
    r = rr.track_refine_ref(preds, boxes, fmap, tracks, max_fill=1, smooth_radius=0)
    assert len(r['preds2']) == 3 and r['fmap2'] == fmap


def test_an_isolated_member_comes_back_bit_equal():
    preds, boxes, fmap, tracks = tracks_of([[(1, 0.1, 0.3, 1.0)], [(1, 0.7, 0.9, 1.0), (9, 0.2, 0.9, 1.0)]])
    r = rr.track_refine_ref(preds, boxes, fmap, tracks, max_fill=2, smooth_radius=2)
    assert np.array_equal(r['preds2'], preds.astype(np.float32)) and np.array_equal(r['boxes2'], boxes)


def test_a_joint_below_conf_thre_neither_moves_nor_contributes():
    preds, boxes, fmap, tracks = tracks_of([[(1, 0.0, 1.0, 1.0), (2, 3.0, 0.2, 1.0), (3, 7.0, 1.0, 1.0), (4, 0.0, 1.0, 1.0)]])
    r = rr.track_refine_ref(preds, boxes, fmap, tracks, max_fill=0, smooth_radius=1, conf_thre=0.2)   # 0.2 is not > 0.2
    g1 = np.exp(-0.5)
    assert r['preds2'][1, 0, 0] == np.float32(3.0)                                             # does not move
    assert r['preds2'][0, 0, 0] == np.float32(0.0)                                             # its only neighbour does not count
    assert r['preds2'][2, 0, 0] == np.float32((7.0 + g1 * 0.0) / (1.0 + g1))                   # frame 3: itself and frame 4
    r = rr.track_refine_ref(preds, boxes, fmap, tracks, max_fill=0, smooth_radius=1, conf_thre=0.1)
    assert r['preds2'][1, 0, 0] != np.float32(3.0) and r['preds2'][0, 0, 0] != np.float32(0.0)


def test_rescoring_and_pruning_of_two_tracks():
    preds, boxes, fmap, tracks = tracks_of([[(1, 0.0, 1.0, 0.5), (2, 1.0, 1.0, 0.25), (4, 2.0, 1.0, 0.75)], [(2, 9.0, 1.0, 0.125)]])
    r = rr.track_refine_ref(preds, boxes, fmap, tracks, max_fill=1, smooth_radius=0, rescore=True, min_len=2)
    # track 0 after the fill: 0.5, 0.25, min(0.25, 0.75), 0.75 -> mean 0.4375; track 1: one member, pruned (and still rescored)
    assert list(r['boxes2'][:, 5]) == [0.4375, 0.4375, 0.4375, 0.125, 0.4375] and list(r['score']) == [0.4375, 0.125]
    assert list(r['tracks2']) == [0, 0, 0, -1, 0]
    assert r['fmap2'] == {KEY % 1: [0], KEY % 2: [1], KEY % 4: [2], KEY % 3: [4]}               # row 3 left its list, the key stays
    r = rr.track_refine_ref(preds, boxes, fmap, tracks, max_fill=1, smooth_radius=0, min_len=5)
    assert all(v == [] for v in r['fmap2'].values()) and len(r['fmap2']) == 4 and (r['tracks2'] == -1).all()


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_smoothing_brings_constant_velocity_tracks_closer_to_the_path(seed):
    """Equal confidences, symmetric weights: on a straight path the filter is unbiased at members with a full window, so
    it only averages the noise down."""
    rng = np.random.RandomState(seed)
    J, F, R = 5, 40, 2
    preds, boxes, fmap, tracks, clean = [], [], {}, [], []
    for p in range(6):
        c0, vel = rng.uniform(100, 900, (J, 2)), 5.0 * rng.standard_normal(2)
        for f in range(F):
            path = c0 + vel * f
            fmap.setdefault(KEY % f, []).append(len(preds))
            clean.append(path)
            preds.append(np.concatenate([path + 2.0 * rng.standard_normal((J, 2)), np.full((J, 1), 0.75)], axis=1))
            boxes.append(np.ones(6))
            tracks.append(p)
    preds, clean = np.asarray(preds), np.asarray(clean)
    r = rr.track_refine_ref(preds, np.asarray(boxes), fmap, np.asarray(tracks), max_fill=0, smooth_radius=R)
    f_of = np.tile(np.arange(F), 6)
    inner = (f_of >= R) & (f_of < F - R)
    before = ((preds[inner, :, :2] - clean[inner]) ** 2).sum(-1).mean()
    after = ((r['preds2'][inner, :, :2] - clean[inner]) ** 2).sum(-1).mean()
    print('seed %d: mean squared distance to the path %.3f -> %.3f' % (seed, before, after))
    assert after < before


def test_default_key_of():
    assert ev.posetrack_key_of('val/000001_bonn', 9, '/d/images/val/000001_bonn/00000007.jpg') == '/d/images/val/000001_bonn/00000009.jpg'
    assert ev.posetrack_key_of('a/b', 123, 'x/a/b/000001.png') == 'x/a/b/000123.png'
    assert ev.posetrack_key_of('a/b', 1234567, 'x/a/b/01.jpg') == 'x/a/b/1234567.jpg'         # wider than the stem: not cut
    assert ev.posetrack_frame_of(ev.posetrack_key_of('a/b', 12, 'x/a/b/0001.jpg')) == ('a/b', 12)
    assert rr.default_key_of('a/b', 12, 'x/a/b/0001.jpg') == ev.posetrack_key_of('a/b', 12, 'x/a/b/0001.jpg')


# ---------------------------------------------------------------------------------------- evaluate.track_refine on the host
def _good():
    return tracks_of([[(1, 0.0, 1.0, 0.5), (2, 1.0, 1.0, 0.25), (4, 2.0, 1.0, 0.75)], [(2, 9.0, 1.0, 0.125)]], J=2)


def test_refusals():
    preds, boxes, fmap, tracks = _good()

    def refused(match, p=preds, b=boxes, m=fmap, t=tracks, **kw):
        with pytest.raises(ValueError, match=match):
            ev.track_refine(p, b, m, t, device='cpu', **kw)

    refused('expects preds', p=preds[:, :, :2])
    refused('expects preds', b=boxes[:, :5])
    refused('supported 1 .. 32', p=np.zeros((4, 33, 3)))
    refused('tracks must be an integer array of 4 entries', t=tracks[:3])
    refused('tracks must be an integer array', t=tracks.astype(np.float64))
    refused('tracks must be an integer array', t=tracks.reshape(2, 2))
    refused('track ids must fit int32', t=tracks + 2 ** 40)
    refused('row 3 is listed by an image and has track id -1', t=np.array([0, 0, 0, -1]))
    refused('track id 0 occurs twice in frame 2 of video', t=np.array([0, 0, 0, 0]))
    for k in ('max_fill', 'smooth_radius'):
        for v in (-1, 17, 1.0, True):
            refused(k + ' must be an integer in 0 .. 16', **{k: v})
    for v in (0, -3, 2.0):
        refused('min_len must be an integer >= 1', min_len=v)
    for v in (0.0, -1.0):
        refused('smooth_sigma must be > 0', smooth_sigma=v)
    for v in (-0.1, 1.5):
        refused(r'fill_conf must be in \[0, 1\]', fill_conf=v)
    refused('conf_thre must be >= 0', conf_thre=-0.5)
    for k in ('fill_conf', 'smooth_sigma', 'conf_thre'):
        for v in (np.nan, np.inf):
            refused('must be finite', **{k: v})
    for bad in (np.nan, np.inf, 1e39):
        p = preds.copy()
        p[3, 1, 0] = bad                                                                       # (a row of its own track, too)
        refused('preds and boxes must be finite', p=p)
        b = boxes.copy()
        b[0, 2] = bad
        refused('preds and boxes must be finite', b=b)
    # what _track_tables refuses
    refused('lists row 4 outside', m={**fmap, KEY % 4: [4]})
    refused('listed 2 times', m={**fmap, KEY % 4: [2, 2]})
    refused('cannot read a video and a frame number', m={'x.jpg': [0]})
    refused('are both frame 1 of video', m={**fmap, '/e/images/val/vid/01.jpg': []})
    # keys of new frames
    refused('which frame_of places at', key_of=lambda video, f, sib: KEY % (f + 100))
    refused('must return', frame_of=lambda key: 7)
    with pytest.raises(RuntimeError, match='HIP path only'):                                   # everything else was in order
        ev.track_refine(preds, boxes, fmap, tracks, device='cpu')


def test_all_stages_off_gives_the_inputs_back_and_inputs_are_never_modified():
    c = rr.cases()[0]
    keep = [c['preds'].copy(), c['boxes'].copy(), {k: list(v) for k, v in c['fmap'].items()}, c['tracks'].copy()]
    p2, b2, m2, t2 = ev.track_refine(c['preds'], c['boxes'], c['fmap'], c['tracks'], device='cpu', **OFF)   # no device is needed
    assert np.array_equal(p2, c['preds']) and p2.dtype == c['preds'].dtype and p2 is not c['preds']
    assert np.array_equal(b2, c['boxes']) and b2 is not c['boxes']
    assert m2 == c['fmap'] and list(m2) == list(c['fmap']) and m2 is not c['fmap'] and all(m2[k] is not c['fmap'][k] for k in m2)
    assert np.array_equal(t2, c['tracks']) and t2.dtype == np.int32
    r = rr.track_refine_ref(c['preds'], c['boxes'], c['fmap'], c['tracks'], **OFF)
    assert np.array_equal(r['preds2'], c['preds'].astype(np.float32)) and np.array_equal(r['boxes2'], c['boxes']) and r['fmap2'] == c['fmap']
    with pytest.raises(RuntimeError, match='HIP path only'):                                   # the whole host half, then the device
        ev.track_refine(c['preds'], c['boxes'], c['fmap'], c['tracks'], device='cpu', max_fill=16, min_len=3, rescore=True)
    for a, b in zip(keep, [c['preds'], c['boxes'], c['fmap'], c['tracks']]):
        assert (a == b) if isinstance(a, dict) else np.array_equal(a, b)


@pytest.mark.parametrize('n', range(len(rr.CASE_IDS)), ids=rr.CASE_IDS)
def test_host_tables_and_keys_are_the_restatements(n):
    """What is uploaded (the fill table, the sorted members, the track segments) and the lists and keys of the result are
    built without the device: they equal the restatement's."""
    c = rr.cases()[n]
    ref, kw, N = c['ref'], c['kw'], len(c['preds'])
    mrow, mvid, mid, mf, videos, key_at = ev._refine_members(c['fmap'], N, c['tracks'], None)
    fill, g_vid, g_id, srow, sf, mtrk, tseg = ev._refine_tables(mrow, mvid, mid, mf, kw.get('max_fill', 2), N)
    for got, name in ((fill, 'fill'), (srow, 'mrow'), (sf, 'mfr'), (mtrk, 'mtrk'), (tseg, 'tseg')):
        assert np.array_equal(got, ref[name]), name
    fmap2 = {k: list(v) for k, v in c['fmap'].items()}
    ev._refine_keys(fmap2, key_at, videos, g_vid, fill, N, None, None)
    dead = set(np.flatnonzero(ref['tracks2'][:len(ref['tracks2'])] < 0).tolist())
    pruned = {k: [r for r in v if r not in dead] for k, v in fmap2.items()}
    assert pruned == ref['fmap2'] and list(pruned) == list(ref['fmap2'])
    assert ev._track_tables(ref['fmap2'], len(ref['preds2']))                                   # the result is a map pose_track accepts


def test_the_cases_hold_what_the_gpu_test_is_about():
    cs = rr.cases()
    main = cs[0]
    assert {1, 2, 63, 64, 65, 300} <= set(np.diff(cs[2]['ref']['tseg']).tolist())             # members per track (max_fill = 0)
    assert len({rr.default_frame_of(k)[0] for k in main['fmap']}) == 40 and len({rr.default_frame_of(k)[0] for k in cs[6]['fmap']}) == 1
    assert {c['preds'].shape[1] for c in cs} == {1, 17, 32}
    assert {c['kw'].get('smooth_radius', 2) for c in cs} >= {0, 1, 2, 16} and {c['kw'].get('max_fill', 2) for c in cs} >= {0, 1, 2, 16}
    r0 = cs[2]['ref']                                                                          # max_fill = 0: the members as given
    gaps = np.concatenate([np.diff(r0['mfr'][s:e]) - 1 for s, e in zip(r0['tseg'][:-1], r0['tseg'][1:])])
    assert {1, 2, 3, 16, 17} <= set(gaps.tolist())                                             # exactly max_fill and max_fill + 1, for 1, 2 and 16
    new_keys = [k for k in main['ref']['fmap2'] if k not in main['fmap']]
    old_rows = [r for k in main['fmap'] for r in main['ref']['fmap2'][k] if r >= len(main['preds'])]
    assert new_keys and old_rows                                                               # new rows in frames without and with a key
    keys = list(main['fmap'])
    vids = [rr.default_frame_of(k)[0] for k in keys]
    assert any(vids[i] != vids[i + 1] for i in range(len(keys) - 1)) and keys != sorted(keys)  # interleaved, out of order
    listed = {r for v in main['fmap'].values() for r in v}
    assert len(listed) == len(main['preds']) - 3                                               # rows that no image lists
    wide = cs[4]['ref']                                                                        # max_fill = 16: the gap of 16 is filled, of 17 not
    vw = [i for i, k in enumerate(cs[4]['ref']['fmap2']) if '/wide/' in k]
    assert len(vw) == 7 + 16
    assert wide['tracks2'].min() == -1


def test_package_export():
    assert fp.track_refine is ev.track_refine and 'track_refine' in fp.__all__
    assert callable(ev.EvalAccumulator.track_refine)
