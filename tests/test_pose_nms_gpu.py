"""Pose rescoring and OKS-NMS on the MI355X (csrc/nms.hip: fami_pose_nms_f32; evaluate.pose_nms /
EvalAccumulator.pose_nms) against the float64 restatement tests/_nms_ref.py and against the reference-made fixture
tests/golden/pose_nms.npz (tests/test_pose_nms_host.py says what that fixture pins).

Bounds.  There are none to choose: `rank`, `kept` and `keep_map` must be EQUAL, and `score` must equal bit for bit the
fp64 product box_score * mean(confidences above in_vis_thre) rounded once to fp32 -- the kernel and the restatement sum
the same fp64 values in the same order, and everything downstream orders by that fp32 value.  What can differ is an OKS
(the device's fp64 exp against numpy's, another summation order: ~1e-16 relative; the reference itself rounds its OKS to
fp32: ~1e-7), so equality is only demanded of inputs on which no decision is that close: every family below is seeded,
and the restatement's smallest decision margin on it (|OKS - thr| / thr of every hard comparison, the relative gap
between the best and the next working score at every soft pick) is asserted to be >= 1e-4 before anything is launched.
The seeds were chosen on the CPU so that this holds.

Shapes (the smallest at which the kernel can go wrong): images of 0, 1 and 2 detections; two detections with identical
keypoints and distinct scores; 63 / 64 / 65 detections (the wave boundary) and 256 (the cap); J = 17 and J = 15 with its
own sigmas; an image whose joints all sit below in_vis_thre (score 0) and below vis_thre (OKS 0: nothing suppressed);
equal scores (the tie rule); row lists interleaved over the images and not contiguous; soft mode with max_dets below, at
and above n."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _nms_ref as nr  # noqa: E402

from fami_pose_amd import evaluate as ev  # noqa: E402
from fami_pose_amd._lib import lib  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pose_nms.npz')
MARGIN = 1e-4
GUARD = 256
SENT = 0x5a5a5a5a
SIGMAS15 = np.array([.89, .87, 1.07, 1.07, .87, .89, .62, .72, .79, .79, .72, .62, .79, .26, .5]) / 10.0   # PoseTrack order
SEED_MAIN, SEED_SMALL, SEED_J15 = 28, 2, 2


def _scatter(rng, parts, J, spare=0):
    """parts: [(name, kpts, area, box_score)] -> preds [N,J,3], boxes [N,6] float64, filenames_map.  The detections get
    rows in a random order (plus `spare` rows that no image lists), so every image's list is interleaved with the others'
    and not contiguous; each list keeps the order of its part."""
    N = sum(len(p[1]) for p in parts) + spare
    rows = rng.permutation(N)
    preds, boxes, fmap = np.zeros((N, J, 3)), np.zeros((N, 6)), {}
    boxes[:, :4] = rng.uniform(0, 100, (N, 4))
    preds[:] = rng.uniform(0.3, 1.0, (N, J, 3))                  # the spare rows hold ordinary values too
    boxes[:, 4:] = rng.uniform(0.3, 1.0, (N, 2))
    i = 0
    for name, k, a, b in parts:
        r = rows[i:i + len(k)]
        i += len(k)
        preds[r], boxes[r, 4], boxes[r, 5] = k, a, b
        fmap[name] = [int(x) for x in r]
    return preds, boxes, fmap


def _main_family():
    """J = 17, ten images, 0 ... 256 detections."""
    rng = np.random.RandomState(SEED_MAIN)
    parts = [('/v/images/val/a/%08d.jpg' % (i + 1),) + nr.make_dets(rng, n) for i, n in enumerate((0, 1, 2, 63, 64, 65, 256))]
    k, a, b = nr.make_dets(rng, 1)                               # identical keypoints, distinct scores
    parts.append(('twin', np.concatenate([k, k]), np.concatenate([a, a]), np.array([0.6, 0.8], np.float32)))
    k, a, b = nr.make_dets(rng, 5, per_cluster=5, spread=(2.0,), conf=(0.02, 0.19))   # one tight cluster nobody can see
    parts.append(('unseen', k, a, b))
    k, a, b = nr.make_dets(rng, 9, per_cluster=3)                # equal scores: equal box scores, equal confidences
    k[:, :, 2] = np.float32(0.5)
    parts.append(('ties', k, a, np.full(9, 0.75, np.float32)))
    preds, boxes, fmap = _scatter(rng, parts, 17, spare=3)
    runs = [dict(in_vis_thre=0.2, oks_thre=0.5), dict(in_vis_thre=0.2, oks_thre=0.9, vis_thre=0.2),
            dict(in_vis_thre=0.0, oks_thre=0.7, vis_thre=0.2, soft=True), dict(in_vis_thre=0.2, oks_thre=0.5, soft=True, max_dets=64)]
    return preds, boxes, fmap, None, runs


def _small_family():
    """J = 17, M = 5 images of 12, 0, 7, 12 and 3 detections: soft mode with max_dets below, at and above n."""
    rng = np.random.RandomState(SEED_SMALL)
    parts = [('img%d' % i,) + nr.make_dets(rng, n) for i, n in enumerate((12, 0, 7, 12, 3))]
    preds, boxes, fmap = _scatter(rng, parts, 17)
    runs = [dict(in_vis_thre=0.1, oks_thre=0.5, soft=True, max_dets=md) for md in (1, 5, 12, 30)]
    runs.append(dict(in_vis_thre=0.1, oks_thre=0.5, soft=True, max_dets=7, vis_thre=0.3))
    return preds, boxes, fmap, None, runs


def _j15_family():
    """J = 15 with its own sigmas."""
    rng = np.random.RandomState(SEED_J15)
    parts = [('p%d' % i,) + nr.make_dets(rng, n, J=15) for i, n in enumerate((5, 9, 70))]
    preds, boxes, fmap = _scatter(rng, parts, 15, spare=1)
    runs = [dict(in_vis_thre=0.2, oks_thre=0.6, vis_thre=0.2), dict(in_vis_thre=0.2, oks_thre=0.6, soft=True)]
    return preds, boxes, fmap, SIGMAS15, runs


def _build():
    """Every (family, run) with its float64 reference, and the assertions made on the reference before any launch."""
    cases = []
    for fam, make in (('main', _main_family), ('small', _small_family), ('j15', _j15_family)):
        preds, boxes, fmap, sigmas, runs = make()
        for kw in runs:
            ref = nr.pose_nms_ref(preds, boxes, fmap, sigmas=sigmas, **kw)
            cases.append({'id': '%s-%s' % (fam, '-'.join('%s=%s' % (k[:3], v) for k, v in sorted(kw.items()))), 'fam': fam,
                          'preds': preds, 'boxes': boxes, 'fmap': fmap, 'sigmas': sigmas, 'kw': kw, 'ref': ref})
    assert [c['fam'] for c in cases] == [fam for fam, n in RUNS for _ in range(n)]
    print('smallest decision margin per case: ' + ', '.join('%s %.2e' % (c['id'], c['ref']['margin']) for c in cases))
    assert min(c['ref']['margin'] for c in cases) >= MARGIN
    # every planted case is what it claims
    main = [c for c in cases if c['fam'] == 'main']
    hard, hard_vis, soft_vis, soft64 = main
    fmap, pr = hard['fmap'], hard['preds']
    sizes = [len(v) for v in fmap.values()]
    assert sizes == [0, 1, 2, 63, 64, 65, 256, 2, 5, 9] and len(pr) == sum(sizes) + 3
    for c in main:
        assert [len(v) for v in list(c['ref']['keep_map'].values())[:2]] == [0, 1]
    rows = np.concatenate([np.asarray(v, np.int64) for v in fmap.values()])
    assert (np.diff(rows) != 1).sum() > len(rows) // 2                       # the lists are not contiguous runs
    for c in (hard, hard_vis):
        km, sc = c['ref']['keep_map'], c['ref']['scores']
        t = fmap['twin']
        assert np.array_equal(pr[t[0]], pr[t[1]]) and sc[t[1]] > sc[t[0]] and km['twin'] == [t[1]]   # OKS 1: one survives
        assert any(0 < len(km[k]) < len(fmap[k]) for k in fmap)              # suppression happens
        u = fmap['unseen']
        assert (sc[u] == 0).all()                                            # nothing above in_vis_thre: score 0 ...
        ti = fmap['ties']
        assert len(set(sc[ti])) == 1 and sc[ti[0]] > 0 and km['ties'][0] == ti[0]    # equal scores: the first listed leads
        assert 1 < len(km['ties']) < 9                                       # ... and the tie image has suppressions
        assert 63 > len(km[list(fmap)[3]]) > 1 and 256 > len(km[list(fmap)[6]]) > 64  # the 256 image keeps more than a wave
    assert len(hard['ref']['keep_map']['unseen']) < 5                        # a tight cluster: suppressed with all joints,
    assert hard_vis['ref']['keep_map']['unseen'] == fmap['unseen']           # kept in list order when no joint is visible
    assert soft_vis['ref']['keep_map']['ties'][0] == fmap['ties'][0]
    assert [len(v) for v in soft_vis['ref']['keep_map'].values()] == [min(n, 20) for n in sizes]
    assert [len(v) for v in soft64['ref']['keep_map'].values()] == [min(n, 64) for n in sizes]
    small = [c for c in cases if c['fam'] == 'small']
    for c in small:
        md = c['kw']['max_dets']
        assert [len(v) for v in c['ref']['keep_map'].values()] == [min(n, md) for n in (12, 0, 7, 12, 3)]
    assert small[1]['ref']['keep_map']['img0'] != sorted(small[1]['fmap']['img0'], key=lambda i: -small[1]['ref']['scores'][i])[:5]
    return cases


_CASES = []


def _cases():
    if not _CASES:
        _CASES.extend(_build())
    return _CASES


RUNS = (('main', 4), ('small', 5), ('j15', 2))                   # runs per family, as the makers above list them
IDS = ['%s-%d' % (fam, i) for fam, n in RUNS for i in range(n)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _raw(dev, preds, boxes, lists, sigmas=None, in_vis_thre=0.0, oks_thre=0.5, soft=False, max_dets=20, vis_thre=None):
    """The entry point itself on lists = [[rows], ...] (unchecked), outputs inside poisoned guard zones ->
    (score bits [N], rank [N], kept [M], guards intact?)."""
    N, J = preds.shape[:2]
    M = len(lists)
    seg = np.concatenate([[0], np.cumsum([len(v) for v in lists])]).astype(np.int32)
    index = np.zeros(max(N, int(seg[-1])), np.int32)
    index[:seg[-1]] = np.concatenate([np.asarray(v, np.int32) for v in lists]) if seg[-1] else 0
    sig = ev.COCO_SIGMAS if sigmas is None else sigmas
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)  # noqa: E731
    ins = [up(preds, np.float32), up(boxes[:, 4], np.float32), up(boxes[:, 5], np.float32), up(sig, np.float32),
           up(index, np.int32), up(seg, np.int32)]
    outs = [torch.full((GUARD + n + GUARD,), SENT, dtype=torch.int32, device=dev) for n in (N, N, M)]
    lib().call('fami_pose_nms_f32', *[t.data_ptr() for t in ins], N, J, M, float(in_vis_thre), float(oks_thre),
               1 if soft else 0, int(max_dets), 0.0 if vis_thre is None else float(vis_thre), 0 if vis_thre is None else 1,
               *[t[GUARD:].data_ptr() for t in outs], torch.cuda.current_stream(dev).cuda_stream)
    res = [t.cpu().numpy() for t in outs]
    intact = all((r[:GUARD] == SENT).all() and (r[GUARD + n:] == SENT).all() for r, n in zip(res, (N, N, M)))
    score, rank, kept = (r[GUARD:GUARD + n] for r, n in zip(res, (N, N, M)))
    return score, rank, kept, intact


# ---------------------------------------------------------------------------------------- 1. against float64
@pytest.mark.parametrize('n', range(len(IDS)), ids=IDS)
def test_against_the_restatement(dev, n):
    c = _cases()[n]
    ref, fmap = c['ref'], c['fmap']
    scores, keep_map = ev.pose_nms(c['preds'], c['boxes'], fmap, sigmas=c['sigmas'], device=dev, **c['kw'])
    assert scores.dtype == np.float64 and scores.shape == (len(c['preds']),)
    assert np.array_equal(_bits(scores), _bits(ref['scores']))                # the fp64 product, rounded once
    assert list(keep_map) == list(fmap)                                       # the keys, in the map's order
    assert keep_map == ref['keep_map']
    # the raw outputs, inside guard zones: rank and kept, rows that no image lists untouched, and a second run bit-equal
    listed = np.zeros(len(c['preds']), bool)
    listed[np.concatenate([np.asarray(v, np.int64) for v in fmap.values()])] = True
    runs = [_raw(dev, c['preds'], c['boxes'], list(fmap.values()), c['sigmas'], **c['kw']) for _ in range(2)]
    score, rank, kept, intact = runs[0]
    assert intact
    assert np.array_equal(score[listed], _bits(ref['scores'])[listed]) and (score[~listed] == SENT).all()
    assert np.array_equal(rank[listed], ref['rank'][listed]) and (rank[~listed] == SENT).all()
    assert np.array_equal(kept, ref['kept'])
    assert all(np.array_equal(a, b) for a, b in zip(runs[0][:3], runs[1][:3]))
    print('%s: %d of %d detections kept in %d images, margin %.2e' % (c['id'], int(kept.sum()), int(listed.sum()), len(kept),
                                                                      ref['margin']))


# ---------------------------------------------------------------------------------------- 2. the fixture
def test_reference_fixture(dev):
    g = np.load(GOLD)
    seg, N = g['seg'], len(g['kpts'])
    boxes = np.zeros((N, 6))
    boxes[:, 4], boxes[:, 5] = g['area'], g['box_score']
    fmap = {'im%02d' % m: list(range(int(seg[m]), int(seg[m + 1]))) for m in range(len(seg) - 1)}
    for c, soft, vis, thr, md, keeps in nr.fixture_cases(g):
        scores, keep_map = ev.pose_nms(g['kpts'], boxes, fmap, in_vis_thre=float(g['in_vis_thre']), oks_thre=thr, soft=soft,
                                       max_dets=md, vis_thre=vis, device=dev)
        assert np.array_equal(_bits(scores), _bits(g['score']))
        for m, (key, want) in enumerate(zip(fmap, keeps)):
            assert keep_map[key] == [int(seg[m]) + i for i in want], (c, m)


# ---------------------------------------------------------------------------------------- 3. what the Python layer refuses
def test_unchecked_lists_never_write_outside_the_outputs(dev):
    """Through the raw entry point: a segment over the cap (300 rows) and a segment naming rows outside [0, N) are marked
    kept = -1 with rank -1 on every row of theirs that can be addressed; the over-long one is still rescored; the
    neighbouring images come out as if they were alone; the guard zones stay intact."""
    rng = np.random.RandomState(11)
    parts = [('A',) + nr.make_dets(rng, 5), ('B',) + nr.make_dets(rng, 300), ('C',) + nr.make_dets(rng, 4),
             ('D',) + nr.make_dets(rng, 3)]
    preds, boxes, fmap = _scatter(rng, parts, 17)
    N = len(preds)
    kw = dict(in_vis_thre=0.2, oks_thre=0.5)
    with pytest.raises(ValueError, match='256'):
        ev.pose_nms(preds, boxes, fmap, device=dev, **kw)
    ref = nr.pose_nms_ref(preds, boxes, {k: fmap[k] for k in 'AC'}, **kw)
    assert ref['margin'] >= MARGIN
    every = nr.rescore(preds.astype(np.float32), boxes[:, 5].astype(np.float32), 0.2)
    lists = [fmap['A'], fmap['B'], fmap['C'], [fmap['D'][0], N + 5, -1]]         # N rows in all: index has no more
    score, rank, kept, intact = _raw(dev, preds, boxes, lists, **kw)
    assert intact
    assert list(kept) == [ref['kept'][0], -1, ref['kept'][1], -1]
    for k in 'AC':
        assert np.array_equal(rank[fmap[k]], ref['rank'][fmap[k]])
        assert np.array_equal(score[fmap[k]], _bits(ref['scores'])[fmap[k]])
    assert (rank[fmap['B']] == -1).all() and np.array_equal(score[fmap['B']], _bits(every)[fmap['B']])
    d = fmap['D']
    assert rank[d[0]] == -1 and rank[d[1]] == SENT and rank[d[2]] == SENT and score[d[1]] == SENT   # d[1], d[2]: unlisted
    # a segment table that is no partition of index[0 .. N): marked, nothing else touched
    score, rank, kept, intact = _raw(dev, preds[:12], boxes[:12], [[0, 1, 2], list(range(20))], **kw)
    assert intact and kept[1] == -1 and kept[0] >= 1 and (rank[3:] == SENT).all() and (score[3:] == SENT).all()


# ---------------------------------------------------------------------------------------- 4. the front door
def test_accumulator_feeds_the_writer(dev, tmp_path):
    """Three frames (3, 2 and 1 detections; frame 1 holds a near-duplicate): EvalAccumulator.pose_nms -> the unchanged
    write_posetrack_results.  The files hold only the kept detections, with the rescored scores; the accumulator is
    as it was."""
    rng = np.random.RandomState(5)
    names = ['/d/images/bonn/000001_bonn/0000000%d.jpg' % i for i in (1, 1, 1, 2, 2, 4)]
    k, a, b = nr.make_dets(rng, 6, per_cluster=1)
    k[2, :, :2] = k[0, :, :2] + 0.5                                            # row 2: row 0 again, half a pixel off
    k[2, :, 2] = k[0, :, 2]
    b[:] = [0.9, 0.8, 0.7, 0.6, 0.95, 0.5]
    scale = np.sqrt(a.astype(np.float64))[:, None] / 200.0 * np.ones((1, 2))
    acc = ev.EvalAccumulator(8)
    for lo, hi in ((0, 4), (4, 6)):                                            # two batches
        acc.add(k[lo:hi, :, :2], k[lo:hi, :, 2:3], k[lo:hi, :, :2], k[lo:hi, :, 2:3], rng.uniform(100, 300, (hi - lo, 2)),
                scale[lo:hi], b[lo:hi], names[lo:hi])
    before = (acc.all_preds.copy(), acc.all_boxes.copy(), {kk: list(v) for kk, v in acc.filenames_map.items()}, acc.idx)
    kw = dict(in_vis_thre=0.2, oks_thre=0.9)
    boxes2, fmap2 = acc.pose_nms(device=dev, **kw)
    ref = nr.pose_nms_ref(acc.all_preds[:6], acc.all_boxes[:6], acc.filenames_map, **kw)
    assert ref['margin'] >= MARGIN
    assert boxes2.shape == (6, 6) and np.array_equal(boxes2[:, :5], acc.all_boxes[:6, :5])
    assert np.array_equal(boxes2[:, 5], ref['scores']) and not np.array_equal(boxes2[:, 5], acc.all_boxes[:6, 5])
    assert fmap2 == ref['keep_map'] and list(fmap2) == list(acc.filenames_map)
    assert sorted(fmap2[names[0]]) == [0, 1] and len(fmap2[names[3]]) == 2 and fmap2[names[5]] == [5]   # row 2 is gone
    assert np.array_equal(acc.all_preds, before[0]) and np.array_equal(acc.all_boxes, before[1])
    assert acc.filenames_map == before[2] and acc.idx == before[3]
    annot = tmp_path / 'annot'
    annot.mkdir()
    for nm in ('000001_bonn.json', 'other.json'):
        (annot / nm).write_text(json.dumps({'images': [{'file_name': 'images/bonn/%s/00000001.jpg' % nm[:-5], 'nframes': 4}]}))
    (path,) = ev.write_posetrack_results(acc.all_preds[:6], boxes2, fmap2, str(annot), str(tmp_path / 'res'))
    data = json.load(open(path))['annolist']
    assert [el['imgnum'][0] for el in data] == [1, 2, 3, 4]
    for el, key in zip((data[0], data[1], data[3]), (names[0], names[3], names[5])):
        assert [r['score'] for r in el['annorect']] == [[float(ref['scores'][i])] for i in fmap2[key]]
    assert data[2]['annorect'][0]['score'] == [0]                              # frame 3: the writer's dummy
    (plain,) = ev.write_posetrack_results(acc.all_preds[:6], acc.all_boxes[:6], acc.filenames_map, str(annot), str(tmp_path / 'raw'))
    assert len(json.load(open(plain))['annolist'][0]['annorect']) == 3         # without the step: duplicates, detector scores
