"""Track refinement on the MI355X (csrc/track_refine.hip: fami_track_fill_f32, fami_track_smooth_f32, fami_track_score_f32;
evaluate.track_refine / EvalAccumulator.track_refine) against the float64 restatement tests/_refine_ref.py.

Bounds.  There are none to choose: every output must EQUAL the restatement bit for bit.  Nothing on the device is
transcendental (the Gaussian table is built by the same numpy expression on the host), every fp64 operation is rounded on
its own on both sides, in the same order, and fp64 division is correctly rounded on both.

Shapes (tests/_refine_ref.py builds them, tests/test_track_refine_host.py asserts what they contain): J = 1, 17 and 32;
radius 0, 1, 2 and 16; max_fill 0, 1, 2 and 16; tracks of 1, 2, 63, 64, 65 and 300 members; gaps of exactly max_fill and
max_fill + 1; windows that reach across filled gaps; frames out of order in the map and videos interleaved; rows that no
image lists; V = 1 and V = 40; new rows in frames with and without a key."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _refine_ref as rr  # noqa: E402
import _track_ref as tr  # noqa: E402

from fami_pose_amd import evaluate as ev  # noqa: E402
from fami_pose_amd._lib import lib  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 256
SENT = 0x5a5a5a5a


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype.itemsize == 4 else np.int64)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


class _Raw:
    """The three entry points on tables given as they are (unchecked), every output inside poisoned guard zones."""

    def __init__(self, dev, preds, boxes, ref, tables=None):
        self.dev, self.N, self.J = dev, preds.shape[0], preds.shape[1]
        t = {k: ref[k] for k in ('fill', 'mrow', 'mfr', 'mtrk', 'tseg')}
        t.update(tables or {})
        self.G, self.Mm, self.T = len(ref['fill']), len(ref['mrow']), len(ref['tseg']) - 1
        self.R = self.N + self.G
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)  # noqa: E731
        self.t = {k: up(np.concatenate([np.reshape(v, -1), [0]]), np.int32) for k, v in t.items()}
        # kpts / boxes [R]: the N given rows, then room for the new ones (poisoned until the fill writes them)
        self.kpts = torch.full((GUARD + self.R * self.J * 3 + GUARD,), SENT, dtype=torch.int32, device=dev).view(torch.float32)
        self.boxes = torch.full((GUARD + self.R * 6 + GUARD,), SENT, dtype=torch.int32, device=dev).view(torch.float32)
        self.kpts[GUARD:GUARD + self.N * self.J * 3] = up(preds, np.float32).reshape(-1)
        self.boxes[GUARD:GUARD + self.N * 6] = up(boxes, np.float32).reshape(-1)
        self.out = torch.full((GUARD + self.R * self.J * 3 + GUARD,), SENT, dtype=torch.int32, device=dev).view(torch.float32)
        self.score = torch.full((GUARD + self.T + GUARD,), SENT, dtype=torch.int32, device=dev).view(torch.float32)
        self.flag = torch.zeros(GUARD + 3 + GUARD, dtype=torch.int32, device=dev)
        self.flag[:GUARD] = SENT
        self.flag[GUARD + 3:] = SENT
        self.s = torch.cuda.current_stream(dev).cuda_stream

    def _at(self, t, words=0):
        return t.data_ptr() + 4 * (GUARD + words)

    def fill(self, fill_conf=1.0):
        lib().call('fami_track_fill_f32', self._at(self.kpts), self._at(self.boxes), self.t['fill'].data_ptr(), self.N, self.J,
                   self.G, float(fill_conf), self._at(self.kpts, self.N * self.J * 3), self._at(self.boxes, self.N * 6),
                   self._at(self.flag, 0), self.s)

    def smooth(self, gauss, radius, conf_thre=0.0):
        g = torch.from_numpy(np.ascontiguousarray(gauss, dtype=np.float64)).to(self.dev)
        lib().call('fami_track_smooth_f32', self._at(self.kpts), self.t['mrow'].data_ptr(), self.t['mfr'].data_ptr(),
                   self.t['mtrk'].data_ptr(), self.t['tseg'].data_ptr(), g.data_ptr(), self.R, self.J, self.Mm, self.T, int(radius),
                   float(np.float32(conf_thre)), self._at(self.out), self._at(self.flag, 1), self.s)

    def rescore(self):
        lib().call('fami_track_score_f32', self._at(self.boxes), self.t['mrow'].data_ptr(), self.t['tseg'].data_ptr(), self.R,
                   self.Mm, self.T, self._at(self.score), self._at(self.flag, 2), self.s)

    def read(self):
        """-> (kpts [R,J,3], boxes [R,6], out [R,J,3], score [T] as int32 bit patterns, flag [3], guards intact?)"""
        res, intact = [], True
        for t, n in ((self.kpts, self.R * self.J * 3), (self.boxes, self.R * 6), (self.out, self.R * self.J * 3), (self.score, self.T),
                     (self.flag, 3)):
            a = t.view(torch.int32).cpu().numpy()
            intact = intact and (a[:GUARD] == SENT).all() and (a[GUARD + n:] == SENT).all()
            res.append(a[GUARD:GUARD + n])
        R, J = self.R, self.J
        return res[0].reshape(R, J, 3), res[1].reshape(R, 6), res[2].reshape(R, J, 3), res[3], res[4], intact


# ---------------------------------------------------------------------------------------- 1. against float64
@pytest.mark.parametrize('n', range(len(rr.CASE_IDS)), ids=rr.CASE_IDS)
def test_against_the_restatement(dev, n):
    c = rr.cases()[n]
    ref, kw = c['ref'], c['kw']
    keep = [c['preds'].copy(), c['boxes'].copy(), {k: list(v) for k, v in c['fmap'].items()}, c['tracks'].copy()]
    runs = [ev.track_refine(c['preds'], c['boxes'], c['fmap'], c['tracks'], device=dev, **kw) for _ in range(2)]
    preds2, boxes2, fmap2, tracks2 = runs[0]
    assert _same(preds2, ref['preds2']) and _same(boxes2, ref['boxes2']) and _same(tracks2, ref['tracks2'])
    assert fmap2 == ref['fmap2'] and list(fmap2) == list(ref['fmap2'])
    assert _same(runs[1][0], preds2) and _same(runs[1][1], boxes2) and runs[1][2] == fmap2 and _same(runs[1][3], tracks2)   # two runs
    for a, b in zip(keep, [c['preds'], c['boxes'], c['fmap'], c['tracks']]):                    # the inputs are as they were
        assert (a == b) if isinstance(a, dict) else np.array_equal(a, b)
    N = len(c['preds'])
    index = ev._track_tables(fmap2, len(preds2))[0]                                             # a map the tracker's tables accept ...
    assert np.isfinite(preds2).all() and (tracks2[index] >= 0).all()                            # ... that lists no pruned row
    print('%s: %d rows + %d new, %d tracks, %d new keys, %d rows pruned' % (rr.CASE_IDS[n], N, len(preds2) - N, len(ref['tseg']) - 1,
                                                                           len(fmap2) - len(c['fmap']), int((tracks2[:N][c['tracks'] >= 0] < 0).sum())))


@pytest.mark.parametrize('n', [0, 4, 6, 9], ids=[rr.CASE_IDS[i] for i in (0, 4, 6, 9)])
def test_raw_outputs_stay_inside_their_guards(dev, n):
    """The entry points themselves: each stage's output equals the restatement's, the words around every output are
    unchanged, and `out` is written for member rows only (rows that no image lists keep the poison)."""
    c = rr.cases()[n]
    ref, kw = c['ref'], c['kw']
    N, G = len(c['preds']), len(ref['fill'])
    assert G > 0
    raw = _Raw(dev, c['preds'], c['boxes'], ref)
    raw.fill(kw.get('fill_conf', 1.0))
    raw.smooth(ref['gauss'], kw.get('smooth_radius', 2), kw.get('conf_thre', 0.0))
    raw.rescore()
    kpts, boxes, out, score, flag, intact = raw.read()
    assert intact and not flag.any()
    assert np.array_equal(kpts, _bits(ref['filled'])) and np.array_equal(boxes, _bits(ref['boxes_filled'].astype(np.float32)))
    member = np.zeros(N + G, dtype=bool)
    member[ref['mrow']] = True
    assert (~member).sum() >= (0 if c['fam'] == 'j1' else 2)
    # (a pruned track's rows are still smoothed: pruning is the host's last step and only takes them off the lists)
    assert np.array_equal(out[member], _bits(ref['preds2'])[member]) and (out[~member] == SENT).all()
    assert np.array_equal(score, _bits(ref['score']))


def test_unchecked_tables_raise_the_flag_and_never_write_outside_the_outputs(dev):
    """Through the raw entry points, what the Python layer never builds: an end row, a member row and a track outside their
    arrays, a frame number outside its gap, segments outside the member list.  The launch's flag word is raised, the guard
    zones stay intact, and no thread that saw a bad index wrote anything."""
    c = rr.cases()[6]                                                                           # J = 1, one video, four tracks
    ref = c['ref']
    N, G, Mm, T = len(c['preds']), len(ref['fill']), len(ref['mrow']), len(ref['tseg']) - 1
    R = N + G
    good = _Raw(dev, c['preds'], c['boxes'], ref)
    good.fill()
    good.smooth(ref['gauss'], 2, 0.5)
    good.rescore()
    g_kpts, g_boxes, g_out, g_score, flag, intact = good.read()
    assert intact and not flag.any()

    def run(name, table, stage):
        raw = _Raw(dev, c['preds'], c['boxes'], ref, {name: table})
        if stage != 'fill':
            raw.fill()                                                                          # the later stages read the filled rows
        getattr(raw, stage)(*((ref['gauss'], 2, 0.5) if stage == 'smooth' else ()))
        kpts, boxes, out, score, flag, intact = raw.read()
        assert intact, (name, stage)
        assert list(flag != 0) == [stage == s for s in ('fill', 'smooth', 'rescore')], (name, stage, flag)
        return kpts, boxes, out, score

    for col, bad in ((0, N), (1, -1), (0, R + 5), (2, int(ref['fill'][0, 3])), (2, int(ref['fill'][0, 4]))):
        fill = ref['fill'].copy()
        fill[0, col] = bad                                                                      # the first new row: nothing of it is written
        kpts, boxes, _, _ = run('fill', fill, 'fill')
        assert (kpts[N] == SENT).all() and (boxes[N] == SENT).all()
        assert np.array_equal(kpts[N + 1:], g_kpts[N + 1:]) and np.array_equal(boxes[N + 1:], g_boxes[N + 1:])
    i = int(ref['tseg'][1]) + 3                                                                 # a member in the middle of track 1
    for bad in (R, -2, 2 ** 30):
        mrow = ref['mrow'].copy()
        mrow[i] = bad
        _, _, out, _ = run('mrow', mrow, 'smooth')
        seen = [k for k in range(Mm) if ref['mtrk'][k] == 1 and abs(int(ref['mfr'][k]) - int(ref['mfr'][i])) <= 2]
        rows = ref['mrow'][[k for k in seen if k != i]]
        assert (out[rows] == SENT).all() and (out[ref['mrow'][i]] == SENT).all()                # every window that holds it
        rest = np.setdiff1d(ref['mrow'], ref['mrow'][seen])
        assert np.array_equal(out[rest], g_out[rest])
        _, _, _, score = run('mrow', mrow, 'rescore')
        assert score[1] == SENT and np.array_equal(np.delete(score, 1), np.delete(g_score, 1))
    for bad in (T, -1):
        mtrk = ref['mtrk'].copy()
        mtrk[i] = bad
        _, _, out, _ = run('mtrk', mtrk, 'smooth')
        assert (out[ref['mrow'][i]] == SENT).all()
    for pos, bad in ((T, Mm + 300), (0, -4), (1, Mm + 1)):
        tseg = ref['tseg'].copy()
        tseg[pos] = bad                                                                         # a segment outside the member list
        run('tseg', tseg, 'smooth')
        _, _, _, score = run('tseg', tseg, 'rescore')
        assert (score == SENT).any()
    tseg = ref['tseg'].copy()
    tseg[2] = tseg[1]                                                                           # an empty track: no mean
    _, _, _, score = run('tseg', tseg, 'rescore')
    assert score[1] == SENT


# ---------------------------------------------------------------------------------------- 2. the front door
def test_nms_track_refine_chain(dev, tmp_path):
    """pose_nms -> pose_track -> track_refine -> write_posetrack_results on a seeded set with dropouts: the refined map is
    one the tracker's tables accept, every id occurs at most once per frame, the result equals the restatement on the
    tracker's ids, and the writer takes it."""
    rng = np.random.RandomState(5)
    vids = {'bonn/%06d_bonn' % (i + 1): tr.make_video(rng, n, list(range(1, 13)), drop=0.15, fp_rate=0.5) for i, n in enumerate((2, 3, 5))}
    preds, boxes, fmap = tr.scatter(rng, vids, 17)
    N = len(preds)
    boxes[:, 5] = rng.uniform(0.3, 1.0, N)
    acc = ev.EvalAccumulator(N)
    names = [None] * N
    for key, rows in fmap.items():
        for r in rows:
            names[r] = key
    scale = np.sqrt(boxes[:, 4])[:, None] / 200.0 * np.ones((1, 2))
    acc.add(preds[:, :, :2], preds[:, :, 2:3], preds[:, :, :2], preds[:, :, 2:3], boxes[:, :2], scale, boxes[:, 5], names)
    boxes_n, keep = acc.pose_nms(in_vis_thre=0.2, oks_thre=0.9, device=dev)
    tracks, num = acc.pose_track(keep, device=dev)
    kw = dict(max_fill=2, smooth_radius=2, rescore=True, min_len=3)
    preds2, boxes2, fmap2, tracks2 = acc.track_refine(tracks, keep, boxes=boxes_n, device=dev, **kw)
    ref = rr.track_refine_ref(acc.all_preds, boxes_n, keep, tracks, **kw)
    assert _same(preds2, ref['preds2']) and _same(boxes2, ref['boxes2']) and _same(tracks2, ref['tracks2']) and fmap2 == ref['fmap2']
    assert len(preds2) > N and (tracks2[:N][tracks >= 0] < 0).any()                                 # rows were added, tracks were pruned
    index, fseg, fnum, vseg, videos = ev._track_tables(fmap2, len(preds2))
    assert len(videos) == 3
    for m in range(len(fnum)):
        ids = tracks2[index[fseg[m]:fseg[m + 1]]]
        assert (ids >= 0).all() and len(set(ids.tolist())) == len(ids)
    annot = tmp_path / 'annot'
    annot.mkdir()
    for v in vids:
        (annot / (v.split('/')[1] + '.json')).write_text(json.dumps({'images': [{'file_name': 'images/%s/00000001.jpg' % v, 'nframes': 12}]}))
    written = ev.write_posetrack_results(preds2, boxes2, fmap2, str(annot), str(tmp_path / 'res'), tracks=tracks2)
    assert sorted(written.values()) == sorted(vids)
    by_key = {tr.default_frame_of(k): rows for k, rows in fmap2.items()}
    for path, v in written.items():
        for el in json.load(open(path))['annolist']:
            rows = by_key.get((v, el['imgnum'][0]))
            if rows:
                assert [r['track_id'] for r in el['annorect']] == [[int(tracks2[i])] for i in rows]
