"""PoseTrack MOTA, the parts that need no GPU: the float64 restatement tests/_mota_ref.py against the reference-made
fixture tests/golden/posetrack_mota.npz (tools/gen_mota_golden.py: the reference's own assignGTmulti and
MOTAccumulator.update, with one stand-in for its empty event table), the new keys of evaluate.pack_posetrack_frames and
what it refuses with seq_ids, the layout of `cum`, the refusal of a CPU device, and the margin condition on every input
family of tests/test_posetrack_mota_gpu.py.

Bounds.  The five counts are integers: equal.  mota / motp / pre / rec within 1e-9 on the 0-100 scale (the AP test's
bound): mota, pre and rec are quotients of those integers, motp carries sumD, of which only the order of at most a few
hundred additions of numbers <= 0.5 differs (~ 300 * 2^-53 * 100 ~ 1e-12).
Margin condition: counts are only pinned where no decision is within rounding of turning: for every (frame, joint)
problem of every family, min |d - thresh| / thresh > 1e-9 and the cost of the best assignment that lacks one of the
chosen valid pairs exceeds the optimum by > 1e-9 (head-size units; one subtraction, sqrt, division and a few additions
in fp64 are ~ 1e-15).  No problem is left out."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ap_ref as ar  # noqa: E402
import _mota_cases as mc  # noqa: E402
import _mota_ref as mr  # noqa: E402

import fami_pose_amd as fp  # noqa: E402
from fami_pose_amd import evaluate as ev  # noqa: E402

TOL = 1e-9
MARGIN = 1e-9
J = ar.J


def _close(got, want):
    return np.array_equal(np.isnan(got), np.isnan(want)) and (np.isnan(want).all() or np.nanmax(np.abs(got - want)) <= TOL)


def test_restatement_against_the_reference():
    packed, (per_seq, sumd_seq, table) = mr.load_fixture(mc.GOLD)
    ref = mc.family('fixture')[3]
    assert per_seq.shape == (8, J, 5) and len(packed['frame_index']) >= 180
    assert np.array_equal(ref['per_seq'], per_seq)
    assert (per_seq.sum(0) > 0).all()                              # every count, every joint
    assert np.abs(ref['sumd_seq'] - sumd_seq).max() <= 1e-12
    for r, key in enumerate(('mota', 'motp', 'pre', 'rec')):
        print(key, ' '.join('%.6f' % v for v in ref[key]), '| off by %.3e' % np.nanmax(np.abs(ref[key] - table[r])))
        assert _close(ref[key], table[r]), key
    # the fixture holds float32-representable coordinates and nothing but data
    g = np.load(mc.GOLD)
    assert all(g[k].dtype == np.float32 for k in ('pr_xys', 'gt_xy', 'gt_head'))
    assert all(g[k].dtype.kind in 'fi' for k in g.files)


def test_the_hand_made_cases_count_what_they_say():
    ref = mc.family('cases')[3]
    both = [j for j in range(J) if j not in (mc.MISS_GT, mc.MISS_PR)]
    for s, (name, (_, want)) in enumerate(mc.CASES.items()):
        for j in both:
            assert tuple(ref['per_seq'][s, j]) == want, (name, j)
    # the seeded 5 x 5: the minimum-cost solution has fewer valid pairs than the largest matching, and SEED_5X5 is the
    # first seed for which it has
    found = next(seed for seed in range(64) if np.less(*mc.fewer_pairs_than_matching(*mc.five_by_five(seed))))
    assert found == mc.SEED_5X5 and mc.fewer_pairs_than_matching(*mc.five_by_five(found)) == (4, 5)
    assert tuple(ref['per_seq'][len(mc.CASES), both[0]]) == (1, 0, 1, 4, 5)
    # a joint nobody annotates: only FPs, mota and rec NaN; a joint nobody predicts: only misses, pre NaN, motp 0
    assert ref['num_objects'][mc.MISS_GT] == 0 and ref['num_false_positives'][mc.MISS_GT] > 0
    assert np.isnan(ref['mota'][mc.MISS_GT]) and np.isnan(ref['rec'][mc.MISS_GT]) and ref['pre'][mc.MISS_GT] == 0.0
    assert ref['num_detections'][mc.MISS_PR] == 0 and ref['num_misses'][mc.MISS_PR] == ref['num_objects'][mc.MISS_PR] > 0
    assert np.isnan(ref['pre'][mc.MISS_PR]) and ref['motp'][mc.MISS_PR] == 0.0 and ref['mota'][mc.MISS_PR] == 0.0
    assert np.isclose(ref['mota'][J], np.nanmean(ref['mota'][:J]))


def test_quirks_and_polygons_by_the_restatement():
    ref = mc.family('quirks')[3]
    assert ref['dummy_frames'] == 2
    want = [(1, 0, 1, 1, 2), (1, 0, 1, 1, 2), (0, 0, 0, 0, 0), (0, 0, 0, 0, 0), (0, 0, 0, 1, 1)]
    assert all(tuple(ref['per_seq'][s, j]) == w for s, w in enumerate(want) for j in range(J))
    ref = mc.family('polygons')[3]
    assert ref['dummy_frames'] == 2
    inside = list(range(2, 9))
    assert all(tuple(ref['per_seq'][0, j]) == (2, 0, 2, 4, 6) for j in range(J) if j not in inside)
    assert tuple(ref['per_seq'][0, 2]) == (2, 0, 2, 3, 5)          # joint 2: the lone poses of the frame without a region
    assert all(tuple(ref['per_seq'][0, j]) == (2, 0, 2, 2, 4) for j in inside[1:])


@pytest.mark.parametrize('name', mc.NAMES)
def test_margin_condition(name):
    ref = mc.family(name)[3]
    print('%s: %d problems, longest chain %d, threshold margin %.3e, uniqueness margin %.3e'
          % (name, ref['problems'], ref['longest'], ref['thr_margin'], ref['uniq_margin']))
    assert ref['problems'] > 0 and ref['thr_margin'] > MARGIN and ref['uniq_margin'] > MARGIN
    if name in ('fixture', 'seeded'):                              # every one of the five counts, for every joint
        assert (ref['per_seq'].sum(0) > 0).all()


def test_pack_with_seq_ids():
    gt, pr, seq, ref = mc.family('quirks')
    before = copy.deepcopy((gt, pr))
    plain = ev.pack_posetrack_frames(gt, pr)
    k = ev.pack_posetrack_frames(gt, pr, seq)
    assert (gt, pr) == before
    assert sorted(plain) == sorted(['pr_xys', 'pr_has', 'gt_xy', 'gt_has', 'gt_head', 'pr_seg', 'gt_seg', 'poly_seg',
                                    'vert_seg', 'verts', 'frame_index'])               # the default dict is unchanged
    assert sorted(set(k) - set(plain)) == ['frame_seq', 'gt_track', 'pr_track', 'seq_seg']
    assert all(np.array_equal(plain[n], k[n]) and plain[n].dtype == k[n].dtype for n in plain)
    assert all(k[n].dtype == np.int32 for n in ('gt_track', 'pr_track', 'seq_seg', 'frame_seq'))
    assert list(k['frame_index']) == [0, 1, 2, 3, 4, 5, 6, 9, 11]
    assert list(k['frame_seq']) == [0, 0, 0, 1, 1, 1, 2, 4, 4] and list(k['seq_seg']) == [0, 3, 6, 7, 7, 9]
    # ids renumbered per sequence in order of appearance, annotated and predicted apart; a rect without a point list has none
    assert list(k['gt_track']) == [0, 1, 0, 0] + [0, 0] + [0] + [0, 0]
    assert list(k['pr_track']) == [0, 0, 1] + [0, 1, 0, 2] + [0] + [0, 1]
    assert len(k['gt_track']) == len(k['gt_has']) and len(k['pr_track']) == len(k['pr_has'])
    # the restatement on the unpacked arrays counts what it counts on the lists
    # (a sequence without a kept frame has no frame to be unpacked from)
    k = ev.pack_posetrack_frames(*mc.family('seeded')[:3])
    again = mr.evaluate_mota(*mr.unpack(k))
    assert np.array_equal(again['per_seq'], mc.family('seeded')[3]['per_seq'][np.unique(k['frame_seq'])])
    for name in ('posetrack_mota', 'evaluate_posetrack_mota', 'evaluate_posetrack'):
        assert name in fp.__all__ and getattr(fp, name) is getattr(ev, name)


def test_pack_refusals_with_seq_ids():
    g, p = mc._gt(7, 0.0), mc._pr(1, 2.0)
    one = ([{'annorect': [g]}], [{'annorect': [p]}])
    ev.pack_posetrack_frames(*one, seq_ids=['a'])
    with pytest.raises(ValueError, match='1 frames, 2 seq_ids'):
        ev.pack_posetrack_frames(*one, seq_ids=[0, 0])
    for side, lists in (('annotated', lambda q: ([{'annorect': [q]}], [{'annorect': [p]}])),
                        ('predicted', lambda q: ([{'annorect': [g]}], [{'annorect': [q]}]))):
        q = copy.deepcopy(g if side == 'annotated' else p)
        del q['track_id']
        with pytest.raises(ValueError, match='%s pose of frame 0 has points but no track_id' % side):
            ev.pack_posetrack_frames(*lists(q), seq_ids=[0])
        ev.pack_posetrack_frames(*lists(q))                        # without seq_ids no track_id is read
    with pytest.raises(ValueError, match='track id 7 is listed twice among the annotated poses of frame 0'):
        ev.pack_posetrack_frames([{'annorect': [g, mc._gt(7, 50.0)]}], [{'annorect': [p]}], seq_ids=[0])
    with pytest.raises(ValueError, match='track id 1 is listed twice among the predicted poses of frame 0'):
        ev.pack_posetrack_frames([{'annorect': [g]}], [{'annorect': [p, mc._pr(1, 50.0)]}], seq_ids=[0])
    ev.pack_posetrack_frames([{'annorect': [g]}], [{'annorect': [p, mc._pr(7, 50.0)]}], seq_ids=[0])   # 7 on both sides is fine
    three = ([{'annorect': [g]}] * 3, [{'annorect': [p]}] * 3)
    with pytest.raises(ValueError, match="sequence 'a' are not contiguous \\(frame 2\\)"):
        ev.pack_posetrack_frames(*three, seq_ids=['a', 'b', 'a'])
    # 256 annotated tracks in a sequence are accepted, the 257th is not; another sequence starts from 0 again
    many = [{'annorect': [mc._gt(64 * f + i, 100.0 * i) for i in range(64)]} for f in range(4)]
    preds = [{'annorect': [p]}] * 4
    k = ev.pack_posetrack_frames(many, preds, seq_ids=[0] * 4)
    assert k['gt_track'].max() == 255
    extra = [{'annorect': [mc._gt(999, 0.0)]}]
    with pytest.raises(ValueError, match='sequence 0 has more than 256 ground-truth tracks \\(at frame 4\\)'):
        ev.pack_posetrack_frames(many + extra, preds + [{'annorect': [p]}], seq_ids=[0] * 5)
    k = ev.pack_posetrack_frames(many + extra, preds + [{'annorect': [p]}], seq_ids=[0] * 4 + [1])
    assert k['gt_track'][-1] == 0 and list(k['seq_seg']) == [0, 4, 5]


def test_load_with_seq(tmp_path):
    import json
    gt, pr, seq, _ = mc.family('quirks')
    for d in ('gt', 'pr'):
        (tmp_path / d).mkdir()
    bounds = [0, 3, 6, 7, 9, 12]
    for s in range(5):
        for d, frames in (('gt', gt), ('pr', pr)):
            (tmp_path / d / ('seq%d.json' % s)).write_text(json.dumps({'annolist': frames[bounds[s]:bounds[s + 1]]}))
    two = ev.load_posetrack_dirs(str(tmp_path / 'gt'), str(tmp_path / 'pr'))
    three = ev.load_posetrack_dirs(str(tmp_path / 'gt'), str(tmp_path / 'pr'), with_seq=True)
    assert len(two) == 2 and len(three) == 3 and two[0] == three[0] == gt and two[1] == three[1] == pr
    assert three[2] == seq


def test_cum_layout_and_empty_set():
    table = np.arange(64, dtype=np.float64).reshape(4, 16)
    cum = ev._get_cum_mot(table)
    assert cum == mr.get_cum(table) and len(cum) == 11
    assert cum[:7] == [np.mean([14, 12, 13]), 8.5, 8.5, 8.5, 2.5, 2.5, 2.5] and cum[7:] == [15.0, 31.0, 47.0, 63.0]
    empty = ev.pack_posetrack_frames([{'annorect': []}], [{'annorect': []}], seq_ids=[0])
    res = ev.posetrack_mota(empty, device='cpu')                   # no device work: no device needed
    assert np.isnan(res['mota']).all() and not res['motp'].any() and np.isnan(res['pre']).all() and np.isnan(res['rec']).all()
    assert all(res[k].dtype == np.int64 and res[k].shape == (J,) and not res[k].any() for k in mr.COUNTS)
    assert res['per_seq'].shape == (1, J, 5) and len(res['cum']) == 11 and res['names'] == ar.NAMES + ['total']
    want = mr.evaluate_mota([{'annorect': []}], [{'annorect': []}], [0])
    assert all(_close(res[k], want[k]) for k in ('mota', 'motp', 'pre', 'rec'))


def test_refusals_before_any_device_work():
    gt, pr, seq, _ = mc.family('quirks')
    k = ev.pack_posetrack_frames(gt, pr, seq)
    with pytest.raises(RuntimeError, match='posetrack_mota runs on the HIP path only'):
        ev.posetrack_mota(k, device='cpu')
    with pytest.raises(ValueError, match='pack them with pack_posetrack_frames\\(gt, pr, seq_ids\\)'):
        ev.posetrack_mota(ev.pack_posetrack_frames(gt, pr), device='cpu')
    with pytest.raises(ValueError, match='dist_thresh must be finite'):
        ev.posetrack_mota(k, dist_thresh=float('nan'), device='cpu')
    for key, val, msg in (('gt_track', 256, 'annotated track ids'), ('pr_track', -1, 'predicted track ids'),
                          ('seq_seg', 99, 'seq_seg must ascend')):
        bad = dict(k)
        bad[key] = k[key].copy()
        bad[key][-1] = val
        with pytest.raises(ValueError, match=msg):
            ev.posetrack_mota(bad, device='cpu')
