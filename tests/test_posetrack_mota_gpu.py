"""PoseTrack MOTA on the MI355X (csrc/posetrack_mot.hip: fami_posetrack_mot_f64, fami_posetrack_mot_final_f64;
evaluate.posetrack_mota / evaluate_posetrack_mota / evaluate_posetrack) against the float64 restatement
tests/_mota_ref.py and the reference-made fixture tests/golden/posetrack_mota.npz (tests/test_posetrack_mota_host.py says
what that fixture pins and holds the margin condition against every family used here; tests/_mota_cases.py states the
families and what each is for).

Bounds.  The five counts per (sequence, joint) must be EQUAL: the kernel and the restatement evaluate the same fp64
distance expression and solve the same assignment problems, and every family is asserted (on the CPU, before any launch)
to keep every `d <= thresh` decision and every optimum further than 1e-9 from turning, where the arithmetic differs by
~ 1e-15.  sumD per (sequence, joint) within 1e-11 (at most 400 additions with partial sums <= 200, in another order:
400 * 200 * 2^-53 ~ 9e-12).
mota / motp / pre / rec within 1e-9 on the 0-100 scale, NaN positions equal.  Two runs agree bit for bit, and the guard
words behind every output are intact; the fp64 inputs lie between NaNs, the int inputs between 0x5a5a5a5a words.

Shapes: frames of 1 x 1 up to the caps (64 annotated x 256 predicted poses with all 15 joints, 65 / 64 / 63 predictions
around the wave boundary, 256 annotated tracks in one sequence), sequences of 0, 1, 2 and up to 40 frames, more rows than
columns and the reverse, a joint that no annotated and one that no predicted pose has."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ap_ref as ar  # noqa: E402
import _mota_cases as mc  # noqa: E402
import _mota_ref as mr  # noqa: E402

from fami_pose_amd import evaluate as ev  # noqa: E402
from fami_pose_amd._lib import lib  # noqa: E402

pytestmark = pytest.mark.gpu

MARGIN = 1e-9
TOL = 1e-9
GUARD = 256
SENT = 0x5a5a5a5a
J = ar.J


# ---------------------------------------------------------------------------------------- raw launches
def _guarded(dev, words):
    return torch.full((GUARD + words + GUARD,), SENT, dtype=torch.int32, device=dev)


def _unguard(t, words):
    a = t.cpu().numpy()
    return a[GUARD:GUARD + words].copy(), bool((a[:GUARD] == SENT).all() and (a[GUARD + words:] == SENT).all())


def _up_f64(dev, a):
    """-> (tensor kept alive, pointer): the array between two runs of NaN."""
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    t = torch.from_numpy(np.concatenate([np.full(GUARD, np.nan), a, np.full(GUARD, np.nan)])).to(dev)
    return t, t[GUARD:].data_ptr()


def _up_i32(dev, a):
    a = np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
    t = torch.from_numpy(np.concatenate([np.full(GUARD, SENT, np.int32), a, np.full(GUARD, SENT, np.int32)])).to(dev)
    return t, t[GUARD:].data_ptr()


def _raw(dev, k, thresh=0.5):
    """The three entry points on packed arrays: the assign launch for the filtered masks, the MOT launch on them, the
    closing launch -> dict(counts [S,15,5], sumd [S,15], status [S], totals [15,5], sumd_tot [15], table [4,16], intact)."""
    P, G, F, S = len(k['pr_has']), len(k['gt_has']), len(k['pr_seg']) - 1, len(k['seq_seg']) - 1
    s = torch.cuda.current_stream(dev).cuda_stream
    f64 = {n: _up_f64(dev, k[n]) for n in ('pr_xys', 'gt_xy', 'gt_head', 'verts')}
    i32 = {n: _up_i32(dev, k[n]) for n in ('pr_has', 'gt_has', 'pr_seg', 'gt_seg', 'poly_seg', 'vert_seg', 'pr_track',
                                           'gt_track', 'seq_seg')}
    a_sizes = (P, G, P, P, F * J)
    a_out = [_guarded(dev, n) for n in a_sizes]
    lib().call('fami_posetrack_assign_f64', f64['pr_xys'][1], i32['pr_has'][1], f64['gt_xy'][1], i32['gt_has'][1],
               f64['gt_head'][1], i32['pr_seg'][1], i32['gt_seg'][1], i32['poly_seg'][1], i32['vert_seg'][1], f64['verts'][1],
               P, G, F, len(k['vert_seg']) - 1, len(k['verts']), float(thresh), *[t[GUARD:].data_ptr() for t in a_out], s)
    sizes = (S * J * 5, 2 * S * J, S, J * 5, 2 * J, 2 * 4 * (J + 1))       # GUARD words = 1 KiB: the doubles stay aligned
    out = [_guarded(dev, n) for n in sizes]
    ptr = [t[GUARD:].data_ptr() for t in out]
    lib().call('fami_posetrack_mot_f64', f64['pr_xys'][1], a_out[0][GUARD:].data_ptr(), f64['gt_xy'][1],
               a_out[1][GUARD:].data_ptr(), f64['gt_head'][1], i32['pr_seg'][1], i32['gt_seg'][1], i32['poly_seg'][1],
               i32['pr_track'][1], i32['gt_track'][1], i32['seq_seg'][1], P, G, F, S, float(thresh), ptr[0], ptr[1], ptr[2], s)
    lib().call('fami_posetrack_mot_final_f64', ptr[0], ptr[1], ptr[2], S, ptr[3], ptr[4], ptr[5], s)
    res = [_unguard(t, n) for t, n in zip(out + a_out, sizes + a_sizes)]
    return {'counts': res[0][0].reshape(S, J, 5), 'sumd': res[1][0].view(np.float64).reshape(S, J), 'status': res[2][0],
            'totals': res[3][0].reshape(J, 5), 'sumd_tot': res[4][0].view(np.float64), 'pr_has': res[6][0],
            'gt_has': res[7][0], 'table': res[5][0].view(np.float64).reshape(4, J + 1), 'intact': all(r[1] for r in res)}


def _close(got, want):
    return np.array_equal(np.isnan(got), np.isnan(want)) and (np.isnan(want).all() or np.nanmax(np.abs(got - want)) <= TOL)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


_PACKED = {}


def _family(name):
    """-> (restatement, packed); what is asserted of the inputs is asserted here, before any launch."""
    if name not in _PACKED:
        gt, pr, seq, ref = mc.family(name)
        assert ref['thr_margin'] > MARGIN and ref['uniq_margin'] > MARGIN
        packed = ev.pack_posetrack_frames(gt, pr, seq)
        assert len(packed['seq_seg']) - 1 == len(ref['per_seq'])
        if name == 'caps':
            n_g, n_p = np.diff(packed['gt_seg']), np.diff(packed['pr_seg'])
            assert list(n_g) == [64] * 6 and list(n_p) == [256, 65, 64, 63, 128, 3]
            assert packed['gt_track'].max() == 255 and (packed['gt_has'] == 0x7fff).all() and (packed['pr_has'] == 0x7fff).all()
            assert ref['num_switches'].min() > 0 and ref['num_misses'].min() > 0
        if name == 'polygons':
            assert len(packed['verts']) > 0
        _PACKED[name] = (ref, packed)
    return _PACKED[name]


# ---------------------------------------------------------------------------------------- 1. against float64
@pytest.mark.parametrize('name', mc.NAMES)
def test_against_the_restatement(dev, name):
    ref, packed = _family(name)
    got = _raw(dev, packed)
    print('%s: %d sequences, %d problems, longest chain %d frames' % (name, len(ref['per_seq']), ref['problems'], ref['longest']))
    for i, key in enumerate(mr.COUNTS):
        print('%-20s kernel %s | float64 %s' % (key, got['totals'][:, i].tolist(), ref[key].tolist()))
    assert got['intact'] and not got['status'].any()
    assert np.array_equal(got['counts'], ref['per_seq'])
    assert np.array_equal(got['totals'], ref['per_seq'].sum(0))
    assert np.abs(got['sumd'] - ref['sumd_seq']).max() <= 1e-11 and np.abs(got["sumd_tot"] - ref["sum_d"]).max() <= 1e-10
    for r, key in enumerate(('mota', 'motp', 'pre', 'rec')):
        print(key, ' '.join('%.6f' % v for v in got['table'][r]), '| off by %.3e' % np.nanmax(np.abs(got['table'][r] - ref[key])))
        assert _close(got['table'][r], ref[key]), key
    # the front door: the same numbers bit for bit, through one buffer
    res = ev.posetrack_mota(packed, device=dev)
    for r, key in enumerate(('mota', 'motp', 'pre', 'rec')):
        assert res[key].dtype == np.float64 and np.array_equal(_bits(res[key]), _bits(got['table'][r])), key
    for i, key in enumerate(mr.COUNTS):
        assert res[key].dtype == np.int64 and np.array_equal(res[key], ref[key]), key
    assert np.array_equal(res['per_seq'], ref['per_seq']) and np.array_equal(_bits(res['sum_d']), _bits(got['sumd_tot']))
    assert res['names'] == ar.NAMES + ['total'] and len(res['cum']) == 11
    assert np.allclose(res['cum'], ref['cum'], rtol=0, atol=TOL, equal_nan=True)
    if name == 'fixture':                                          # ... and against the reference's own numbers
        per_seq, sumd_seq, table = mr.load_fixture(mc.GOLD)[1]
        assert np.array_equal(res['per_seq'], per_seq) and np.abs(got["sumd"] - sumd_seq).max() <= 1e-11
        assert all(_close(res[key], table[r]) for r, key in enumerate(('mota', 'motp', 'pre', 'rec')))
    if name == 'cases':                                            # ... and what each hand-made case says it counts
        both = [j for j in range(J) if j not in (mc.MISS_GT, mc.MISS_PR)]
        for s, (case, (_, want)) in enumerate(mc.CASES.items()):
            assert all(tuple(got['counts'][s, j]) == want for j in both), case
        assert mc.fewer_pairs_than_matching(*mc.five_by_five(mc.SEED_5X5)) == (4, 5)
        assert all(tuple(got['counts'][len(mc.CASES), j]) == (1, 0, 1, 4, 5) for j in both)
        assert np.isnan(res['mota'][mc.MISS_GT]) and np.isnan(res['pre'][mc.MISS_PR]) and res['motp'][mc.MISS_PR] == 0.0
    if name == 'quirks':
        want = [(1, 0, 1, 1, 2), (1, 0, 1, 1, 2), (0, 0, 0, 0, 0), (0, 0, 0, 0, 0), (0, 0, 0, 1, 1)]
        assert all(tuple(got['counts'][s, j]) == w for s, w in enumerate(want) for j in range(J))
    if name == 'polygons':                                         # the masks the MOT launch read are the filtered ones
        assert (got['pr_has'] != packed['pr_has']).any() and (got['gt_has'] != packed['gt_has']).any()
        assert tuple(got['counts'][0, 0]) == (2, 0, 2, 4, 6) and tuple(got['counts'][0, 5]) == (2, 0, 2, 2, 4)


def test_two_runs_agree_bit_for_bit(dev):
    ref, packed = _family('seeded')
    a, b = _raw(dev, packed), _raw(dev, packed)
    for key in ('counts', 'status', 'totals'):
        assert np.array_equal(a[key], b[key]), key
    for key in ('sumd', 'sumd_tot', 'table'):
        assert np.array_equal(_bits(a[key]), _bits(b[key])), key
    res = ev.posetrack_mota(packed, device=dev)
    assert all(np.array_equal(res['per_seq'][:, :, i].sum(0), res[key]) for i, key in enumerate(mr.COUNTS))
    assert (res['num_objects'] == res['num_detections'] + res['num_misses']).all()


# ---------------------------------------------------------------------------------------- 2. what the Python layer refuses
def test_unchecked_tables_mark_their_sequence_only(dev):
    """Through the raw entry points: a sequence whose frames reach past the kept frames, one with an annotated track id
    of 256 and one with a negative predicted track id get status 1 and counts -1; the others come out as if alone, the
    closing launch leaves the marked one out, and nothing outside the outputs is written."""
    ref, packed = _family('seeded')
    S = len(ref['per_seq'])
    for key, at, val, hit in (('seq_seg', S, len(packed['frame_index']) + 5, S - 1),
                              ('gt_track', 0, 256, 0),
                              ('pr_track', 0, -1, 0)):
        k = {n: v.copy() for n, v in packed.items()}
        k[key][at] = val
        got = _raw(dev, k)
        assert got['intact'] and got['status'][hit] == 1 and (got['counts'][hit] == -1).all() and not got['sumd'][hit].any()
        keep = [s for s in range(S) if s != hit]
        assert not got['status'][keep].any() and np.array_equal(got['counts'][keep], ref['per_seq'][keep])
        assert np.array_equal(got['totals'], ref['per_seq'][keep].sum(0))       # the closing launch leaves the marked one out
        with pytest.raises(ValueError):
            ev.posetrack_mota(k, device=dev)
    k = {n: v.copy() for n, v in packed.items()}
    k['gt_seg'][-1] = len(k['gt_has']) + 7                         # the last frame reaches past the annotated poses:
    with pytest.raises(RuntimeError, match='refused kept frame'):  # the assign launch marks it, the front door reports it
        ev.posetrack_mota(k, device=dev)


# ---------------------------------------------------------------------------------------- 3. the drop-in
def test_evaluate_posetrack_shares_one_assign_launch(dev, tmp_path, monkeypatch):
    gt, pr, seq, ref = mc.family('seeded')
    for d in ('gt', 'pr'):
        (tmp_path / d).mkdir()
    for s in sorted(set(seq)):
        idx = [i for i, q in enumerate(seq) if q == s]
        for d, frames in (('gt', gt), ('pr', pr)):
            (tmp_path / d / ('seq%02d.json' % s)).write_text(json.dumps({'annolist': [frames[i] for i in idx]}))
    gt_dir, pr_dir = str(tmp_path / 'gt'), str(tmp_path / 'pr')
    ap = ev.posetrack_ap(ev.pack_posetrack_frames(gt, pr), device=dev)
    mota = ev.posetrack_mota(_family('seeded')[1], device=dev)
    calls, real = [], lib().call
    monkeypatch.setattr(lib(), 'call', lambda name, *a: (calls.append(name), real(name, *a))[1])
    cum, track_cum = ev.evaluate_posetrack(gt_dir, pr_dir, device=dev)
    assert calls == ['fami_posetrack_assign_f64', 'fami_posetrack_curve_f64', 'fami_posetrack_mot_f64',
                     'fami_posetrack_mot_final_f64']
    assert len(cum) == 8 and len(track_cum) == 11
    assert np.array_equal(_bits(np.array(cum)), _bits(np.array(ap['cum'])))
    assert np.array_equal(_bits(np.array(track_cum)), _bits(np.array(mota['cum'])))
    assert np.allclose(track_cum, ref['cum'], rtol=0, atol=TOL, equal_nan=True) and 0.0 < track_cum[7] < 100.0
    del calls[:]
    assert ev.evaluate_posetrack_mota(gt_dir, pr_dir, device=dev) == track_cum
    assert calls == ['fami_posetrack_assign_f64', 'fami_posetrack_mot_f64', 'fami_posetrack_mot_final_f64']
    del calls[:]
    only_ap = ev.evaluate_posetrack(gt_dir, pr_dir, eval_track=False, device=dev)
    assert only_ap[1] is None and only_ap[0] == cum and calls == ['fami_posetrack_assign_f64', 'fami_posetrack_curve_f64']
    only_mot = ev.evaluate_posetrack(gt_dir, pr_dir, eval_pose=False, device=dev)
    assert np.isnan(only_mot[0]).all() and len(only_mot[0]) == 8 and only_mot[1] == track_cum
