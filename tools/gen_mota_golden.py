"""Writes tests/golden/posetrack_mota.npz: the reference's OWN assignGTmulti (poseval/py/eval_helpers.py:453-668, after
its cleanupData) and MOTAccumulator.update (py-motmetrics/motmetrics/mot.py:90-196) on seeded sequences, driven as
evaluateTracking.computeMetrics drives them (:60-102): one accumulator per (sequence, joint), the frames of a sequence
but its last (`imgidxs[:-1]`; this tool's own loop applies that truncation), one update per frame and joint.  Runs only
where the reference tree is present (oracle.ref_harness); nothing of the reference enters the repository, only the
numbers it computes.

    python tools/gen_mota_golden.py

The reference's tracking half does not run as it stands under a current pandas; ONE function is replaced:
MOTAccumulator.new_event_dataframe (mot.py:198-212) builds its empty event table with `pd.MultiIndex(labels=...)`, an
argument that pandas no longer has.  The stand-in below builds the same empty table with `codes=` and `object` columns
for the two id fields.  Everything else of mot.py -- update, _sanitize_dists, scipy's linear_sum_assignment -- runs
unchanged; it is loaded by path on its own (the package's __init__ imports metrics.py, see below).

The counts.  `mm.metrics.create().compute` is tried first; motmetrics/metrics.py does not import here
(`from collections import Iterable`), which the tool reports, and the five counts are then taken from the event tables
by that file's definitions (:196-218): num_matches / num_switches / num_false_positives / num_misses = the events of
that Type, num_detections = matches + switches, num_objects = the events with an OId (MATCH + SWITCH + MISS); sumD =
events['D'].sum() (evaluateTracking.py:99-102).  The table [4,16] is evaluateTracking.py:158-192 on those counts, by
tests/_mota_ref.finish.

Fixture: 8 seeded sequences, 200 frames (tests/_mota_ref.make_sequences, seed below; coordinates on a 1/8 pixel grid and
scores on a 2^-24 grid: float32-representable), no ignore regions (the reference filters them with shapely, absent
here), stored as the packed arrays of evaluate.pack_posetrack_frames(gt, pr, seq_ids) and the reference's per_seq
[S,15,5] (misses, switches, false positives, detections, objects), sumd_seq [S,15], table [4,16].
The tool refuses to write a fixture when
  * the float64 restatement (tests/_mota_ref.evaluate_mota) differs from the reference in any count of any (sequence,
    joint), or in a sumD by more than 1e-12;
  * a threshold margin min |d - 0.5| / 0.5 or a uniqueness margin (the smallest cost increase when a chosen valid pair
    is forbidden) of any (frame, joint) problem is not above 1e-9;
  * one of the five counts is zero for some joint."""
import copy
import importlib.util
import os
import sys

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(ROOT, 'tests', 'golden', 'posetrack_mota.npz')
SEED = 3
LENGTHS = (40, 30, 25, 35, 20, 28, 12, 10)
GRID = 2.0 ** -3


def new_event_dataframe():
    """The stand-in: the empty event table of mot.py:198-212 for a pandas without `MultiIndex(labels=...)`."""
    idx = pd.MultiIndex(levels=[[], []], codes=[[], []], names=['FrameId', 'Event'])
    cats = pd.Categorical([], categories=['FP', 'MISS', 'SWITCH', 'MATCH'])
    return pd.DataFrame({'Type': pd.Series(cats), 'OId': pd.Series(dtype=object), 'HId': pd.Series(dtype=object),
                         'D': pd.Series(dtype=float)}, index=idx)


def load_reference():
    """-> (eval_helpers, mot module with the stand-in installed, how the counts are taken)."""
    import gen_ap_golden
    from oracle import ref_harness
    eh, _ = gen_ap_golden.load_reference()
    base = os.path.join(ref_harness.REF, 'datasets', 'zoo', 'posetrack', 'posetrack_utils', 'poseval', 'py-motmetrics',
                        'motmetrics')
    spec = importlib.util.spec_from_file_location('_reference_mot', os.path.join(base, 'mot.py'))
    mot = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mot)
    mot.MOTAccumulator.new_event_dataframe = staticmethod(new_event_dataframe)
    how = 'event tables'
    try:                                                          # mm.metrics.create().compute, if it can be had
        saved = {k: sys.modules.get(k) for k in ('motmetrics', 'motmetrics.mot')}
        sys.modules['motmetrics.mot'] = mot
        spec = importlib.util.spec_from_file_location('_reference_metrics', os.path.join(base, 'metrics.py'))
        metrics = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(metrics)
        how = metrics.create()
    except Exception as e:                                        # noqa: BLE001
        print('motmetrics/metrics.py cannot be used (%s: %s): counts from the event tables by its definitions'
              % (type(e).__name__, e))
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return eh, mot, how


def reference_counts(eh, mot, how, gt, pr, seq_ids):
    """-> per_seq [S,15,5] int64, sumd_seq [S,15]: the reference's numbers, sequence by sequence."""
    g, p = copy.deepcopy(gt), copy.deepcopy(pr)
    for frame, sid in zip(g, seq_ids):
        frame['seq_id'], frame['seq_name'] = sid, 'seq%02d' % sid
    for frames in (g, p):                                         # load_data_dir :404-438: ids unique across sequences
        for frame, sid in zip(frames, seq_ids):
            for r in frame['annorect']:
                r['track_id'][0] += sid * eh.MAX_TRACK_ID
    g, p = eh.cleanupData(g, p)
    g, p = eh.removeIgnoredPoints(g, p)
    mot_all = eh.assignGTmulti(g, p, 0.5)[3]
    seq = np.array([f['seq_id'] for f in g])
    uniq = np.unique(seq)
    per_seq, sumd_seq = np.zeros((len(uniq), 15, 5), np.int64), np.zeros((len(uniq), 15))
    for si, sid in enumerate(uniq):
        accs = [mot.MOTAccumulator(auto_id=True) for _ in range(15)]
        for imgidx in np.flatnonzero(seq == sid)[:-1]:
            for j in range(15):
                m = mot_all[imgidx][j]
                accs[j].update(m['trackidxGT'], m['trackidxPr'], m['dist'])
        for j, acc in enumerate(accs):
            ev = acc.events
            if how == 'event tables':
                n = {t: int((ev.Type == t).sum()) for t in ('MATCH', 'SWITCH', 'FP', 'MISS')}
                row = (n['MISS'], n['SWITCH'], n['FP'], n['MATCH'] + n['SWITCH'], int(ev.OId.count()))
            else:
                names = ['num_misses', 'num_switches', 'num_false_positives', 'num_detections', 'num_objects']
                got = how.compute(acc, metrics=names, return_dataframe=False, name='acc')
                row = tuple(int(got[k]) for k in names)
            per_seq[si, j] = row
            s = ev['D'].sum()
            sumd_seq[si, j] = 0.0 if np.isnan(s) else s
    return per_seq, sumd_seq


def main(seed=SEED):
    import _mota_ref as mr
    from fami_pose_amd import evaluate as ev
    eh, mot, how = load_reference()
    rng = np.random.RandomState(seed)
    gt, pr, seq_ids = mr.make_sequences(rng, len(LENGTHS), LENGTHS, grid=GRID)
    per_seq, sumd_seq = reference_counts(eh, mot, how, gt, pr, seq_ids)
    mine = mr.evaluate_mota(gt, pr, seq_ids)
    table = mr.finish(per_seq.sum(0), sumd_seq.sum(0))
    print('seed %d, counts from %s: %d problems, longest chain %d frames, %d dummy frames, margins %.3e (threshold) %.3e '
          '(uniqueness)' % (seed, how if how == 'event tables' else 'metrics.compute', mine['problems'], mine['longest'],
                            mine['dummy_frames'], mine['thr_margin'], mine['uniq_margin']))
    print('totals  ' + '  '.join('%s %s' % (k[4:], per_seq.sum(0)[:, i].tolist()) for i, k in enumerate(mr.COUNTS)))
    print('mota %.3f  motp %.3f  pre %.3f  rec %.3f' % tuple(table[:, 15]))
    assert np.array_equal(mine['per_seq'], per_seq), np.argwhere(mine['per_seq'] != per_seq)
    assert np.abs(mine['sumd_seq'] - sumd_seq).max() <= 1e-12
    assert mine['thr_margin'] > 1e-9 and mine['uniq_margin'] > 1e-9
    assert (per_seq.sum(0) > 0).all(), 'a count is zero for some joint'
    packed = ev.pack_posetrack_frames(gt, pr, seq_ids)
    assert len(packed['verts']) == 0
    out = {k: packed[k] for k in ('pr_has', 'gt_has', 'pr_seg', 'gt_seg', 'frame_index', 'gt_track', 'pr_track',
                                  'frame_seq', 'seq_seg')}
    for k in ('pr_xys', 'gt_xy', 'gt_head'):                     # on the grids every value is an fp32 number: stored as such
        out[k] = packed[k].astype(np.float32)
        assert np.array_equal(out[k].astype(np.float64), packed[k])
    out.update({'per_seq': per_seq.astype(np.int32), 'sumd_seq': sumd_seq, 'table': table})
    np.savez_compressed(OUT, **out)
    print('wrote %s (%d bytes)' % (OUT, os.path.getsize(OUT)))


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else SEED)
