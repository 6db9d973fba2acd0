"""The supervision head's launches inside the gradient computation, pinned: the cases of tests/test_engine_launches_gpu.py
turn no loss option on, these turn each of them on -- OHKM on sub-pixel, joint-weighted targets; the integral L1 term; the
structure term alone; all of them under a dynamic fp16 loss scale; all of them captured and replayed; the integral term with
neither PCK nor MI seeds.  Recorder, sizes, row format and comparison are that module's (tests/_engine_log.py; W48, S = 2,
B = 2 at 288 x 160, targets_from_joints=True); only the case table and the fixture differ.  tests/golden/head_engine_launches.json
was recorded like tests/golden/engine_launches.json: this module, tests/test_engine_launches_gpu.py, tests/_engine_log.py and
tests/_launch_log.py placed into a checkout of the commit it names, RECORD_PARENT set to that commit's hash; every later tree
must reproduce it by equality.  The head's tensors appear by name in the rows (tests/_launch_log.py, _head_named)."""
import os

import pytest

from _engine_log import BLOCK, record_trainer
from test_engine_launches_gpu import _check, _launches, _load, _release_graphs  # noqa: F401  (the autouse fixture)

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'head_engine_launches.json')
RECORD_PARENT = None        # the hash of the checked-out commit: write the fixture instead of comparing with it

JOINT_W = (1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.2, 1.2, 1.5, 1.5, 1.0, 1.0, 1.2, 1.2, 1.5, 1.5)
ALL = dict(ohkm_topk=8, integral_l1_weight=0.5, structure_cos_weight=0.5)
# key -> (compute mode, deterministic, use_graph, environment, Trainer options): the layout of _engine_log.CASES
CASES = {
    'f32-ohkm-ex': (None, False, False, {}, dict(ohkm_topk=8, target_encoding='subpixel', joint_weights=JOINT_W)),
    'bf16-integral': ('bf16', False, False, {}, dict(integral_l1_weight=0.5)),
    'f32-structure': (None, False, False, {}, dict(structure_cos_weight=0.5)),
    'f16-all-dynamic': ('f16', False, False, {}, dict(loss_scale='dynamic', **ALL)),
    'bf16-all-graph': ('bf16', False, True, {}, dict(ALL)),
    'f32-no-pck-no-mi': (None, False, False, {}, dict(pck=False, use_mi=False, integral_l1_weight=0.5)),
}
OHKM = ('fami_ohkm_fwd_f32',)
COORDS = ('fami_softargmax_fwd_f32', 'fami_heatmap_xy_f32')
INTEGRAL = ('fami_integral_l1_fwd_f32', 'fami_integral_l1_bwd_f32')
STRUCTURE = ('fami_structure_cos_fwd_f32', 'fami_structure_cos_bwd_f32', 'fami_softargmax_bwd_f32')
# key -> (the entry points the case is there for, those it must not reach)
PATHS = {
    'f32-ohkm-ex': (OHKM + ('fami_gauss_target_ex_f32',), ('fami_wmse_fwd_f32', 'fami_gauss_target_f32') + COORDS + INTEGRAL + STRUCTURE),
    'bf16-integral': (COORDS + INTEGRAL + ('fami_wmse_fwd_f32', 'fami_gauss_target_f32'), OHKM + STRUCTURE),
    'f32-structure': (COORDS + STRUCTURE + ('fami_wmse_fwd_f32',), OHKM + INTEGRAL),
    'f16-all-dynamic': (OHKM + COORDS + INTEGRAL + STRUCTURE, ('fami_wmse_fwd_f32',)),
    'bf16-all-graph': (OHKM + COORDS + INTEGRAL + STRUCTURE, ('fami_wmse_fwd_f32',)),
    'f32-no-pck-no-mi': (COORDS + INTEGRAL + ('fami_wmse_fwd_f32',), OHKM + STRUCTURE + ('fami_pck_accuracy_f32',)),
}


def _per_engine(rows, marks, name):
    """how many `name` rows each Engine of a step() call enqueued"""
    ends = list(marks[1:]) + [len(rows)]
    return [sum(r[0] == name for r in rows[a:b]) for a, b in zip(marks, ends)]


def _head_conditions(key, calls):
    """a record that misses the path its case is there for must not pass quietly (the Engine-level conditions are checked by
    test_engine_launches_gpu._check)"""
    names = {r[0] for rows, _ in calls for r in rows}
    want, never = PATHS[key]
    assert not [n for n in want if n not in names], (key, [n for n in want if n not in names])
    assert not [n for n in never if n in names], (key, [n for n in never if n in names])
    for rows, marks in calls:
        # one heat-map seed per Engine, and the coordinate terms share one soft-argmax and one set of target positions
        assert _per_engine(rows, marks, 'fami_wmse_bwd_f32') == [1] * len(marks), key
        for n in COORDS:
            assert _per_engine(rows, marks, n) == [int(n in want)] * len(marks), (key, n)
    if CASES[key][2]:
        assert len(calls[0][1]) >= 2 and not calls[1][1] and not calls[1][0], key      # warm-up runs and the capture, then a replay
    else:
        assert len(calls[0][1]) == 1 and len(calls[1][1]) == 1, key
    if key == 'f32-ohkm-ex':
        for r in _launches(calls, 'fami_gauss_target_ex_f32'):
            assert r[1][2] == '_joint_w+0' and r[1][-1] == 1, (key, r)        # joint weights, subpixel
        for r in _launches(calls, 'fami_ohkm_fwd_f32'):
            assert r[1][4] == 'sel_w[2x17]+0' and r[1][8] == 8, (key, r)
        assert all(r[1][2] == 'sel_w[2x17]+0' for r in _launches(calls, 'fami_wmse_bwd_f32')), key      # the seed reads the selection
    # the loss scale of the seeds: the device scalar of a dynamic scale reaches every one of them, a static one none
    gdev = 'scaler_state+0' if CASES[key][4].get('loss_scale') == 'dynamic' else 'NULL'
    for name, at in (('fami_wmse_bwd_f32', -2), ('fami_integral_l1_bwd_f32', -2), ('fami_structure_cos_bwd_f32', -1)):
        assert all(r[1][at] == gdev for r in _launches(calls, name)), (key, name)
    # accumulate: the heat-map seed writes, the coordinate seeds add
    assert all(r[1][-1] == 0 for r in _launches(calls, 'fami_wmse_bwd_f32')), key
    assert all(r[1][-1] == 1 for n in ('fami_integral_l1_bwd_f32', 'fami_softargmax_bwd_f32') for r in _launches(calls, n)), key
    mi = [r for r in _launches(calls, 'fami_axpby_f32') if str(r[1][2]).startswith('loss_parts+') and r[1][2] != 'loss_parts+0']
    assert bool(mi) == CASES[key][4].get('use_mi', True), key


@pytest.mark.parametrize('key', list(CASES))
def test_step_enqueues_the_recorded_rows(dev, key, monkeypatch, tmp_path):
    for k, v in CASES[key][3].items():
        monkeypatch.setenv(k, v)
    calls, counters = record_trainer(dev, key, cases=CASES)
    _head_conditions(key, calls)
    _check(key, calls, counters, tmp_path, fixture=FIXTURE, record_parent=RECORD_PARENT)


def test_fixture_is_the_described_one():
    """every case at the one image size, two step() calls each; the graph case's second call is a replay"""
    data = _load(FIXTURE)
    assert len(data['recorded_on_commit']) == 40
    cases = data['cases']
    assert sorted(cases) == sorted(CASES)
    for key, c in cases.items():
        assert c['image'] == [288, 160] and len(c['calls']) == 2, key
        for call in c['calls']:
            assert len(call['blocks']) == -(-call['rows'] // BLOCK) and sum(call['names'].values()) == call['rows'], key
        want, never = PATHS[key]
        assert all(n in c['calls'][0]['names'] for n in want) and not any(n in c['calls'][0]['names'] for n in never), key
    assert cases['bf16-all-graph']['calls'][1]['rows'] == 0
    one = cases['f16-all-dynamic']['calls'][1]['names']
    assert one['fami_softargmax_fwd_f32'] == one['fami_heatmap_xy_f32'] == one['fami_wmse_bwd_f32'] == 1
