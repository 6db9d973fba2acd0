"""The supervision head's launches of Trainer.step() outside the gradient computation, pinned: under gradient accumulation
every scalar term kept beside `loss_parts` (integral L1, structure cosine) adds one window-sum launch per call, behind that of
`loss_parts` and in that order.  Recorder, sizes, helpers and comparison are those of tests/test_train_launches_gpu.py
(tests/_launch_log.py; W48, S = 2, 128x96, B = 2, deterministic model); only the configurations and the fixture differ.
tests/golden/head_trainer_launches.json was recorded like tests/golden/trainer_launches.json: this module,
tests/test_train_launches_gpu.py and tests/_launch_log.py placed into a checkout of the commit it names, RECORD_PARENT set to
that commit's hash; every later tree must reproduce it by equality."""
import os

import pytest

from _launch_log import record_steps
from test_train_gpu_clip import _batch, _trainer
from test_train_launches_gpu import _check, _load, _release_graphs  # noqa: F401  (the autouse fixture)

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'head_trainer_launches.json')
RECORD_PARENT = None        # the hash of the checked-out commit: write the fixture instead of comparing with it

BOTH = dict(accum_steps=2, integral_l1_weight=0.5, structure_cos_weight=0.5)
# name -> (compute mode, Trainer options): the layout of _launch_log.CONFIGS
CONFIGS = {
    'accum-both': (None, dict(BOTH)),
    'accum-both-f16-dynamic': ('f16', dict(loss_scale='dynamic', **BOTH)),
}


@pytest.mark.parametrize('use_graph', [False, True], ids=['eager', 'graph'])
@pytest.mark.parametrize('config', sorted(CONFIGS))
def test_step_launches_equal_the_recorded_ones(dev, config, use_graph):
    mode, kw = CONFIGS[config]
    tr = _trainer(dev, use_graph, deterministic=True, mode=mode, **kw)
    records = record_steps(tr, _batch(dev))
    assert len(records) == tr.accum_steps + 1 and records[0]
    if use_graph:
        # the capture is in the first call; a later call replays and enqueues behind the replay
        assert any(r[3] for r in records[0]) and not any(r[3] for call in records[1:] for r in call)
    for call in records:        # every call ends with the three window sums, uncaptured
        assert [r[0] for r in call[-3:]] == ['fami_axpby_f32'] * 3 and not any(r[3] for r in call[-3:]), config
    _check('%s-%s' % (config, 'graph' if use_graph else 'eager'), records, fixture=FIXTURE, record_parent=RECORD_PARENT)


def test_fixture_rows_derived_from_the_source():
    """rows of the fixture worked out by hand from the code of the commit it was recorded on (_window_call_done): behind the
    accumulating launch of a window's first call, and behind the update of its second, the sums of `loss_parts` (7 values),
    of the integral term and of the structure term, in that order -- the first call into row 0 of each window tensor, the
    closing one from row 0 into row 1; the third call opens the next window like the first"""
    data = _load(FIXTURE)
    assert len(data['recorded_on_commit']) == 40
    cases = data['cases']
    assert sorted(cases) == sorted('%s-%s' % (c, m) for c in CONFIGS for m in ('eager', 'graph'))
    one = (1.0).hex()

    def sums(closing):
        """this call's value (+ row 0 of the window tensor when closing) -> row 1 when closing, row 0 otherwise"""
        return [('fami_axpby_f32', [value + '+0', window + '+0' if closing else 'NULL', '%s+%d' % (window, 4 * n if closing else 0), n, one, one])
                for value, window, n in (('loss_parts', '_window_loss', 7), ('integral_loss', '_window_integral', 1),
                                         ('structure_loss', '_window_structure', 1))]

    for key, calls in cases.items():
        assert len(calls) == 3, key
        tail = [[(r[0], r[1]) for r in call[-3:]] for call in calls]
        assert tail[0] == tail[2] == sums(False) and tail[1] == sums(True), key
        assert all(r[2] == 'current' and not r[3] for call in calls for r in call[-3:]), key
    got = [(r[0], r[1][:3]) for r in cases['accum-both-eager'][0]]
    assert got[0] == ('fami_axpby_f32', ['grad+0', 'NULL', 'accum+0']) and len(got) == 4
