"""The launches of Trainer.step() outside the gradient computation, pinned record by record: which entry points, with
which arguments, on which stream, inside a capture or not (tests/_launch_log.py says what a record holds).  The fixture
tests/golden/trainer_launches.json was recorded with this module and tests/_launch_log.py placed into a checkout of the
commit it names, RECORD_PARENT set to that commit's hash; every later tree must reproduce it by equality.  It pins the end
of a step (gradient pass, clip coefficient, scale update, optimizers, moving average), the accumulating launches, and the
structure of a capture: in graph mode the first call holds the warm-up runs and the captured launches, a later call
nothing or only the launches enqueued behind a replay.

Sizes and helpers are those of tests/test_train_gpu_clip.py: W48, S = 2, 128x96, B = 2, deterministic model."""
import json
import os
import subprocess
import sys

import pytest

from _launch_log import CONFIGS, record_steps
from test_train_gpu_clip import _batch, _trainer

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, 'golden', 'trainer_launches.json')
RECORD_PARENT = None        # the hash of the checked-out commit: write the fixture instead of comparing with it
DDP_PLANS = ('serial', 'overlap', 'eager-hooks')
DDP_CONFIGS = (1, 7, 9)


@pytest.fixture(autouse=True)
def _release_graphs():
    """what tests/conftest.py does behind the other trainer modules: collect this case's Trainer (its hipGraph executables
    own streams) before the next case builds one"""
    yield
    import gc
    import torch
    if torch.cuda.is_available():
        gc.collect()
        torch.cuda.synchronize()
        gc.collect()


def _load(fixture=FIXTURE):
    with open(fixture) as f:
        return json.load(f)


def _check(key, records, fixture=FIXTURE, record_parent=None):
    """compare with the entry of `fixture` (or, recording -- this module's RECORD_PARENT or the caller's -- write it)"""
    records = json.loads(json.dumps(records))
    record_parent = record_parent or RECORD_PARENT
    if record_parent is not None:
        data = _load(fixture) if os.path.isfile(fixture) else {}
        data['recorded_on_commit'] = record_parent
        data.setdefault('cases', {})[key] = records
        with open(fixture, 'w') as f:
            json.dump(data, f, indent=0, sort_keys=True)
            f.write('\n')
        return
    want = _load(fixture)['cases'][key]
    assert len(records) == len(want), key
    for k, (got, exp) in enumerate(zip(records, want)):
        for j, (g, e) in enumerate(zip(got, exp)):
            assert g == e, '%s, step() call %d, launch %d' % (key, k, j)
        assert len(got) == len(exp), '%s, step() call %d: %d launches, the fixture has %d' % (key, k, len(got), len(exp))


@pytest.mark.parametrize('use_graph', [False, True], ids=['eager', 'graph'])
@pytest.mark.parametrize('config', sorted(CONFIGS))
def test_step_launches_equal_the_recorded_ones(dev, config, use_graph):
    mode, kw = CONFIGS[config]
    tr = _trainer(dev, use_graph, deterministic=True, mode=mode, **kw)
    records = record_steps(tr, _batch(dev))
    assert len(records) == tr.accum_steps + 1 and records[0]
    if use_graph:
        # the capture is in the first call; a later call replays (and, accumulating, enqueues behind the replay)
        assert any(r[3] for r in records[0]) and not any(r[3] for call in records[1:] for r in call)
    _check('%d-%s' % (config, 'graph' if use_graph else 'eager'), records)


def test_fixture_rows_derived_from_the_source():
    """rows of the fixture worked out by hand from the code of the commit it was recorded on (eager, outside
    _forward_backward): a fixture that lacks them was not recorded as described"""
    cases = _load()['cases']
    n = cases['4-eager'][0][0][1][1]

    def rows(key, call):
        return [(r[0], r[1]) for r in cases[key][call]]

    one = (1.0).hex()
    got = rows('4-eager', 0)
    assert got[0] == ('fami_unscale_check_f32', ['grad+0', n, (1.0 / 8192).hex(), 'overflow+0'])
    assert [r[0] for r in got] == ['fami_unscale_check_f32', 'fami_adam_prep_checked_f32', 'fami_adam_f32']
    got = rows('5-eager', 0)
    assert got[0] == ('fami_sumsq_f32', ['grad+0', n, '_partials+0'])
    assert [r[0] for r in got] == ['fami_sumsq_f32', 'fami_clip_coef_f32', 'fami_adam_prep_checked_f32', 'fami_adam_scaled_f32']
    assert got[3][1][-1] == 'clip+4'
    assert rows('8-eager', 0) == [('fami_axpby_f32', ['grad+0', 'NULL', 'accum+0', n, one, one]),
                                  ('fami_axpby_f32', ['loss_parts+0', 'NULL', '_window_loss+0', 7, one, one])]
    got = rows('8-eager', 1)
    assert got[0] == ('fami_accum_unscale_check_sumsq_f32', ['grad+0', 'accum+0', n, (0.5).hex(), 'NULL', 'NULL', 'NULL'])
    assert [r[0] for r in got[1:3]] == ['fami_adam_prep_f32', 'fami_adam_f32']
    assert got[3] == ('fami_axpby_f32', ['loss_parts+0', '_window_loss+0', '_window_loss+28', 7, one, one]) and len(got) == 4
    # configuration 1: nothing outside _forward_backward; inside it the scalars first, the arena outside the stem stretch
    # on the side lane, the stretch on the main one
    got = cases['1-eager'][0]
    assert got[0][0] == 'fami_adam_prep_f32' and {r[0] for r in got[1:]} == {'fami_adam_f32'}
    assert [r[2] for r in got[1:]] == ['other'] * (len(got) - 2) + ['current'] and len(got) >= 3


def test_data_parallel_plans_single_rank(dev):
    """Configurations 1, 7 and 9 on the three data-parallel plans (serial, overlap, eager hooks) with ONE rank over RCCL,
    in a child process (tests/_ddp_single_rank_launches.py; tests/test_model_gpu.py::test_ddp_path_single_rank_rccl says
    why a child).  The child prints its records, the comparison is made here."""
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT='29525')
    r = subprocess.run([sys.executable, os.path.join(HERE, '_ddp_single_rank_launches.py')],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'DDP_LAUNCHES_SINGLE_RANK_OK' in r.stdout
    found = {}
    for line in r.stdout.splitlines():
        if line.startswith('LAUNCHES '):
            _, key, records = line.split(' ', 2)
            found[key] = json.loads(records)
    assert sorted(found) == sorted('ddp-%s-%d' % (p, c) for p in DDP_PLANS for c in DDP_CONFIGS)
    for key in sorted(found):
        _check(key, found[key])
