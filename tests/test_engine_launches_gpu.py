"""Everything the Engine enqueues in a step, pinned: every library launch with its arguments and buffers, every event
record and every stream wait, in order (tests/_engine_log.py says what a row holds and how pointers, streams and events
are named).  The fixture tests/golden/engine_launches.json was recorded with this module, tests/_engine_log.py and
tests/_ddp_single_rank_engine_launches.py placed into a checkout of the commit it names, RECORD_PARENT set to that
commit's hash; every later tree must reproduce it by equality.  Per case and step() call it keeps the row count, the count
per row name, the row index at which each Engine was created and a sha256 per block of 64 rows; a mismatch writes the
first offending block's rows to tmp_path (the full records of two trees: `python tests/_engine_log.py --dump DIR`).

W48, S = 2, B = 2 at 288 x 160 (heatmap 72 x 40, N = 6 frames).  The weight-resident 16-bit kernels take heatmap widths 64
and 72 only (csrc/conv_t6.hip, t6_plan), and of the even heights up to 128 at those widths 40 is the smallest at which the
host queries answer yes for the 48-channel branch on every path the defaults use: fami_conv_t6_eligible (statistics
epilogues), fami_conv2d_fwd_bnin_ok (BatchNorm apply inside the consumer), fami_conv2d_bwd_pair_ok and _ok_f32 (combined
backward launches) and fami_conv2d_xbn_ok_f32.  At 256 x 192 (heatmap 64 x 48) both combined-launch queries answer no on
every branch.  `_conditions` asserts from the record's own names that each case reached the paths it is there for."""
import json
import os
import subprocess
import sys

import pytest

from _engine_log import BLOCK, CASES, DDP_PLANS, INFERENCE, record_inference, record_trainer, summary

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, 'golden', 'engine_launches.json')
RECORD_PARENT = None        # the hash of the checked-out commit: write the fixture instead of comparing with it


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


def _launches(calls, name):
    return [r for rows, _ in calls for r in rows if r[0] == name]


def _conditions(key, calls, counters):
    """a record that misses the path its case is there for must not pass quietly"""
    names = {r[0] for rows, _ in calls for r in rows}

    def has(*want):
        assert not [n for n in want if n not in names], (key, [n for n in want if n not in names])

    base = key[4:] if key.startswith('ddp-') else key
    if base in ('f32', 'f32-graph'):
        has('fami_conv2d_fwd_xbn_f32', 'fami_conv2d_bwd_pair_f32', 'fami_conv2d_wgrad_defer_xbn_f32')
    if base in ('bf16', 'bf16-graph', 'overlap-bf16', 'eager-hooks-bf16'):
        has('fami_conv2d_fwd_bnin_bf16', 'fami_conv2d_bwd_pair_bf16')
        assert any(r[1][-1] != 'NULL' for r in _launches(calls, 'fami_conv2d_bwd_pair_bf16')), key      # (the last argument: slots)
    if base == 'bf16-fuse-bn':
        has('fami_conv2d_dgrad_bnstats_bf16', 'fami_bn_bwd_apply_slots_bf16')
    if base.endswith('-det'):
        sfx = '_' + base[:3]
        has('fami_bn_train_fwd' + sfx, 'fami_bn_bwd' + sfx, 'fami_dcn_bwd_det_om' + sfx)
        assert not [n for n in names if '_fwd2' in n or '_bwd2' in n], key
    if base == 'f32-frozen-bn':
        has('fami_bn_eval_bwd_f32')
        rows = [r for r in calls[0][0] if r[0].startswith('fami_')]
        assert any(a[0] == 'fami_pool_relu_bwd_f32' and b[0] == 'fami_bn_eval_bwd_f32' for a, b in zip(rows, rows[1:])), key
    if base == 'bf16-two-predictors':
        has('fami_dcn_fwd_bf16')
    if base == 'eager-hooks-bf16':
        assert calls[1][1], key                 # no graph: the second call builds an Engine too
    if base in ('overlap-bf16', 'f32-graph', 'bf16-graph'):
        assert len(calls[0][1]) >= 2 and not calls[1][1], key      # the warm-up runs and the capture, then a replay
    # the counters are those of the Engine created last
    rows, marks = [c for c in calls if c[1]][-1]
    last = [r for r in rows[marks[-1]:] if r[0].startswith('fami_conv2d_')]
    assert counters['xbn'] == sum(r[0].startswith('fami_conv2d_fwd_xbn') for r in last), key
    # (slots is the last argument of the 16-bit combined launch; the f32 one has no statistics epilogue)
    assert counters['bwd'] == sum('dgrad_bnstats' in r[0] or ('bwd_pair_' in r[0] and not r[0].endswith('_f32') and r[1][-1] != 'NULL')
                                  for r in last), key


def _check(key, calls, counters, tmp_path, fixture=FIXTURE, record_parent=None):
    """compare with the entry of `fixture` (or, recording -- this module's RECORD_PARENT or the caller's -- write it)"""
    calls = json.loads(json.dumps(calls))
    assert len(calls) == 2 and calls[0][0], key
    _conditions(key, calls, counters)
    got = summary(calls, counters)
    record_parent = record_parent or RECORD_PARENT
    if record_parent is not None:
        data = _load(fixture) if os.path.isfile(fixture) else {}
        data['recorded_on_commit'] = record_parent
        data.setdefault('cases', {})[key] = got
        with open(fixture, 'w') as f:
            json.dump(data, f, indent=0, sort_keys=True)
            f.write('\n')
        return
    want = _load(fixture)['cases'][key]
    for k, (g, e) in enumerate(zip(got['calls'], want['calls'])):
        for j, (gb, eb) in enumerate(zip(g['blocks'], e['blocks'])):
            if gb != eb:
                path = os.path.join(str(tmp_path), '%s-call%d-block%d.json' % (key, k, j))
                with open(path, 'w') as f:
                    json.dump({'case': key, 'call': k, 'block': j, 'first_row': j * BLOCK, 'sha256': gb, 'fixture_sha256': eb,
                               'rows': calls[k][0][j * BLOCK:(j + 1) * BLOCK]}, f, indent=0)
                raise AssertionError('%s, step() call %d: rows %d.. differ from the recorded ones (this tree\'s rows: %s)'
                                     % (key, k, j * BLOCK, path))
        assert g == e, '%s, step() call %d: %d rows, the fixture has %d' % (key, k, g['rows'], e['rows'])
    assert got == want, key


@pytest.mark.parametrize('key', list(CASES))
def test_step_enqueues_the_recorded_rows(dev, key, monkeypatch, tmp_path):
    for k, v in CASES[key][3].items():
        monkeypatch.setenv(k, v)
    calls, counters = record_trainer(dev, key)
    _check(key, calls, counters, tmp_path)


@pytest.mark.parametrize('key', list(INFERENCE))
def test_inference_enqueues_the_recorded_rows(dev, key, tmp_path):
    calls, counters = record_inference(dev, key)
    packs = [sum(r[0].startswith('fami_pack_conv_weight') for r in rows) for rows, _ in calls]
    assert packs[1] < packs[0], packs        # the second forward meets the cached weight images
    _check(key, calls, counters, tmp_path)


def test_data_parallel_plans_single_rank(dev, tmp_path):
    """The bf16 case on the overlap and the eager-hooks data-parallel plans with ONE rank over RCCL, in a child process
    (tests/_ddp_single_rank_engine_launches.py).  The child writes its records, the comparison is made here."""
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT='29526')
    r = subprocess.run([sys.executable, os.path.join(HERE, '_ddp_single_rank_engine_launches.py'), str(tmp_path)],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'DDP_ENGINE_LAUNCHES_SINGLE_RANK_OK' in r.stdout
    for key in DDP_PLANS:
        with open(os.path.join(str(tmp_path), key + '.json')) as f:
            found = json.load(f)
        _check(key, found['calls'], found['counters'], tmp_path)


def test_fixture_is_the_described_one():
    """every case at the one image size, with counters, and the paths of the default cases on it by count"""
    data = _load()
    assert len(data['recorded_on_commit']) == 40
    cases = data['cases']
    assert sorted(cases) == sorted(list(CASES) + list(INFERENCE) + list(DDP_PLANS))
    for key, c in cases.items():
        assert c['image'] == [288, 160] and len(c['calls']) == 2, key
        for call in c['calls']:
            assert len(call['blocks']) == -(-call['rows'] // BLOCK) and sum(call['names'].values()) == call['rows'], key
    assert cases['f32']['counters']['xbn'] == cases['f32']['calls'][1]['names']['fami_conv2d_fwd_xbn_f32'] > 0
    assert cases['bf16']['counters']['bwd'] > 0 and cases['bf16-fuse-bn']['counters']['bwd'] > cases['bf16']['counters']['bwd']
    assert cases['f32-no-fuse-no-xbn']['counters'] == {'fwd': 0, 'bwd': 0, 'xbn': 0}
