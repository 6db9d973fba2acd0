"""Host side of the batched clip preparation (fami-pose_amd/data.py): half_body_transform against the reference's own
outputs (tests/golden/g15_half_body.npz, tools/gen_half_body_golden.py), draw_augmentation's consumption of the two
random generators against a literal transcription of PoseTrack_Alignment.py:386-412, ClipBatcher's refusals, and the
exported entry points.  No GPU."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

from fami_pose_amd import data as D

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g15_half_body.npz')


def test_half_body_transform_matches_reference_golden():
    g = np.load(GOLDEN)
    assert list(g['names']) == ['upper_wide', 'upper_tall', 'lower', 'lower_fallback', 'upper_too_few', 'none']
    upper = tuple(int(i) for i in g['upper_body_ids'])
    for k, name in enumerate(g['names']):
        joints, vis = g['joints'][k].copy(), g['joints_vis'][k].copy()
        rng = np.random.RandomState(int(g['seed'][k]))
        c, s = D.half_body_transform(joints, vis, 17, upper, float(g['aspect_ratio']), int(g['pixel_std']), rng)
        assert np.array_equal(joints, g['joints'][k]) and np.array_equal(vis, g['joints_vis'][k])
        if g['is_none'][k]:
            assert c is None and s is None, name
        else:
            assert c.dtype == np.float32 and s.dtype == np.float32, name
            assert np.array_equal(c, g['center'][k]) and np.array_equal(s, g['scale'][k]), name
        # exactly one randn() was consumed
        want = np.random.RandomState(int(g['seed'][k]))
        want.randn()
        assert rng.randn() == want.randn()
    # the default generator is numpy.random, as in the reference
    np.random.seed(int(g['seed'][0]))
    c, s = D.half_body_transform(g['joints'][0], g['joints_vis'][0], 17, upper, float(g['aspect_ratio']), int(g['pixel_std']))
    assert np.array_equal(c, g['center'][0]) and np.array_equal(s, g['scale'][0])
    fj, fv = D.fliplr_joints(g['joints'][2], g['joints_vis'][2], int(g['flip_width']), [tuple(p) for p in g['flip_pairs']])
    assert np.array_equal(fj, g['flip_joints']) and np.array_equal(fv, g['flip_vis'])


OPTS = {'num_joints_half_body': 8, 'prob_half_body': 0.3, 'scale_factor': 0.35, 'rot_factor': 45, 'flip': True,
        'num_joints': 17, 'aspect_ratio': 288 / 384}


def _transcription(joints, joints_vis, center, scale, o, np_rng, py_rng, log):
    """PoseTrack_Alignment.py:386-412, statement for statement, on explicit generators; `log` records which draws
    happened.  (None, None) from the half body keeps the box, as draw_augmentation documents."""
    class NP:
        def rand(self):
            log.append('np.rand')
            return np_rng.rand()

        def randn(self):
            log.append('np.randn')
            return np_rng.randn()

    class PY:
        def random(self):
            log.append('py.random')
            return py_rng.random()
    np_random, py_random = NP(), PY()
    r = 0
    if (np.sum(joints_vis[:, 0]) > o['num_joints_half_body'] and np_random.rand() < o['prob_half_body']):
        c_half_body, s_half_body = D.half_body_transform(joints, joints_vis, o['num_joints'], D.UPPER_BODY_IDS,
                                                         o['aspect_ratio'], D.PIXEL_STD, np_random)
        log.append('half_body taken' if c_half_body is not None else 'half_body none')
        if c_half_body is not None:
            center, scale = c_half_body, s_half_body
    scale_factor = o['scale_factor']
    rotation_factor = o['rot_factor']
    if isinstance(scale_factor, list) or isinstance(scale_factor, tuple):
        scale_factor = scale_factor[0]
    scale = scale * np.clip(np_random.randn() * scale_factor + 1, 1 - scale_factor, 1 + scale_factor)
    r = np.clip(np_random.randn() * rotation_factor, -rotation_factor * 2, rotation_factor * 2) \
        if py_random.random() <= 0.6 else 0
    flip = False
    if o['flip'] and py_random.random() <= 0.5:
        flip = True
    return center, scale, r, flip


def _sample(nvis):
    rng = np.random.RandomState(100 + nvis)
    joints = np.zeros((17, 3), np.float32)
    joints[:, 0], joints[:, 1] = rng.uniform(0, 640, 17), rng.uniform(0, 480, 17)
    vis = np.zeros((17, 3), np.float32)
    vis[:nvis, :2] = 1
    return joints, vis, np.array([320.5, 200.25], np.float32), np.array([1.2, 1.6], np.float32)


def _find_seeds(nvis, opts, wanted):
    """first (np seed, py seed) under which the transcription's draw log satisfies `wanted`"""
    joints, vis, center, scale = _sample(nvis)
    for s in range(400):
        log = []
        _transcription(joints, vis, center, scale, opts, np.random.RandomState(s), random.Random(s + 1), log)
        if wanted(log):
            return s, s + 1
    raise AssertionError('no seed found')


SEQ_SKIP = ['np.randn', 'py.random']          # ... then the rotation's randn (or not) and the flip's random (or not)
CASES = {
    # name: (visible joints, options, predicate on the transcription's log)
    'half_body_skipped_few_joints': (8, OPTS, lambda l: 'np.rand' not in l and l.count('py.random') == 2),
    'half_body_drawn_rejected': (12, OPTS, lambda l: l[0] == 'np.rand' and 'half_body taken' not in l),
    'half_body_drawn_taken': (12, OPTS, lambda l: l[:3] == ['np.rand', 'np.randn', 'half_body taken']),
    'rotation_skipped': (12, OPTS, lambda l: l[-3:] == ['np.randn', 'py.random', 'py.random']),
    'rotation_drawn': (12, OPTS, lambda l: l[-4:] == ['np.randn', 'py.random', 'np.randn', 'py.random']),
    'flip_disabled': (12, dict(OPTS, flip=False), lambda l: l.count('py.random') == 1),
    'scale_factor_list': (12, dict(OPTS, scale_factor=[0.25, 0.4]), lambda l: True),
}


def _run_case(name):
    nvis, opts, wanted = CASES[name]
    s_np, s_py = _find_seeds(nvis, opts, wanted)
    joints, vis, center, scale = _sample(nvis)
    keep = [a.copy() for a in (joints, vis, center, scale)]
    np_rng, py_rng = np.random.RandomState(s_np), random.Random(s_py)
    got = D.draw_augmentation(joints, vis, center, scale, opts, np_rng, py_rng)
    np_ref, py_ref, log = np.random.RandomState(s_np), random.Random(s_py), []
    want = _transcription(keep[0].copy(), keep[1].copy(), keep[2].copy(), keep[3].copy(), opts, np_ref, py_ref, log)
    assert wanted(log)
    unmodified = all(np.array_equal(a, b) for a, b in zip((joints, vis, center, scale), keep))
    return got, want, (np_rng, py_rng), (np_ref, py_ref), unmodified


@pytest.mark.parametrize('name', list(CASES))
def test_draw_augmentation_leaves_both_generators_where_the_reference_order_does(name):
    _, _, (np_rng, py_rng), (np_ref, py_ref), _ = _run_case(name)
    assert np_rng.rand() == np_ref.rand() and np_rng.randn() == np_ref.randn()
    assert py_rng.random() == py_ref.random()


@pytest.mark.parametrize('name', list(CASES))
def test_draw_augmentation_values(name):
    (center, scale, rot, flip), (c0, s0, r0, f0), _, _, unmodified = _run_case(name)
    assert unmodified
    assert np.array_equal(center, c0) and np.array_equal(scale, s0) and scale.dtype == np.asarray(s0).dtype
    assert rot == r0 and flip is f0
    if name == 'rotation_skipped':
        assert rot == 0
    if name == 'rotation_drawn':
        assert rot != 0 and abs(rot) <= 90
    if name == 'flip_disabled':
        assert flip is False
    if name == 'half_body_drawn_taken':
        assert not np.array_equal(center, _sample(12)[2])
    if name in ('half_body_skipped_few_joints', 'half_body_drawn_rejected'):
        assert np.array_equal(center, _sample(CASES[name][0])[2])


def test_draw_augmentation_reads_the_cfg_and_keeps_the_box_on_none():
    import fami_pose_amd as fp
    cfg = fp.default_cfg()
    joints, vis, center, scale = _sample(12)
    a = D.draw_augmentation(joints, vis, center, scale, cfg, np.random.RandomState(3), random.Random(4))
    b = D.draw_augmentation(joints, vis, center, scale, OPTS, np.random.RandomState(3), random.Random(4))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # (None, None): only reachable with a threshold below the reference's 8 -- one visible joint, half body forced
    joints, vis, center, scale = _sample(1)
    o = dict(OPTS, num_joints_half_body=0, prob_half_body=1.0)
    np_rng = np.random.RandomState(5)
    c, s, _, _ = D.draw_augmentation(joints, vis, center, scale, o, np_rng, random.Random(6))
    ref = np.random.RandomState(5)
    ref.rand(), ref.randn()
    assert np.array_equal(c, center) and np.array_equal(s, scale * np.clip(ref.randn() * 0.35 + 1, 0.65, 1.35))
    with pytest.raises(KeyError):
        D.draw_augmentation(joints, vis, center, scale, {k: v for k, v in OPTS.items() if k != 'flip'},
                            np.random.RandomState(0), random.Random(0))


def _clip(frames):
    return {'frames': frames, 'joints': np.zeros((17, 3), np.float32), 'joints_vis': np.ones((17, 3), np.float32),
            'center': np.array([30.0, 20.0]), 'scale': np.array([0.3, 0.4]), 'rot': 0.0, 'flip': False}


def test_clip_batcher_refuses_before_any_device_work(monkeypatch):
    """CPU frames, a wrong frame count, mixed sizes inside a clip, more samples than batch_size, non-uint8 frames: each
    raises from the checks alone -- no buffer is allocated and no entry point is called."""
    from fami_pose_amd import _lib
    b = D.ClipBatcher(2, 3, (40, 52))
    called = []
    monkeypatch.setattr(_lib._Lib, 'call', lambda self, name, *a: called.append(name))
    monkeypatch.setattr(D.ClipBatcher, '_buffers', lambda self: called.append('_buffers'))
    f = torch.zeros(60, 90, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='CUDA'):
        b.prepare([_clip([f, f, f])])
    with pytest.raises(ValueError, match='frames'):
        b.prepare([_clip([f, f])])
    with pytest.raises(ValueError, match='sizes'):
        b.prepare([_clip([f, f, torch.zeros(60, 91, 3, dtype=torch.uint8)])])
    with pytest.raises(ValueError, match='samples'):
        b.prepare([_clip([f, f, f])] * 3)
    with pytest.raises(ValueError, match='samples'):
        b.prepare([])
    with pytest.raises(RuntimeError, match='uint8'):
        b.prepare([_clip([f, f, f.float()])])
    with pytest.raises(ValueError):
        b.prepare([_clip([f, f, f[:, :, :2]])])
    assert called == []
    with pytest.raises(RuntimeError):
        D.ClipBatcher(2, 3, (40, 52), device='cpu')
    with pytest.raises(ValueError):
        D.ClipBatcher(0, 3, (40, 52))


def test_library_exports_the_batched_entry_point():
    from fami_pose_amd import _lib
    from fami_pose_amd._lib import lib
    protos = _lib.parse_header()
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('fami_warp_normalize_batch_u8', 'fami_warp_batch_table_bytes'):
        assert name in protos and hasattr(cdll, name), name
    assert len(protos['fami_warp_normalize_batch_u8'][1]) == 15
    L = lib()
    # 64-byte records, then one pointer per (clip, frame); the structured dtype of data.py is the header's struct
    assert D._CLIP_REC.itemsize == 64 and D._CLIP_REC.fields['flip'][1] == 48 and D._CLIP_REC.fields['Ws'][1] == 56
    assert L.cdll.fami_warp_batch_table_bytes(4, 5) == 4 * 64 + 4 * 5 * 8
    assert L.cdll.fami_warp_batch_table_bytes(32, 5) == 32 * 64 + 32 * 5 * 8
    assert L.cdll.fami_warp_batch_table_bytes(0, 5) == -1 and L.cdll.fami_warp_batch_table_bytes(4, 0) == -1
    # argument checks: FAMI_ERR without a launch (no device needed to get here)
    one = ctypes.c_void_p(64)          # a non-null address that is never dereferenced: every call below is refused
    ok = (1, 1, 8, 8, 0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, None)
    bad = [
        (None, one, one) + ok,                                                  # null table
        (one, None, one) + ok,                                                  # null key
        (one, one, None, 1, 2) + ok[2:],                                        # null sup with F = 2
        (one, one, one, 0) + ok[1:],                                            # B = 0
        (one, one, one, 1, 0) + ok[2:],                                         # F = 0
        (one, one, one, 1, 1, 1 << 16, 1 << 15) + ok[4:],                       # Hd * Wd = 2^31
        (one, one, one, 1, 1, 8, 8, 0, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0, None),     # zero std
    ]
    for args in bad:
        assert L.cdll.fami_warp_normalize_batch_u8(*args) == -1, args
        assert b'fami_warp_normalize_batch_u8' in L.cdll.fami_last_error()
