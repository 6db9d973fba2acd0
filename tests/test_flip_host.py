"""Host logic of flip testing (fami_pose_amd.evaluate): the joint permutation of flip_back
(datasets/process/pose_process.py:29-42) as one gather, and the reference's four switches
(posetimation/config/mppe_config.py:322,329,340,346) read per phase."""
import pytest

import fami_pose_amd as fp
from fami_pose_amd import evaluate as ev
from fami_pose_amd.data import FLIP_PAIRS


def test_flip_perm_coco():
    assert ev.flip_perm(17) == [0, 1, 2, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15]
    assert ev.flip_perm(17, FLIP_PAIRS) == ev.flip_perm(17)
    assert ev.flip_perm(5, ()) == [0, 1, 2, 3, 4]
    assert ev.flip_perm(5, ((0, 4), (1, 2))) == [4, 2, 1, 3, 0]
    p = ev.flip_perm(17)
    assert [p[p[j]] for j in range(17)] == list(range(17))          # an involution: flipping back twice is the identity


@pytest.mark.parametrize('pairs', [((0, 5),), ((-1, 2),), ((3, 17),),      # an index outside [0, J)
                                   ((0, 1), (1, 2)), ((0, 1), (2, 0)), ((0, 1), (0, 1)),      # a joint that occurs twice
                                   ((2, 2),)])                             # a joint paired with itself
def test_flip_perm_rejects(pairs):
    J = 17 if pairs == ((3, 17),) else 5
    with pytest.raises(ValueError):
        ev.flip_perm(J, pairs)


def test_default_cfg_carries_the_switches_off():
    cfg = fp.default_cfg(48)
    assert cfg.VAL.FLIP_VAL is False and cfg.VAL.SHIFT_HEATMAP is False
    assert cfg.TEST.FLIP_TEST is False and cfg['TEST']['SHIFT_HEATMAP'] is False
    for phase in (fp.VAL_PHASE, fp.TEST_PHASE):
        assert ev.flip_test_options(cfg, phase) == {'flip': False, 'shift_heatmap': False}


def test_flip_test_options_per_phase():
    cfg = fp.default_cfg(48)
    cfg.VAL.FLIP_VAL = True
    cfg.TEST.SHIFT_HEATMAP = True
    assert ev.flip_test_options(cfg, fp.VAL_PHASE) == {'flip': True, 'shift_heatmap': False}
    assert ev.flip_test_options(cfg, fp.TEST_PHASE) == {'flip': False, 'shift_heatmap': True}
    cfg.VAL.SHIFT_HEATMAP = True
    cfg.TEST.FLIP_TEST = True
    assert ev.flip_test_options(cfg, fp.VAL_PHASE) == {'flip': True, 'shift_heatmap': True}
    assert ev.flip_test_options(cfg, fp.TEST_PHASE) == {'flip': True, 'shift_heatmap': True}
    cfg.VAL.FLIP_VAL = False                                        # each phase reads its own node only
    assert ev.flip_test_options(cfg, fp.VAL_PHASE) == {'flip': False, 'shift_heatmap': True}
    assert ev.flip_test_options(cfg, fp.TEST_PHASE) == {'flip': True, 'shift_heatmap': True}
    with pytest.raises(ValueError):
        ev.flip_test_options(cfg, fp.TRAIN_PHASE)


def test_flip_test_options_missing_node_or_key():
    cfg = fp.default_cfg(48)
    del cfg['VAL']
    del cfg['TEST']['SHIFT_HEATMAP']
    cfg.TEST.FLIP_TEST = True
    assert ev.flip_test_options(cfg, fp.VAL_PHASE) == {'flip': False, 'shift_heatmap': False}
    assert ev.flip_test_options(cfg, fp.TEST_PHASE) == {'flip': True, 'shift_heatmap': False}
    assert ev.flip_test_options(fp.CfgNode(), fp.TEST_PHASE) == {'flip': False, 'shift_heatmap': False}
    assert ev.flip_test_options({'VAL': {'SHIFT_HEATMAP': True}}, fp.VAL_PHASE) == {'flip': False, 'shift_heatmap': True}


def test_signatures_keep_the_plain_call():
    """The option is opt-in: the new keywords default to the plain path."""
    import inspect
    for fn in (ev.predict, ev.evaluate_loop):
        ps = inspect.signature(fn).parameters
        assert ps['flip'].default is False and ps['shift_heatmap'].default is False
        assert ps['flip_pairs'].default == FLIP_PAIRS
