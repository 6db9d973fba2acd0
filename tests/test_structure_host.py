"""The structure (limb-direction cosine) term without a GPU: the float64 restatement (tests/_structure_ref.py) against numbers
derived by hand and against torch.nn.functional.cosine_similarity under autograd, the option checks, data.LIMB_PAIRS and the
configuration keys."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _structure_ref as sr  # noqa: E402

import fami_pose_amd as fp  # noqa: E402
from fami_pose_amd import loss as FL  # noqa: E402
from fami_pose_amd.data import FLIP_PAIRS, LIMB_PAIRS  # noqa: E402
from fami_pose_amd.train import Trainer  # noqa: E402

ONE = ((0, 1),)


def _two(u, t, w=(1.0, 1.0)):
    """one sample, one limb 0 -> 1 with predicted direction u and target direction t, joint 0 at (3, 4)"""
    c = np.array([[[3.0, 4.0], [3.0 + u[0], 4.0 + u[1]]]], np.float32)
    x = np.array([[[3.0, 4.0], [3.0 + t[0], 4.0 + t[1]]]], np.float32)
    return c, x, np.array([w], np.float32)


# ------------------------------------------------------------------------------------------ hand-derived numbers
def test_parallel_antiparallel_and_orthogonal_limbs():
    assert sr.rows(*_two((3, 4), (3, 4)), ONE)[0, 0] == 0.0                # u = t: 25 / (5 * 5)
    assert sr.rows(*_two((-3, -4), (3, 4)), ONE)[0, 0] == 2.0              # u = -t
    c, x, w = _two((1, 0), (0, 2))
    valid, cos, d = sr.limbs(c, x, w, ONE)
    assert valid[0, 0] and cos[0, 0] == 0.0 and sr.rows(c, x, w, ONE)[0, 0] == 1.0
    # dcos/du = t / (|u| |t|) - cos u / |u|^2 = (0, 2) / 2 - 0 = (0, 1)
    assert d[0, 0].tolist() == [0.0, 1.0]
    # d(1 - cos)/dc_b = -(0, 1), at c_a the opposite; the scale multiplies
    g = sr.gcoords(c, x, w, ONE, 0.5)
    assert g[0].tolist() == [[0.0, 0.5], [0.0, -0.5]]
    assert sr.gcoords(c, x, w, ONE, 0.5, gdev=4.0)[0].tolist() == [[0.0, 2.0], [0.0, -2.0]]
    # a 3-4-5 limb against the x axis: cos = 3/5; dcos/du = (1, 0) / 5 - (3/5) (3, 4) / 25 = (0.2 - 0.072, -0.096)
    c, x, w = _two((3, 4), (2, 0))
    _, cos, d = sr.limbs(c, x, w, ONE)
    assert cos[0, 0] == pytest.approx(0.6, abs=1e-15) and d[0, 0] == pytest.approx([0.128, -0.096], abs=1e-15)


def test_masked_and_short_limbs_give_zero_and_no_gradient():
    for w in ((0.0, 1.0), (1.0, 0.0), (float('nan'), 1.0), (-1.0, 1.0)):
        c, x, wt = _two((1, 0), (0, 2), w)
        assert not sr.limbs(c, x, wt, ONE)[0][0, 0]
        assert sr.rows(c, x, wt, ONE)[0, 0] == 0.0 and not sr.gcoords(c, x, wt, ONE, 1.0).any()
    c, x, w = _two((1, 0), (0, 0.75))                    # shorter than min_len = 1
    assert sr.rows(c, x, w, ONE)[0, 0] == 0.0 and not sr.gcoords(c, x, w, ONE, 1.0).any()
    assert sr.rows(c, x, w, ONE, min_len=0.5)[0, 0] == 1.0          # ... and counted below it
    c, x, w = _two((1, 0), (0, 1.0))                     # exactly min_len: `>` is strict
    assert sr.rows(c, x, w, ONE)[0, 0] == 0.0
    c, x, w = _two((1, 0), (float('nan'), 2.0))           # a NaN target: the comparison is false
    assert sr.rows(c, x, w, ONE)[0, 0] == 0.0 and not sr.gcoords(c, x, w, ONE, 1.0).any()
    assert sr.rows(c, x, None, ONE)[0, 0] == 0.0
    c, x, w = _two((1, 0), (0, 2), (0.0, 0.0))
    assert sr.rows(c, x, None, ONE)[0, 0] == 1.0          # w = None: every weight 1


def test_a_joint_on_two_limbs_sums_both_and_a_free_joint_gets_zero():
    # joints 0, 1, 2 on the chain 0 -> 1 -> 2, joint 3 on no limb; limb 0 -> 1 predicted along x against y, limb 1 -> 2 along y
    # against x: dcos/du = (0, 1) and (1, 0)
    c = np.array([[[0, 0], [1, 0], [1, 1], [7, 7]]], np.float32)
    x = np.array([[[0, 0], [0, 2], [2, 2], [5, 5]]], np.float32)
    w = np.ones((1, 4), np.float32)
    pairs = ((0, 1), (1, 2))
    _, cos, d = sr.limbs(c, x, w, pairs)
    assert cos[0].tolist() == [0.0, 0.0] and d[0].tolist() == [[0.0, 1.0], [1.0, 0.0]]
    g = sr.gcoords(c, x, w, pairs, 1.0)[0]
    # joint 1 is b of limb 0 (-(0, 1)) and a of limb 1 (+(1, 0))
    assert g.tolist() == [[0.0, 1.0], [1.0, -1.0], [-1.0, 0.0], [0.0, 0.0]]
    assert sr.loss(sr.rows(c, x, w, pairs).astype(np.float32), 0.25) == 0.5


def test_a_predicted_limb_within_eps_takes_the_clamp_branch():
    eps = float(np.float32(1e-8))
    c, x, w = _two((0, 0), (0, 2))                       # nu = 0 <= eps: cos = 0 / (eps * 2), dcos/du = t / (eps * 2) = (0, 1 / eps)
    valid, cos, d = sr.limbs(c, x, w, ONE)
    assert valid[0, 0] and cos[0, 0] == 0.0 and d[0, 0].tolist() == [0.0, 2.0 / (eps * 2.0)]
    # a tiny limb along the target: cos = nu nt / (eps nt) = nu / eps, not 1
    tiny = np.float32(2.0 ** -30)
    c = np.array([[[0, 0], [0, tiny]]], np.float32)
    _, cos, d = sr.limbs(c, x, w, ONE)
    assert float(tiny) < eps and cos[0, 0] == pytest.approx(float(tiny) / eps, rel=1e-15) and d[0, 0, 1] == 2.0 / (eps * 2.0)
    big = sr.limbs(c, x, w, ONE, eps=2.0 ** -40)[1][0, 0]          # the same limb above eps: the plain cosine
    assert big == 1.0


# ------------------------------------------------------------------------------------------ independence
def test_restatement_agrees_with_torch_cosine_similarity_under_autograd():
    """40 samples x 5 limbs = 200 rows on a 6-joint tree with shared joints, some weights 0 and some short targets; both sides in
    float64 on the CPU.  They differ only in the order of float64 operations (torch normalises each vector, then takes the dot
    product): 1e-12 on values of order 1."""
    B, J = 40, 6
    pairs = ((0, 1), (1, 2), (1, 3), (3, 4), (5, 3))
    c, x, w = sr.skeleton_case(B, J, pairs, 77)
    rng = np.random.RandomState(5)
    w[rng.rand(B, J) < 0.1] = 0.0
    x[3, 2] = x[3, 1] + np.float32(0.25)                    # a target limb shorter than min_len
    valid, _, _ = sr.limbs(c, x, w, pairs)
    assert valid.sum() >= 120 and (~valid).sum() >= 20
    ct = torch.from_numpy(c.astype(np.float64)).requires_grad_(True)
    xt = torch.from_numpy(x.astype(np.float64))
    a, b = torch.tensor([p[0] for p in pairs]), torch.tensor([p[1] for p in pairs])
    cos = torch.nn.functional.cosine_similarity(ct[:, b] - ct[:, a], xt[:, b] - xt[:, a], dim=-1, eps=float(np.float32(1e-8)))
    l = torch.where(torch.from_numpy(valid), 1.0 - cos, torch.zeros_like(cos))
    (0.125 * l.sum()).backward()
    er = np.abs(l.detach().numpy() - sr.rows(c, x, w, pairs)).max()
    eg = np.abs(ct.grad.numpy() - sr.gcoords(c, x, w, pairs, 0.125)).max()
    print('against torch: row values %.3g, gcoords %.3g' % (er, eg))
    assert er <= 1e-12 and eg <= 1e-12 and np.abs(ct.grad.numpy()).max() > 0.01


# ------------------------------------------------------------------------------------------ options, table, configuration
def test_limb_pairs_table():
    assert len(LIMB_PAIRS) == 16 and len(set(LIMB_PAIRS)) == 16
    joints = {j for p in LIMB_PAIRS for j in p}
    assert max(joints) < 17 and min(joints) >= 0 and 3 not in joints and 4 not in joints
    assert joints == set(range(17)) - {3, 4}
    swap = {}
    for a, b in FLIP_PAIRS:
        swap[a], swap[b] = b, a
    und = {frozenset(p) for p in LIMB_PAIRS}
    assert {frozenset(swap.get(j, j) for j in p) for p in LIMB_PAIRS} == und          # closed under the mirror
    assert FL.check_structure_options(1.0, LIMB_PAIRS, 1.0, 1e-8, 17) == (1.0, LIMB_PAIRS, 1.0, 1e-8)
    assert FL.StructureCosineSimilarity().pairs == LIMB_PAIRS


def test_option_checks():
    ok = FL.check_structure_options(np.float32(0.5), [[0, 1], (np.int64(2), 1)], 0, np.float64(1e-6))
    assert ok == (0.5, ((0, 1), (2, 1)), 0.0, 1e-6)
    for pairs in (((1, 1),), ((0, 17),), ((-1, 2),), tuple((0, 1) for _ in range(65)), (), ((0, 1, 2),), ((0, 1.0),), ((True, 2),), 5):
        with pytest.raises(ValueError):
            FL.check_structure_options(1.0, pairs, 1.0, 1e-8, 17)
    FL.check_structure_options(1.0, ((0, 17),), 1.0, 1e-8, 18)
    FL.check_structure_options(1.0, tuple((0, 1) for _ in range(64)), 1.0, 1e-8, 2)
    for kw in (dict(weight=0.0), dict(weight=-1.0), dict(weight=float('nan')), dict(weight=True), dict(min_len=-0.5),
               dict(min_len=float('inf')), dict(min_len=1e39), dict(eps=0.0), dict(eps=-1e-8), dict(eps=1e-50), dict(eps=float('nan')),
               dict(num_joints=1), dict(num_joints=65)):
        a = dict(weight=1.0, pairs=ONE, min_len=1.0, eps=1e-8, num_joints=17)
        a.update(kw)
        with pytest.raises(ValueError):
            FL.check_structure_options(**a)
    with pytest.raises(ValueError):
        FL.StructureCosineSimilarity(pairs=((2, 2),))
    with pytest.raises(ValueError):
        FL.StructureCosineSimilarity(beta=0.0)


class _NoDevice(torch.nn.Module):
    """a model whose parameters live on the host: a Trainer that got past its argument checks raises RuntimeError"""
    num_joints = 17

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))


def test_trainer_refuses_before_device_work():
    with pytest.raises(ValueError, match='targets_from_joints'):
        Trainer(_NoDevice(), structure_cos_weight=1.0, targets_from_joints=False)
    for kw in (dict(structure_cos_weight=-1.0), dict(structure_cos_weight=0.0), dict(structure_cos_weight=1.0, integral_beta=0.0),
               dict(structure_cos_weight=1.0, structure_pairs=((0, 17),)), dict(structure_cos_weight=1.0, structure_pairs=((3, 3),)),
               dict(structure_cos_weight=1.0, structure_min_len=-1.0)):
        with pytest.raises(ValueError):
            Trainer(_NoDevice(), targets_from_joints=True, **kw)
    with pytest.raises(RuntimeError, match='GPU'):          # good options reach the device check
        Trainer(_NoDevice(), structure_cos_weight=0.5, targets_from_joints=True)
    with pytest.raises(RuntimeError, match='GPU'):          # ... and without the term its options are not looked at
        Trainer(_NoDevice(), structure_pairs=((3, 3),), structure_min_len=-1.0)


def test_from_cfg_maps_the_two_keys(monkeypatch):
    cfg = fp.default_cfg(48)
    assert cfg['LOSS']['STRUCTURE_COSINE'] == {'USE': False, 'WEIGHT': 1.0}
    seen = []
    monkeypatch.setattr(Trainer, '__init__', lambda self, model, **kw: seen.append(kw))
    Trainer.from_cfg(cfg, None)
    assert 'structure_cos_weight' not in seen[-1]
    cfg['LOSS']['STRUCTURE_COSINE'] = {'USE': True, 'WEIGHT': 0.25}
    Trainer.from_cfg(cfg, None)
    assert seen[-1]['structure_cos_weight'] == 0.25 and 'integral_l1_weight' not in seen[-1]
    Trainer.from_cfg(cfg, None, structure_cos_weight=None, structure_min_len=2.0)          # keyword arguments win
    assert seen[-1]['structure_cos_weight'] is None and seen[-1]['structure_min_len'] == 2.0
    cfg['LOSS']['STRUCTURE_COSINE'] = {'USE': True}
    Trainer.from_cfg(cfg, None)
    assert seen[-1]['structure_cos_weight'] == 1.0
    del cfg['LOSS']['STRUCTURE_COSINE']          # a configuration from before the key
    Trainer.from_cfg(cfg, None)
    assert 'structure_cos_weight' not in seen[-1]
