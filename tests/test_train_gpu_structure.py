"""Trainer(structure_cos_weight=, structure_pairs=, structure_min_len=): the structure (limb-direction cosine) term on the
MI355X, eager launches and hipGraph replay.  Test for test tests/test_train_gpu_integral.py with its sizes, helpers and
tolerances (W48, S = 2, 128x96, B = 2; every Trainer compared runs model.set_deterministic(True), so equal launch sequences give
equal bits; 1e-6 relative is for scales that are equal in exact arithmetic and rounded differently)."""
import pytest
import torch

from fami_pose_amd import loss as FL
from fami_pose_amd.data import LIMB_PAIRS
from test_train_gpu_clip import H, W, _batch, _model, _relerr, _trainer

pytestmark = pytest.mark.gpu
HM = (W // 4, H // 4)
WS = 0.5          # the weight of the term in these tests
SEAM = ('softargmax', 'integral', 'heatmap_xy', 'wmse', 'structure')


def _record(monkeypatch):
    from fami_pose_amd._lib import lib
    names = []
    L = lib()
    call, call_routed = L.call, L.call_routed
    monkeypatch.setattr(L, 'call', lambda name, *a: (names.append(name), call(name, *a))[1])
    monkeypatch.setattr(L, 'call_routed', lambda route, name, *a: (names.append(name), call_routed(route, name, *a))[1])
    return names


def test_default_trainer_launches_none_of_it(dev, monkeypatch):
    names = _record(monkeypatch)
    tr = _trainer(dev, False)
    assert tr.structure_cos_weight is None and tr.structure_loss is None and tr.structure_cosines() is None
    assert not tr.head.bufs and tr.head.pairs_dev is None
    tr.step(*_batch(dev))
    torch.cuda.synchronize(dev)
    assert names and not [n for n in names if any(k in n for k in ('structure', 'softargmax', 'heatmap_xy'))]
    assert tr.structure_loss_value() == 0.0 and tr.structure_cosines() is None and not tr.head.bufs
    # with the option: the three forward launches behind the heatmap loss, the two seed launches directly behind the MSE seed
    names.clear()
    tr = _trainer(dev, False, structure_cos_weight=WS)
    tr.step(*_batch(dev))
    torch.cuda.synchronize(dev)
    seam = [n for n in names if any(k in n for k in SEAM)]
    assert seam == ['fami_wmse_fwd_f32', 'fami_softargmax_fwd_f32', 'fami_heatmap_xy_f32', 'fami_structure_cos_fwd_f32',
                    'fami_wmse_bwd_f32', 'fami_structure_cos_bwd_f32', 'fami_softargmax_bwd_f32']
    i = names.index('fami_wmse_bwd_f32')
    assert names[i + 1:i + 3] == ['fami_structure_cos_bwd_f32', 'fami_softargmax_bwd_f32'] and names[i + 3].startswith('fami_nchw_to_nhwc')
    assert tr.integral_loss is None and tr.integral_loss_value() == 0.0
    # with the integral term as well: ONE soft-argmax and ONE target position launch, shared
    names.clear()
    tr = _trainer(dev, False, structure_cos_weight=WS, integral_l1_weight=0.25)
    tr.step(*_batch(dev))
    torch.cuda.synchronize(dev)
    seam = [n for n in names if any(k in n for k in SEAM)]
    assert seam == ['fami_wmse_fwd_f32', 'fami_softargmax_fwd_f32', 'fami_heatmap_xy_f32', 'fami_integral_l1_fwd_f32',
                    'fami_structure_cos_fwd_f32', 'fami_wmse_bwd_f32', 'fami_integral_l1_bwd_f32', 'fami_structure_cos_bwd_f32',
                    'fami_softargmax_bwd_f32']
    i = names.index('fami_wmse_bwd_f32')
    assert names[i + 4].startswith('fami_nchw_to_nhwc')
    assert tr.integral_loss_value() > 0 and tr.structure_loss_value() > 0
    assert tr.loss_value() == pytest.approx(tr._total_loss(tr.loss_parts.tolist()) + tr.integral_loss_value() + tr.structure_loss_value(), rel=1e-6)


_eager = {}


def _eager_pair(dev, monkeypatch):
    """One Trainer step and, from the same start, the eager path: model(...) under autograd, JointMSELoss + WS *
    StructureCosineSimilarity + the MI terms, backward().  -> the relative differences (computed once)

    Both sides run with FAMI_MERGE_PREDICTORS=0, for the reason tests/test_train_gpu_integral.py::_eager_pair gives: on the
    two-convolution predictor route the final maps are equal bit for bit, hence the coordinates and the gcoords, and the 1e-6 of
    that file applies.  The gradient-arena difference WITHOUT the term is measured in the same run (a Trainer without it against
    the eager path without it) and printed beside the one with it."""
    if _eager:
        return _eager
    monkeypatch.setenv('FAMI_MERGE_PREDICTORS', '0')
    kf, sup, joints, vis = _batch(dev)
    tr = _trainer(dev, False, deterministic=True, structure_cos_weight=WS)
    final = tr.step(kf, sup, joints, vis)[0]
    plain = _trainer(dev, False, deterministic=True)          # a Trainer without the term, same start
    plain.step(kf, sup, joints, vis)
    names = {id(p): n for n, p in tr.model.named_parameters()}

    def eager(with_term):
        model = _model().to(dev)
        model.set_deterministic(True)
        f, k, mi = model(kf, sup)
        t, w = FL.generate_heatmaps(joints, vis, 3, (W, H), HM)
        txy = FL.heatmap_xy(joints, (W, H), HM)
        mse = FL.JointMSELoss()(f, t, w)
        term = FL.StructureCosineSimilarity()(f, txy, w) if with_term else None
        total = mse + 0.5 * (-0.1 * mi[0] + 0.1 * mi[1] + mi[2] - mi[3] + mi[4] - mi[5])
        if with_term:
            total = total + WS * term
        total.backward()
        params = dict(model.named_parameters())
        want = torch.zeros_like(tr.grad)
        for p, o, n in tr.table:
            want[o:o + n] = params[names[id(p)]].grad.reshape(-1)
        return f.detach(), mse, term, mi, total, want, txy, w

    f, mse, term, mi, total, want, txy, w = eager(True)
    want_plain = eager(False)[5]
    cosv = tr.structure_cosines()
    _eager.update(
        final=_relerr(f, final), mse=abs(tr.loss_parts[0].item() - mse.item()) / abs(mse.item()),
        term=abs(tr.structure_loss_value() - WS * term.item()) / abs(WS * term.item()),
        mi=max(abs(tr.loss_parts[1 + i].item() - mi[i].item()) / abs(mi[i].item()) for i in range(6)),
        total=abs(tr.loss_value() - total.item()) / abs(total.item()), grad=_relerr(tr.grad, want),
        grad_without=_relerr(plain.grad, want_plain), term_value=term.item(),
        cos_equal=torch.equal(torch.nan_to_num(cosv, nan=7.0),
                              torch.nan_to_num(FL.limb_cosines(FL.soft_argmax(final), txy, w), nan=7.0)),
        cos_shape=tuple(cosv.shape), cos_valid=int((~torch.isnan(cosv)).sum()),
        plain_parts_equal=torch.equal(plain.loss_parts, tr.loss_parts), plain_grad=_relerr(plain.grad, tr.grad))
    print('structure_cos_weight=%.2f against the eager path: final map %.3g, mse %.3g, structure term %.3g, MI %.3g, total %.3g, '
          'gradient arena %.3g (without the term, same run: %.3g) (relative)'
          % tuple([WS] + [_eager[k] for k in ('final', 'mse', 'term', 'mi', 'total', 'grad', 'grad_without')]))
    return _eager


def test_step_losses_match_the_eager_recomputation(dev, monkeypatch):
    e = _eager_pair(dev, monkeypatch)
    assert e['term_value'] > 0 and max(e['final'], e['mse'], e['term'], e['mi'], e['total']) <= 1e-6
    assert e['cos_equal'] and e['cos_shape'] == (2, len(LIMB_PAIRS)) and 0 < e['cos_valid'] < 2 * len(LIMB_PAIRS)
    # the term is really in the gradient: a Trainer without it has the same loss parts and another gradient
    assert e['plain_parts_equal'] and e['plain_grad'] > 1e-4


def test_step_gradients_match_the_eager_recomputation(dev, monkeypatch):
    """The gradient arena of the Trainer step against the eager path's parameter gradients, max |difference| over max |gradient|,
    at the 1e-6 of tests/test_train_gpu_integral.py, both on the two-convolution predictor route (_eager_pair says why); the
    difference without the term, from the same run, is printed beside it."""
    e = _eager_pair(dev, monkeypatch)
    print('gradient arena against the eager path: %.3g with the term, %.3g without' % (e['grad'], e['grad_without']))
    assert e['grad'] <= 1e-6


def test_graph_replay_equals_eager_launches(dev):
    runs = []
    for use_graph in (False, True):
        tr = _trainer(dev, use_graph, deterministic=True, lr=1e-3, structure_cos_weight=WS, integral_beta=12.0)
        vals = []
        for k in range(3):
            tr.step(*_batch(dev, 9 + k % 2))
            vals.append((tr.structure_loss.clone(), torch.nan_to_num(tr.structure_cosines(), nan=7.0), tr.loss_parts.clone()))
        torch.cuda.synchronize(dev)
        runs.append((tr.flat.detach().clone(), tr.grad.detach().clone(), vals))
        if use_graph:
            assert len(tr._cache) == 1
    (f0, g0, v0), (f1, g1, v1) = runs
    assert torch.equal(f0, f1) and torch.equal(g0, g1)
    assert all(torch.equal(a, b) for x, y in zip(v0, v1) for a, b in zip(x, y))
    assert v0[0][0].item() > 0 and not torch.equal(v0[0][1], v0[2][1])


@pytest.mark.parametrize('use_graph', [False, True], ids=['eager', 'graph'])
def test_loss_scale_leaves_the_gradients_bitwise(dev, use_graph):
    """loss_scale = 4 multiplies every seed by a power of two and the pass over the arena divides it out again"""
    a = _trainer(dev, use_graph, deterministic=True, structure_cos_weight=WS)
    b = _trainer(dev, use_graph, deterministic=True, structure_cos_weight=WS, loss_scale=4.0)
    a.step(*_batch(dev))
    b.step(*_batch(dev))
    assert torch.equal(a.grad, b.grad) and torch.equal(a.structure_loss, b.structure_loss) and torch.equal(a.loss_parts, b.loss_parts)


def test_window_loss_includes_the_term(dev):
    tr = _trainer(dev, True, deterministic=True, structure_cos_weight=WS, accum_steps=2)
    assert 'structure_loss_sum' not in tr.accum_state_dict()
    per_call, terms = [], []
    for k in range(2):
        tr.step(*_batch(dev, 9 + k))
        per_call.append(tr.loss_value())
        terms.append(tr.structure_loss_value())
        if k == 0:
            sd = tr.accum_state_dict()
            assert sd['position'] == 1 and sd['structure_loss_sum'].item() == pytest.approx(terms[0], rel=1e-6)
            assert 'integral_loss_sum' not in sd
    assert terms[0] > 0 and terms[0] != terms[1]
    assert tr.window_loss_value() == pytest.approx(sum(per_call) / 2, rel=1e-6)
    assert tr.head.structure.window[1].item() == pytest.approx(sum(terms), rel=1e-6)
    assert tr.loss_parts.numel() == 7 and tr._window_loss.shape == (2, 7)
    # without the option the checkpoint entry has no such key, inside a window too ...
    off = _trainer(dev, False, accum_steps=2)
    off.step(*_batch(dev))
    sd_off = off.accum_state_dict()
    assert off.window_position == 1 and set(sd_off) == {'steps', 'position', 'arena', 'loss_sum'}
    # ... and a Trainer with the term refuses such a checkpoint, as for the integral sum
    with pytest.raises(ValueError, match='without the structure cosine term'):
        tr.load_accum_state_dict(sd_off)
    tr.load_accum_state_dict(sd)
    assert tr.window_position == 1 and tr.head.structure.window[0].item() == pytest.approx(terms[0], rel=1e-6)


def test_ohkm_selection_is_unaffected_and_the_term_reads_the_target_weights(dev):
    bt = _batch(dev)
    both = _trainer(dev, True, deterministic=True, ohkm_topk=8, structure_cos_weight=WS)
    ohkm = _trainer(dev, True, deterministic=True, ohkm_topk=8)
    term = _trainer(dev, True, deterministic=True, structure_cos_weight=WS)
    for tr in (both, ohkm, term):
        tr.step(*bt)
    assert torch.equal(both.ohkm_selection(), ohkm.ohkm_selection()) and torch.equal(both.loss_parts, ohkm.loss_parts)
    assert both.ohkm_selection().sum().item() < (bt[3] != 0).sum().item()          # the selection drops visible joints ...
    assert torch.equal(both.structure_loss, term.structure_loss)                       # ... the term still counts them
    a, b = both.structure_cosines(), term.structure_cosines()
    assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0))
    assert not torch.equal(both.grad, ohkm.grad) and not torch.equal(both.grad, term.grad)
