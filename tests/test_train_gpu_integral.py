"""Trainer(integral_l1_weight=, integral_beta=): the integral L1 coordinate term on the MI355X, eager launches and hipGraph
replay.  Sizes and helpers are those of tests/test_train_gpu_loss_options.py (W48, S = 2, 128x96, B = 2), and so are the
tolerances: every Trainer here runs model.set_deterministic(True), so equal launch sequences give equal bits; 1e-6 relative is
for scales that are equal in exact arithmetic and rounded differently (mse_weight / (B L J) against 1 / (B L) / J, a weight
folded into the scale against one multiplied afterwards)."""
import pytest
import torch

from fami_pose_amd import loss as FL
from test_train_gpu_clip import H, W, _batch, _model, _relerr, _trainer

pytestmark = pytest.mark.gpu
HM = (W // 4, H // 4)
WI = 0.5          # the weight of the term in these tests


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
    assert tr.integral_l1_weight is None and tr.integral_loss is None and tr.integral_coords() is None and not tr.head.bufs
    tr.step(*_batch(dev))
    torch.cuda.synchronize(dev)
    assert names and not [n for n in names if 'softargmax' in n or 'integral' in n or 'heatmap_xy' in n]
    assert tr.integral_loss_value() == 0.0 and tr.integral_coords() is None
    # ... and with the option: the three forward launches behind the heatmap loss, the seed directly behind the MSE seed
    names.clear()
    tr = _trainer(dev, False, integral_l1_weight=WI)
    tr.step(*_batch(dev))
    torch.cuda.synchronize(dev)
    seam = [n for n in names if 'softargmax' in n or 'integral' in n or 'heatmap_xy' in n or 'wmse' in n]
    assert seam == ['fami_wmse_fwd_f32', 'fami_softargmax_fwd_f32', 'fami_heatmap_xy_f32', 'fami_integral_l1_fwd_f32',
                    'fami_wmse_bwd_f32', 'fami_integral_l1_bwd_f32']
    i = names.index('fami_wmse_bwd_f32')
    assert names[i + 1] == 'fami_integral_l1_bwd_f32' and names[i + 2].startswith('fami_nchw_to_nhwc')


_eager = {}


def _eager_pair(dev, monkeypatch):
    """One Trainer step and, from the same start, the eager path: model(...) under autograd, JointMSELoss + WI * IntegralL1Loss +
    the MI terms, backward().  -> the relative differences (computed once)

    Both sides run with FAMI_MERGE_PREDICTORS=0.  A Trainer runs the offset and the mask predictor of a DCN layer as ONE
    convolution (engine.CatParam), which needs its gradient arena; a model called under autograd has none and runs two.  The
    1e-6 of tests/test_train_gpu_loss_options.py is for equal launch sequences, and across that one difference the final maps
    already sit 3.85e-7 of their maximum apart and the gradient arenas 1.19e-6 WITHOUT the term, 1.25e-6 with it (measured; the
    soft-argmax multiplies a distance in the map by beta).  On the two-convolution route the final maps are equal bit for bit
    and the arenas 5.4e-7 apart with the term, 6.0e-7 without (the Trainer seeds the repeated MI term once with the summed
    coefficient, autograd twice).  The merged route against the
    two-convolution route is tests/test_train_gpu.py::test_merged_predictors_match_the_two_convolution_path."""
    if _eager:
        return _eager
    monkeypatch.setenv('FAMI_MERGE_PREDICTORS', '0')
    kf, sup, joints, vis = _batch(dev)
    tr = _trainer(dev, False, deterministic=True, integral_l1_weight=WI)
    final = tr.step(kf, sup, joints, vis)[0]
    model = _model().to(dev)
    model.set_deterministic(True)
    f, k, mi = model(kf, sup)
    t, w = FL.generate_heatmaps(joints, vis, 3, (W, H), HM)
    txy = FL.heatmap_xy(joints, (W, H), HM)
    mse, integral = FL.JointMSELoss()(f, t, w), FL.IntegralL1Loss()(f, txy, w)
    total = mse + WI * integral + 0.5 * (-0.1 * mi[0] + 0.1 * mi[1] + mi[2] - mi[3] + mi[4] - mi[5])
    total.backward()
    names = {id(p): n for n, p in tr.model.named_parameters()}
    eager = dict(model.named_parameters())
    want = torch.zeros_like(tr.grad)
    for p, o, n in tr.table:
        want[o:o + n] = eager[names[id(p)]].grad.reshape(-1)
    # a Trainer without the term, same start
    plain = _trainer(dev, False, deterministic=True)
    plain.step(kf, sup, joints, vis)
    _eager.update(
        final=_relerr(f.detach(), final), mse=abs(tr.loss_parts[0].item() - mse.item()) / abs(mse.item()),
        term=abs(tr.integral_loss_value() - WI * integral.item()) / abs(WI * integral.item()),
        mi=max(abs(tr.loss_parts[1 + i].item() - mi[i].item()) / abs(mi[i].item()) for i in range(6)),
        total=abs(tr.loss_value() - total.item()) / abs(total.item()), grad=_relerr(tr.grad, want),
        term_value=integral.item(), coords_equal=torch.equal(tr.integral_coords(), FL.soft_argmax(final)),
        coords_shape=tuple(tr.integral_coords().shape), plain_parts_equal=torch.equal(plain.loss_parts, tr.loss_parts),
        plain_grad=_relerr(plain.grad, tr.grad))
    print('integral_l1_weight=%.2f against the eager path: final map %.3g, mse %.3g, integral term %.3g, MI %.3g, total %.3g, '
          'gradient arena %.3g (relative)' % tuple([WI] + [_eager[k] for k in ('final', 'mse', 'term', 'mi', 'total', 'grad')]))
    return _eager


def test_step_losses_match_the_eager_recomputation(dev, monkeypatch):
    e = _eager_pair(dev, monkeypatch)
    assert e['term_value'] > 0 and max(e['final'], e['mse'], e['term'], e['mi'], e['total']) <= 1e-6
    assert e['coords_equal'] and e['coords_shape'] == (2, 17, 2)
    # the term is really in the gradient: a Trainer without it has the same loss parts and another gradient
    assert e['plain_parts_equal'] and e['plain_grad'] > 1e-4


def test_step_gradients_match_the_eager_recomputation(dev, monkeypatch):
    """The gradient arena of the Trainer step against the eager path's parameter gradients, max |difference| over max |gradient|,
    at the 1e-6 of tests/test_train_gpu_loss_options.py, both on the two-convolution predictor route (_eager_pair says why)."""
    e = _eager_pair(dev, monkeypatch)
    assert e['grad'] <= 1e-6


def test_graph_replay_equals_eager_launches(dev):
    runs = []
    for use_graph in (False, True):
        tr = _trainer(dev, use_graph, deterministic=True, lr=1e-3, integral_l1_weight=WI, integral_beta=12.0)
        vals = []
        for k in range(3):
            tr.step(*_batch(dev, 9 + k % 2))
            vals.append((tr.integral_loss.clone(), tr.integral_coords().clone(), tr.loss_parts.clone()))
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
    """loss_scale = 4 multiplies both seeds by a power of two and the pass over the arena divides it out again"""
    a = _trainer(dev, use_graph, deterministic=True, integral_l1_weight=WI)
    b = _trainer(dev, use_graph, deterministic=True, integral_l1_weight=WI, loss_scale=4.0)
    a.step(*_batch(dev))
    b.step(*_batch(dev))
    assert torch.equal(a.grad, b.grad) and torch.equal(a.integral_loss, b.integral_loss) and torch.equal(a.loss_parts, b.loss_parts)


def test_window_loss_includes_the_term(dev):
    tr = _trainer(dev, True, deterministic=True, integral_l1_weight=WI, accum_steps=2)
    assert 'integral_loss_sum' not in tr.accum_state_dict()
    per_call, terms = [], []
    for k in range(2):
        tr.step(*_batch(dev, 9 + k))
        per_call.append(tr.loss_value())
        terms.append(tr.integral_loss_value())
        if k == 0:
            sd = tr.accum_state_dict()
            assert sd['position'] == 1 and sd['integral_loss_sum'].item() == pytest.approx(terms[0], rel=1e-6)
    assert terms[0] > 0 and terms[0] != terms[1]
    assert tr.window_loss_value() == pytest.approx(sum(per_call) / 2, rel=1e-6)
    assert tr.head.integral.window[1].item() == pytest.approx(sum(terms), rel=1e-6)
    assert tr.loss_parts.numel() == 7 and tr._window_loss.shape == (2, 7)
    # without the option the checkpoint entry has no such key, inside a window too
    off = _trainer(dev, False, accum_steps=2)
    off.step(*_batch(dev))
    assert off.window_position == 1 and set(off.accum_state_dict()) == {'steps', 'position', 'arena', 'loss_sum'}


def test_ohkm_selection_is_unaffected_and_the_term_reads_the_target_weights(dev):
    bt = _batch(dev)
    both = _trainer(dev, True, deterministic=True, ohkm_topk=8, integral_l1_weight=WI)
    ohkm = _trainer(dev, True, deterministic=True, ohkm_topk=8)
    term = _trainer(dev, True, deterministic=True, integral_l1_weight=WI)
    for tr in (both, ohkm, term):
        tr.step(*bt)
    assert torch.equal(both.ohkm_selection(), ohkm.ohkm_selection()) and torch.equal(both.loss_parts, ohkm.loss_parts)
    assert both.ohkm_selection().sum().item() < (bt[3] != 0).sum().item()          # the selection drops visible joints ...
    assert torch.equal(both.integral_loss, term.integral_loss)                         # ... the term still counts them
    assert torch.equal(both.integral_coords(), term.integral_coords())
    assert not torch.equal(both.grad, ohkm.grad) and not torch.equal(both.grad, term.grad)
