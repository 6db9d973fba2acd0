"""The optimizer front door of the reference on the host (posetimation/optimizer/optimizer.py:16-76,
posetimation/optimizer/scheduler.py:14-27, engine/defaults/checkpoints.py:45-107): TRAIN.OPTIMIZER / LR / MOMENTUM / WD /
NESTEROV / LR_SECOND_GROUP -> optimizer kind, hyper-parameters and learning-rate groups; FlatSGD's host protocol; the
checkpoint converters of SGD and of two Adam groups against real torch optimizers.  CPU only: no kernel is launched."""
import pytest
import torch

import fami_pose_amd as fp
from fami_pose_amd import checkpoint as ck
from fami_pose_amd.config import CfgNode
from fami_pose_amd.train import (FlatAdam, FlatSGD, build_lr_scheduler, build_optimizers, flatten_parameters,
                                 optimizer_kwargs, parameter_groups)


def _cfg(width=48, freeze=False, **train):
    cfg = fp.default_cfg(width, freeze_backbone=freeze)
    cfg['TRAIN'].update(train)
    return cfg


def _names(groups):
    return [[n for n, _ in g] for g in groups]


class _HostTrainer:
    """What checkpoint.py reads of a train.Trainer, built by the Trainer's own optimizer builder, without a GPU."""

    def __init__(self, model, **kw):
        self.flat, self.table = flatten_parameters(model)
        self.optimizers, self.group_rows = build_optimizers(model, self.flat, self.table, **kw)
        self.opt = self.optimizers[0]


def test_front_door_adam_one_group():
    model = fp.build_model(_cfg(), fp.TRAIN_PHASE)
    kw = optimizer_kwargs(_cfg(WD=1e-4))
    assert kw == {'optimizer': 'adam', 'lr': 1e-3, 'lr_groups': None}
    groups = parameter_groups(model, kw['lr_groups'])
    assert _names(groups) == [[n for n, p in model.named_parameters() if p.requires_grad]]
    opts, rows = build_optimizers(model, *flatten_parameters(model), **kw)
    # the reference's Adam is built from `lr` alone (optimizer.py:68): TRAIN.WD does not reach it
    assert len(opts) == 1 and isinstance(opts[0], FlatAdam) and opts[0].wd == 0.0 and opts[0].lr == 1e-3
    assert opts[0].runs == [(0, 64655204)] and rows == [list(range(984))]


def test_front_door_adam_second_group():
    model = fp.build_model(_cfg(), fp.TRAIN_PHASE)
    kw = optimizer_kwargs(_cfg(LR=2e-3, LR_SECOND_GROUP=['hrnet'], LR_SECOND_GROUP_VALUE=1e-5, WD=1e-4))
    assert kw == {'optimizer': 'adam', 'lr': 2e-3, 'lr_groups': [(('hrnet',), 1e-5)]}
    base, second = _names(parameter_groups(model, kw['lr_groups']))
    every = [n for n, _ in model.named_parameters()]
    assert second == [n for n in every if n.startswith('hrnet')] and len(second) == 878
    assert base == [n for n in every if not n.startswith('hrnet')] and len(base) == 106
    flat, table = flatten_parameters(model)
    opts, rows = build_optimizers(model, flat, table, **kw)
    assert [o.lr for o in opts] == [2e-3, 1e-5] and all(o.wd == 0.0 for o in opts)
    # self.hrnet is constructed first: each group is ONE contiguous arena run, so one launch per group and step
    assert opts[1].runs == [(0, 63595745)] and opts[0].runs == [(63595745, 64655204)]
    assert opts[1].m is opts[0].m and opts[1].v is opts[0].v and opts[1].grad is opts[0].grad
    names = [n for n, _ in model.named_parameters()]
    assert [names[i] for i in rows[1]] == second and [names[i] for i in rows[0]] == base


def test_front_door_sgd():
    model = fp.build_model(_cfg(), fp.TRAIN_PHASE)
    kw = optimizer_kwargs(_cfg(OPTIMIZER='sgd'))            # MOMENTUM / WD / NESTEROV missing: defaults.py:137-140
    assert kw == {'optimizer': 'sgd', 'lr': 1e-3, 'momentum': 0.9, 'weight_decay': 1e-4, 'nesterov': False}
    kw = optimizer_kwargs(_cfg(OPTIMIZER='sgd', LR=0.01, MOMENTUM=0.8, WD=5e-4, NESTEROV=True))
    assert kw == {'optimizer': 'sgd', 'lr': 0.01, 'momentum': 0.8, 'weight_decay': 5e-4, 'nesterov': True}
    opts, rows = build_optimizers(model, *flatten_parameters(model), **kw)
    o = opts[0]
    assert len(opts) == 1 and isinstance(o, FlatSGD)
    assert (o.lr, o.momentum, o.dampening, o.wd, o.nesterov) == (0.01, 0.8, 0.0, 5e-4, True)
    assert o.buf is not None and o.buf.numel() == 64655204
    assert _names(parameter_groups(model)) == [[n for n, _ in model.named_parameters()]]


def test_front_door_sgd_frozen_backbone():
    model = fp.build_model(_cfg(16, freeze=True), fp.TRAIN_PHASE)
    kw = optimizer_kwargs(_cfg(16, freeze=True, OPTIMIZER='sgd'))
    (names,) = _names(parameter_groups(model))
    assert names and not any(n.startswith('hrnet') for n in names)
    assert names == [n for n, p in model.named_parameters() if p.requires_grad]
    flat, table = flatten_parameters(model)
    opts, rows = build_optimizers(model, flat, table, **kw)
    assert rows == [list(range(len(names)))] and opts[0].runs == [(0, flat.numel())]


def test_front_door_rejects_what_the_reference_cannot_build():
    with pytest.raises(ValueError, match='TypeError'):
        optimizer_kwargs(_cfg(OPTIMIZER='sgd', LR_SECOND_GROUP=['hrnet']))
    with pytest.raises(ValueError):
        optimizer_kwargs(_cfg(OPTIMIZER='rmsprop'))
    model = fp.build_model(_cfg(16), fp.TRAIN_PHASE)
    flat, table = flatten_parameters(model)
    with pytest.raises(ValueError, match='no trainable parameter'):
        build_optimizers(model, flat, table, lr_groups=[(('no_such_module',), 1e-5)])
    with pytest.raises(ValueError):
        build_optimizers(model, flat, table, optimizer='adam', momentum=0.9)


def test_flat_sgd_host_protocol():
    flat = torch.zeros(1003)
    o = FlatSGD(flat, lr=0.1)
    assert o.buf is None and o.state.tolist() == pytest.approx([0.0, 0.1, 1.0])
    o.set_lr(0.01)
    assert o.hyper_version == 0 and o.lr == 0.01 and o.state[1].item() == pytest.approx(0.01)
    o.set_hyper(momentum=0.9)
    assert o.hyper_version == 1 and o.buf is not None and o.buf.shape == flat.shape
    o.set_hyper(momentum=0.9)
    assert o.hyper_version == 1
    for k, kv in enumerate(({'weight_decay': 1e-4}, {'dampening': 0.1}, {'dampening': 0.0, 'nesterov': True})):
        o.set_hyper(**kv)
        assert o.hyper_version == 2 + k
    with pytest.raises(ValueError, match='Nesterov'):
        o.set_hyper(dampening=0.1)
    assert o.hyper_version == 4 and o.dampening == 0.0
    with pytest.raises(ValueError, match='Nesterov'):
        FlatSGD(flat, lr=0.1, nesterov=True)
    with pytest.raises(ValueError, match='Nesterov'):
        FlatSGD(flat, lr=0.1, momentum=0.9, dampening=0.1, nesterov=True)
    with pytest.raises(ValueError):
        torch.optim.SGD([torch.nn.Parameter(flat.clone())], lr=0.1, nesterov=True)    # (what torch does)


def test_lr_scheduler_per_group():
    model = fp.build_model(_cfg(16), fp.TRAIN_PHASE)
    one = _HostTrainer(model, lr=1e-3)
    s = build_lr_scheduler(_cfg(16, LR_STEP=[1, 2], LR_FACTOR=0.5), one)
    assert not isinstance(s, list) and s.opt is one.opt
    two = _HostTrainer(model, lr=1e-3, lr_groups=[(('hrnet',), 1e-5)])
    ss = build_lr_scheduler(_cfg(16, LR_STEP=[1, 2], LR_FACTOR=0.5), two)
    assert isinstance(ss, list) and [x.opt for x in ss] == two.optimizers
    for x in ss:
        x.step()
    assert two.optimizers[0].lr == pytest.approx(5e-4) and two.optimizers[1].lr == pytest.approx(5e-6)


def _fill(t, seed):
    t.copy_(torch.randn(t.shape, generator=torch.Generator().manual_seed(seed)))


@pytest.mark.parametrize('momentum', [0.0, 0.9])
def test_sgd_state_round_trips_through_torch(tmp_path, momentum):
    model = fp.build_model(_cfg(16), fp.TRAIN_PHASE)
    tr = _HostTrainer(model, optimizer='sgd', lr=0.02, momentum=momentum, weight_decay=1e-4)
    if momentum:
        _fill(tr.opt.buf, 1)
    tr.opt.state.copy_(torch.tensor([3.0, 0.02, 1.0]))
    (sd,) = ck.optimizer_state_dicts(tr)
    g = sd['param_groups'][0]
    assert list(g) == ['lr', 'initial_lr', 'momentum', 'dampening', 'weight_decay', 'nesterov', 'maximize', 'foreach',
                       'differentiable', 'fused', 'params']
    # a real torch.optim.SGD on the same parameters takes it, and its own state_dict() comes back
    ps = [p for p in model.parameters() if p.requires_grad]
    opt = torch.optim.SGD(ps, lr=0.5, momentum=momentum, weight_decay=1e-4)
    opt.load_state_dict(sd)
    assert opt.param_groups[0]['lr'] == pytest.approx(0.02) and opt.param_groups[0]['momentum'] == momentum
    tsd = opt.state_dict()
    if momentum:
        assert len(tsd['state']) == len(ps)
        for i, (p, off, n) in enumerate(tr.table):
            assert torch.equal(tsd['state'][i]['momentum_buffer'], tr.opt.buf[off:off + n].view(p.shape))
    else:
        assert tsd['state'] == {} and sd['state'] == {}
    tr2 = _HostTrainer(model, optimizer='sgd', lr=1.0)
    ck.load_optimizer_state_dicts(tr2, [tsd])
    o = tr2.opt
    assert (o.lr, o.momentum, o.wd, o.nesterov) == (pytest.approx(0.02), momentum, 1e-4, False)
    assert o.hyper_version == 1          # the kernel arguments changed: a graph-mode Trainer re-captures
    if momentum:
        assert torch.equal(o.buf, tr.opt.buf)
        assert o.state[0].item() >= 1.0                        # the next update takes the running rule
    else:
        assert o.buf is None and o.state[0].item() == 0.0
    # the other kind is refused, naming both
    with pytest.raises(ValueError, match='adam.*sgd|sgd.*adam'):
        ck.load_optimizer_state_dicts(_HostTrainer(model, lr=1e-3), [tsd])
    with pytest.raises(ValueError, match='adam.*sgd|sgd.*adam'):
        ck.load_optimizer_state_dicts(tr2, ck.optimizer_state_dicts(_HostTrainer(model, lr=1e-3)))


def test_two_adam_groups_round_trip_through_a_list_of_torch_adams(tmp_path):
    model = fp.build_model(_cfg(16), fp.TRAIN_PHASE)
    groups = [(('hrnet',), 1e-5)]
    tr = _HostTrainer(model, lr=1e-3, lr_groups=groups)
    _fill(tr.opt.m, 2)
    _fill(tr.opt.v, 3)
    tr.opt.v.abs_()
    tr.optimizers[0].state.copy_(torch.tensor([4.0, 1e-3, 1 - 0.9 ** 4, 1 - 0.999 ** 4]))
    tr.optimizers[1].state.copy_(torch.tensor([4.0, 1e-5, 1 - 0.9 ** 4, 1 - 0.999 ** 4]))
    sds = ck.optimizer_state_dicts(tr)
    assert len(sds) == 2 and [len(s['param_groups'][0]['params']) for s in sds] == [106, 878]
    # the reference's list of two Adams (optimizer.py:47-53,69-72), built on the same parameters
    names = dict((id(p), n) for n, p in model.named_parameters())
    base = [p for p in model.parameters() if p.requires_grad and not names[id(p)].startswith('hrnet')]
    extra = [p for p in model.parameters() if p.requires_grad and names[id(p)].startswith('hrnet')]
    refs = [torch.optim.Adam(base, lr=1.0), torch.optim.Adam(extra, lr=1.0)]
    for o, s in zip(refs, sds):
        o.load_state_dict(s)
    assert refs[0].param_groups[0]['lr'] == pytest.approx(1e-3) and refs[1].param_groups[0]['lr'] == pytest.approx(1e-5)
    for o, ps in zip(refs, (base, extra)):
        for p in ps:
            st = o.state[p]
            off, n = next((off, n) for q, off, n in tr.table if q is p)
            assert torch.equal(st['exp_avg'], tr.opt.m[off:off + n].view(p.shape)) and float(st['step']) == 4.0
    # the reference's resume matches the dicts by parameter count: hand them over in the other order
    back = [refs[1].state_dict(), refs[0].state_dict()]
    tr2 = _HostTrainer(model, lr=1.0, lr_groups=groups)
    ck.load_optimizer_state_dicts(tr2, back)
    assert back == []
    assert torch.equal(tr2.opt.m, tr.opt.m) and torch.equal(tr2.opt.v, tr.opt.v)
    for a, b in zip(tr2.optimizers, tr.optimizers):
        assert torch.allclose(a.state, b.state) and a.lr == pytest.approx(b.lr)
    # save_checkpoint / resume carry the list
    path = ck.save_checkpoint(3, str(tmp_path), model, tr)
    assert len(torch.load(path)['optimizer']) == 2
    tr3 = _HostTrainer(model, lr=1.0, lr_groups=groups)
    _, _, begin = ck.resume(model, tr3, path)
    assert begin == 4 and torch.equal(tr3.opt.m, tr.opt.m) and torch.equal(tr3.opt.v, tr.opt.v)
    assert [o.lr for o in tr3.optimizers] == [pytest.approx(1e-3), pytest.approx(1e-5)]
    # a single-group checkpoint has no dict with either group's parameter count
    with pytest.raises(ValueError, match='parameters'):
        ck.load_optimizer_state_dicts(tr3, ck.optimizer_state_dicts(_HostTrainer(model, lr=1e-3)))


def test_cfg_node_defaults_are_the_reference_ones():
    """Missing TRAIN keys take the reference defaults (LR_SECOND_GROUP [None] = one group)."""
    cfg = CfgNode.wrap({'TRAIN': {}})
    assert optimizer_kwargs(cfg) == {'optimizer': 'adam', 'lr': 0.001, 'lr_groups': None}
    cfg = CfgNode.wrap({'TRAIN': {'LR_SECOND_GROUP': [None], 'OPTIMIZER': 'sgd'}})
    assert optimizer_kwargs(cfg)['momentum'] == 0.9
