"""The training step of the hot path, MI355X-first.

Restates engine/core/functions/alignment_mi_function_term6_1.py:104-156
(model call, JointMSELoss * W_mse, MI combination with alpha 0.5 / beta 0.1,
zero_grad / backward / Adam step) -- the reference loop itself is not importable
 -- with these design choices:

* parameters, gradients and both Adam moments live in four flat fp32 arenas
  (one allocation each); nn.Parameter objects are views, so state_dict() is
  unchanged.  Adam is ONE kernel over the arena; the data-parallel all-reduce
  needs no flatten/unflatten copies: a bucket is a slice of the gradient arena.
  TRAIN.OPTIMIZER 'sgd' is ONE fused SGD kernel the same way (FlatSGD).  A second
  learning-rate group (TRAIN.LR_SECOND_GROUP) keeps the one arena: each group
  updates its own contiguous arena runs with its own device state vector.
* one process per GPU; gradients are averaged with RCCL all-reduce over xGMI,
  bucket by bucket, each bucket launched as soon as the backward tape has
  enqueued the last contribution to it (reverse registration order: the head
  and stage 4 first), overlapping with the rest of backward.  BatchNorm
  statistics stay per replica (what the reference's nn.DataParallel does).
* the whole launch sequence of a step is captured once into hipGraphs and
  replayed (torch.cuda.CUDAGraph is used purely as the capture/replay handle).
  With world_size > 1 the backward is cut into one graph per bucket so the
  collectives run between graph launches on RCCL's stream.
"""
import contextlib

import torch
import torch.distributed as dist

from . import options
from ._lib import lib
from .engine import Engine, _p
from .head import SupervisionHead


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


class _FlatOptimizer:
    """What FlatAdam and FlatSGD share: the arena runs, the learning rate (host copy and the device scalar state[1]), the
    gradient multiplier, and a step as "the scalars, then one launch per run".  A subclass supplies `_prep(flag, s)` (the
    step's scalars; flag: the device u32 of the checked step, None: unchecked) and `_launch(lo, hi, s)`."""

    gmul = None

    def __init__(self, flat_param, lr, runs):
        self.p = flat_param
        self.runs = [(0, flat_param.numel())] if runs is None else [(int(a), int(b)) for a, b in runs]
        self.lr = float(lr)
        # the undecayed rate an LR schedule scales (torch stores it as param_groups[0]['initial_lr'] the first time a
        # scheduler is attached; checkpoints carry it so a resumed MultiStepLR does not decay an already decayed rate)
        self.initial_lr = float(lr)
        self.hyper_version = 0

    def set_grad_multiplier(self, t):
        """t: device float tensor [1] read by every later update (None: back to the unscaled update).  A graph-mode
        Trainer bakes the choice into its captured plan: it sets it once, at construction."""
        self.gmul = _check_gmul(t, self.p)

    def set_lr(self, lr):
        self.lr = float(lr)
        self.state[1] = self.lr

    def step(self, flag=None):
        """flag: device u32 raised by fami_unscale_check_f32 on non-finite gradients -> the step is skipped."""
        s = _stream(self.p.device)
        self._prep(flag, s)
        for lo, hi in self.runs:
            self._launch(lo, hi, s)

    def prep(self, s=None):
        """the step's scalars alone (step count, bias corrections): a step split into ranges prepares once, up front"""
        self._prep(None, _stream(self.p.device) if s is None else s)

    def apply(self, lo, hi, s=None):
        """the update of arena[lo:hi] (restricted to this optimizer's runs) with the prepared scalars"""
        s = _stream(self.p.device) if s is None else s
        for a, b in _clip(self.runs, lo, hi):
            self._launch(a, b, s)

    def _scaled(self, name):
        """-> (entry point, trailing arguments): `name`, or its _scaled variant with the multiplier pointer appended"""
        return (name + '_f32', ()) if self.gmul is None else (name + '_scaled_f32', (_p(self.gmul),))


class FlatAdam(_FlatOptimizer):
    """torch.optim.Adam(lr, betas=(0.9,0.999), eps=1e-8, weight_decay=0) on one flat fp32 arena
    (posetimation/optimizer/optimizer.py:66-68 builds the reference's).  The step count, the learning rate and the two
    bias corrections live in a device vector, so an LR schedule needs no re-capture of a hipGraph; betas / eps /
    weight decay are kernel arguments: changing them (set_hyper, or loading a checkpoint) bumps `hyper_version`,
    which makes a graph-mode Trainer re-capture.

    runs: the arena ranges [(lo, hi)] this optimizer updates (None: the whole arena) -- one learning-rate group of a
    Trainer (parameter_groups).  share: another group's optimizer whose gradient and moment arenas this one uses.
    gmul (set_grad_multiplier): a device float the gradient is multiplied by on load -- the clip coefficient of
    fami_clip_coef_f32; the gradient arena itself is not rewritten.  None: exactly the launches of the plain update."""

    kind = 'adam'

    def __init__(self, flat_param, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, runs=None, share=None):
        super().__init__(flat_param, lr, runs)
        if share is None:
            self.grad = torch.zeros_like(flat_param)
            self.m = torch.zeros_like(flat_param)
            self.v = torch.zeros_like(flat_param)
        else:
            self.grad, self.m, self.v = share.grad, share.m, share.v
        self.betas, self.eps, self.wd = tuple(betas), eps, weight_decay
        self.state = torch.tensor([0.0, lr, 1.0, 1.0], device=flat_param.device)   # step, lr, bc1, bc2

    def tensors(self):
        """the device state a step mutates besides the parameters (a graph capture's warm-up restores it)"""
        return [self.m, self.v, self.state]

    def set_hyper(self, betas=None, eps=None, weight_decay=None):
        new = (tuple(betas) if betas is not None else self.betas, self.eps if eps is None else eps,
               self.wd if weight_decay is None else weight_decay)
        if new != (self.betas, self.eps, self.wd):
            self.betas, self.eps, self.wd = new
            self.hyper_version += 1

    def _prep(self, flag, s):
        if flag is None:
            lib().call('fami_adam_prep_f32', _p(self.state), self.betas[0], self.betas[1], s)
        else:
            lib().call('fami_adam_prep_checked_f32', _p(self.state), self.betas[0], self.betas[1], _p(flag), s)

    def _launch(self, lo, hi, s):
        name, gmul = self._scaled('fami_adam')
        lib().call(name, _p(self.p[lo:hi]), _p(self.grad[lo:hi]), _p(self.m[lo:hi]), _p(self.v[lo:hi]), hi - lo,
                   _p(self.state), self.betas[0], self.betas[1], self.eps, self.wd, *gmul, s)


class FlatSGD(_FlatOptimizer):
    """torch.optim.SGD(lr, momentum, dampening, weight_decay, nesterov) on one flat fp32 arena: TRAIN.OPTIMIZER 'sgd'
    (posetimation/optimizer/optimizer.py:58-64; MOMENTUM 0.9 / WD 1e-4 / NESTEROV False in posetimation/config/
    defaults.py:137-140).  The protocol of FlatAdam: the step count (it selects the momentum buffer's first-step rule),
    the learning rate and the skip decision of the checked step live in a device vector; momentum / dampening / weight
    decay / nesterov are kernel arguments (set_hyper bumps `hyper_version`).  The momentum buffer exists only with a
    momentum, as torch's does.  gmul / set_grad_multiplier: as FlatAdam's."""

    kind = 'sgd'

    def __init__(self, flat_param, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, runs=None,
                 share=None):
        _check_sgd(lr, momentum, dampening, weight_decay, nesterov)
        super().__init__(flat_param, lr, runs)
        self.grad = torch.zeros_like(flat_param) if share is None else share.grad
        self.momentum, self.dampening, self.wd, self.nesterov = float(momentum), float(dampening), float(weight_decay), bool(nesterov)
        self.buf = None
        if self.momentum != 0.0:
            self.buf = share.buf if share is not None and share.buf is not None else torch.zeros_like(flat_param)
        self.state = torch.tensor([0.0, lr, 1.0], device=flat_param.device)        # step, lr, apply

    def tensors(self):
        return ([] if self.buf is None else [self.buf]) + [self.state]

    def set_hyper(self, momentum=None, dampening=None, weight_decay=None, nesterov=None):
        new = (self.momentum if momentum is None else float(momentum), self.dampening if dampening is None else float(dampening),
               self.wd if weight_decay is None else float(weight_decay), self.nesterov if nesterov is None else bool(nesterov))
        if new != (self.momentum, self.dampening, self.wd, self.nesterov):
            _check_sgd(self.lr, *new)
            self.momentum, self.dampening, self.wd, self.nesterov = new
            if self.momentum != 0.0 and self.buf is None:
                self.buf = torch.zeros_like(self.p)
            self.hyper_version += 1

    def _prep(self, flag, s):
        if flag is None:
            lib().call('fami_sgd_prep_f32', _p(self.state), s)
        else:
            lib().call('fami_sgd_prep_checked_f32', _p(self.state), _p(flag), s)

    def _launch(self, lo, hi, s):
        name, gmul = self._scaled('fami_sgd')
        lib().call(name, _p(self.p[lo:hi]), _p(self.grad[lo:hi]), None if self.momentum == 0.0 else _p(self.buf[lo:hi]),
                   hi - lo, _p(self.state), self.momentum, self.dampening, self.wd, int(self.nesterov), *gmul, s)


def _check_gmul(t, like):
    if t is not None and not (torch.is_tensor(t) and t.dtype == torch.float32 and t.numel() == 1 and t.device == like.device):
        raise ValueError('the gradient multiplier is one fp32 element on the device of the parameters')
    return t


def _check_ema_decay(v):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 < float(v) < 1.0:
        raise ValueError('ema_decay is None or a number in (0, 1), not %r' % (v,))
    return float(v)


def _check_sgd(lr, momentum, dampening, weight_decay, nesterov):
    """torch.optim.SGD.__init__'s argument checks"""
    if lr < 0.0:
        raise ValueError('Invalid learning rate: {}'.format(lr))
    if momentum < 0.0:
        raise ValueError('Invalid momentum value: {}'.format(momentum))
    if weight_decay < 0.0:
        raise ValueError('Invalid weight_decay value: {}'.format(weight_decay))
    if nesterov and (momentum <= 0 or dampening != 0):
        raise ValueError('Nesterov momentum requires a momentum and zero dampening')


def _clip(runs, lo, hi):
    """the non-empty pieces of [lo, hi) inside the runs"""
    out = []
    for a, b in runs:
        a, b = max(a, lo), min(b, hi)
        if b > a:
            out.append((a, b))
    return out


class MultiStepLR:
    """torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones, gamma, last_epoch) for the flat Adam: what
    posetimation/optimizer/scheduler.py:14-35 builds from TRAIN.LR_STEP / TRAIN.LR_FACTOR ([8, 12, 16] x 0.1 in
    configs/Alignment/Base_PoseTrack17.yaml) and engine/defaults/trainer.py steps once per epoch.  `opt` is a FlatAdam /
    FlatSGD (one learning-rate group: an entry of Trainer.optimizers) or a Trainer (its base group); the new rate is
    written into the optimizer's device-resident state, so captured graphs keep replaying."""

    def __init__(self, opt, milestones, gamma=0.1, last_epoch=-1, base_lr=None):
        import bisect
        self._bisect = bisect.bisect_right
        self.opt = opt.opt if hasattr(opt, 'opt') else opt
        self.milestones = sorted(int(m) for m in milestones)
        self.gamma = float(gamma)
        # torch's rule (lr_scheduler.LRScheduler.__init__): a fresh schedule (last_epoch == -1) adopts the optimizer's
        # current rate as `initial_lr`; a resumed one REQUIRES the stored `initial_lr` -- never the current, already
        # decayed `lr` (resuming at epoch 10 gave 1e-5 instead of 1e-4)
        if base_lr is not None:
            self.base_lr = float(base_lr)
        elif int(last_epoch) == -1:
            self.base_lr = float(self.opt.lr)
        else:
            self.base_lr = float(getattr(self.opt, 'initial_lr', self.opt.lr))
        self.opt.initial_lr = self.base_lr
        self.last_epoch = int(last_epoch)
        self.step()          # like torch: construction performs the step to epoch last_epoch + 1

    def get_last_lr(self):
        return [self.base_lr * self.gamma ** self._bisect(self.milestones, self.last_epoch)]

    def step(self):
        self.last_epoch += 1
        self.opt.set_lr(self.get_last_lr()[0])

    def state_dict(self):
        return {'milestones': list(self.milestones), 'gamma': self.gamma, 'base_lr': self.base_lr,
                'last_epoch': self.last_epoch}

    def load_state_dict(self, sd):
        self.milestones, self.gamma = sorted(sd['milestones']), float(sd['gamma'])
        self.base_lr, self.last_epoch = float(sd['base_lr']), int(sd['last_epoch'])
        self.opt.set_lr(self.get_last_lr()[0])


def frozen_batchnorm_names(model):
    """Names (named_modules() order) of the BatchNorm2d modules whose statistics are frozen (freeze_batchnorm)."""
    return [n for n, m in model.named_modules()
            if isinstance(m, torch.nn.BatchNorm2d) and getattr(m, 'frozen_stats', False)]


def freeze_batchnorm(model, scope):
    """Freeze the statistics of BatchNorm2d modules of `model` (`norm_eval` / FrozenBatchNorm of other toolboxes): a frozen
    BatchNorm normalises with its running statistics in train mode too, leaves them and num_batches_tracked untouched,
    still propagates gradients and still trains gamma / beta (set requires_grad = False on those to fix them as well).
    scope: 'all'; 'backbone' (module names under `hrnet.`); a tuple of module-name prefixes (or one prefix that is
    neither word); None clears the flag everywhere.  The modules in scope get `frozen_stats = True`, every other
    BatchNorm2d loses the flag: the call states the whole set.  -> the frozen names in named_modules() order.  A
    prefix that matches no BatchNorm2d raises ValueError (nothing is changed then).  The flag is a plain attribute:
    model.train() / model.eval() do not touch it and state_dict() does not carry it.  The reference has no such switch:
    its MODEL.FREEZE_HRNET_WEIGHTS stops the weights and lets the statistics follow every batch."""
    bns = [(n, m) for n, m in model.named_modules() if isinstance(m, torch.nn.BatchNorm2d)]
    if scope is None:
        prefixes = ()
    elif scope == 'all':
        prefixes = ('',)
    elif scope == 'backbone':
        prefixes = ('hrnet.',)
    elif isinstance(scope, str):
        prefixes = (scope,)
    else:
        prefixes = tuple(scope)
        if not prefixes or not all(isinstance(q, str) for q in prefixes):
            raise ValueError("scope is None, 'all', 'backbone' or a tuple of module-name prefixes, not %r" % (scope,))
    for q in prefixes:
        if not any(n.startswith(q) for n, _ in bns):
            raise ValueError('no BatchNorm2d module name starts with %r' % (q,))
    names = []
    for n, m in bns:
        if any(n.startswith(q) for q in prefixes):
            m.frozen_stats = True
            names.append(n)
        elif 'frozen_stats' in m.__dict__:
            del m.frozen_stats
    return names


def flatten_parameters(model):
    """Move every trainable parameter into one flat arena (views keep names/shapes). -> (flat, [(param, off, n)])"""
    ps = [p for p in model.parameters() if p.requires_grad]
    # groups the model wants adjacent (engine.CatParam: the two predictor convolutions of a DCN layer run as one): the later
    # members move directly behind the first one
    groups = [g for g in (model.adjacent_parameters() if hasattr(model, 'adjacent_parameters') else [])
              if all(q.requires_grad for q in g)]
    follow = {id(g[0]): g[1:] for g in groups}
    moved = {id(q) for g in groups for q in g[1:]}
    ordered = []
    for p in ps:
        if id(p) in moved:
            continue
        ordered.append(p)
        ordered.extend(follow.get(id(p), ()))
    total = sum(p.numel() for p in ps)
    flat = torch.empty(total, dtype=torch.float32, device=ps[0].device)
    where, off = {}, 0
    for p in ordered:                      # the arena's layout
        n = p.numel()
        flat[off:off + n].copy_(p.data.reshape(-1))
        p.data = flat[off:off + n].view(p.shape)
        if hasattr(p, '_fami_packed'):          # a packed image cached while the parameter was frozen is stale now
            del p._fami_packed
        where[id(p)] = off
        off += n
    # the table stays in model.parameters() order: torch.optim.Adam numbers its state that way (checkpoint.py)
    return flat, [(p, where[id(p)], p.numel()) for p in ps]


def parameter_groups(model, lr_groups=None):
    """-> [[(name, param)], ...]: the base learning-rate group, then one group per `lr_groups` entry (name_prefixes, lr):
    the trainable parameters whose names start with one of its prefixes (the first matching entry wins).  That is
    posetimation/optimizer/optimizer.py:18-55 for TRAIN.LR_SECOND_GROUP: `name.startswith` over model.named_parameters(),
    frozen parameters in no group, each group in model.parameters() order."""
    lr_groups = list(lr_groups or ())
    prefixes = [(p,) if isinstance(p, str) else tuple(p) for p, _ in lr_groups]
    groups = [[] for _ in range(1 + len(lr_groups))]
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        k = next((j + 1 for j, pre in enumerate(prefixes) if name.startswith(pre)), 0)
        groups[k].append((name, p))
    return groups


def _runs(spans):
    """[(off, n)] -> the sorted, merged arena ranges [(lo, hi)] they cover"""
    out = []
    for off, n in sorted(spans):
        if out and out[-1][1] == off:
            out[-1] = (out[-1][0], off + n)
        else:
            out.append((off, off + n))
    return out


def build_optimizers(model, flat, table, optimizer='adam', lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0,
                     nesterov=False, lr_groups=None):
    """The flat optimizer(s) of a Trainer -> (optimizers, rows): one FlatAdam / FlatSGD per learning-rate group
    (parameter_groups), the base group first; rows[k] = the indices into `table` of group k's parameters.  Without
    lr_groups: ONE optimizer over the whole arena, exactly the launches of a plain FlatAdam / FlatSGD.  With them, every
    group updates only its own arena runs, keeps its own device state vector (rate, step count) and shares the
    gradient and moment arenas of the base group."""
    if optimizer == 'adam':
        if momentum or dampening or nesterov:
            raise ValueError('momentum / dampening / nesterov are arguments of the sgd optimizer, not of adam')

        def make(rate, runs, share):
            return FlatAdam(flat, lr=rate, weight_decay=weight_decay, runs=runs, share=share)
    elif optimizer == 'sgd':
        def make(rate, runs, share):
            return FlatSGD(flat, lr=rate, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                           nesterov=nesterov, runs=runs, share=share)
    else:
        raise ValueError("optimizer must be 'adam' or 'sgd', not %r" % (optimizer,))
    if not lr_groups:
        return [make(lr, None, None)], [list(range(len(table)))]
    index = {id(p): i for i, (p, _, _) in enumerate(table)}
    rates = [lr] + [float(r) for _, r in lr_groups]
    opts, rows = [], []
    for k, (members, rate) in enumerate(zip(parameter_groups(model, lr_groups), rates)):
        if not members:
            # (torch.optim raises on an empty parameter list too)
            raise ValueError('learning-rate group %d (%s) has no trainable parameter' %
                             (k, 'base' if k == 0 else lr_groups[k - 1][0]))
        idx = [index[id(p)] for _, p in members]
        opts.append(make(rate, _runs([table[i][1:] for i in idx]), opts[0] if opts else None))
        rows.append(idx)
    return opts, rows


def optimizer_kwargs(cfg):
    """The Trainer's optimizer arguments from a reference config: posetimation/optimizer/optimizer.py:16-76 reads
    TRAIN.OPTIMIZER / LR / MOMENTUM / WD / NESTEROV / LR_SECOND_GROUP / LR_SECOND_GROUP_VALUE (defaults
    posetimation/config/defaults.py:137-140 and mppe_config.py:306-307).  Its Adam is built from `lr` alone
    (optimizer.py:68,72), so TRAIN.WD reaches SGD only."""
    t = cfg['TRAIN']
    kind = t.get('OPTIMIZER', 'adam')
    lr = float(t.get('LR', 0.001))
    second = list(t.get('LR_SECOND_GROUP', None) or [None])
    groups = None if second[0] is None else [(tuple(second), float(t.get('LR_SECOND_GROUP_VALUE', 1e-6)))]
    if kind == 'sgd':
        if groups:
            raise ValueError("TRAIN.OPTIMIZER 'sgd' with TRAIN.LR_SECOND_GROUP cannot be built: the reference hands "
                             "torch.optim.SGD a list of parameter-group lists (optimizer.py:50-53,58-59), which torch "
                             "rejects with a TypeError")
        return {'optimizer': 'sgd', 'lr': lr, 'momentum': float(t.get('MOMENTUM', 0.9)),
                'weight_decay': float(t.get('WD', 1e-4)), 'nesterov': bool(t.get('NESTEROV', False))}
    if kind == 'adam':
        return {'optimizer': 'adam', 'lr': lr, 'lr_groups': groups}
    raise ValueError("TRAIN.OPTIMIZER must be 'adam' or 'sgd', not %r" % (kind,))


def build_lr_scheduler(cfg, trainer, last_epoch=-1):
    """posetimation/optimizer/scheduler.py:14-27: TRAIN.LR_SCHEDULER 'MultiStepLR' over TRAIN.LR_STEP / LR_FACTOR -- one
    MultiStepLR for one learning-rate group, a list of them (one per group, each decaying its own rate) otherwise."""
    t = cfg['TRAIN']
    if t.get('LR_SCHEDULER', 'MultiStepLR') != 'MultiStepLR':
        raise ValueError('TRAIN.LR_SCHEDULER must be MultiStepLR, not %r' % (t.get('LR_SCHEDULER'),))
    steps, factor = t.get('LR_STEP', [90, 110]), float(t.get('LR_FACTOR', 0.1))
    opts = getattr(trainer, 'optimizers', None) or [trainer]
    out = [MultiStepLR(o, steps, factor, last_epoch=last_epoch) for o in opts]
    return out[0] if len(out) == 1 else out


class WeightPacker:
    """MFMA-fragment images of every trainable nn.Conv2d weight (forward and dgrad orientation), rebuilt from the
    flat fp32 parameter arena in ONE launch per step (fami_pack_conv_weights_batch_*) instead of ~600."""

    def __init__(self, model, flat, table, dtype, cats=None, route=None):
        """route: the Trainer's kernel-routing state (None: the process default) -- the size queries and the pack launches run
        under the route the model's engines dispatch by (today no route field changes an image's geometry; the DCN backward
        image already did once)."""
        import numpy as np
        self.route = route
        lib().bind(route)
        L = lib().cdll
        from .engine import _SFX
        bf = dtype != torch.float32      # 16-bit images (bf16 | fp16) share one geometry
        elems = L.fami_packed_weight_elems_bf16 if bf else L.fami_packed_weight_elems
        convs = {id(m.weight) for m in model.modules() if isinstance(m, torch.nn.Conv2d)}
        recs, self.views, off = [], {}, 0
        spans = []
        # merged convolutions (engine.CatParam over adjacent weights): ONE image of the concatenated weight, keyed by the
        # CatParam; the parts get no image of their own
        cats = {id(c.parts[0]): c for c in (cats or ()) if len(c.shape) == 4}
        skip = {id(q) for c in cats.values() for q in c.parts[1:]}
        for prm, src, _ in table:
            if id(prm) not in convs or id(prm) in skip:
                continue
            if id(prm) in cats:
                prm = cats[id(prm)]
            Co, Ci, kh, kw = prm.shape
            for mode in (0, 1):
                n = elems(Co, Ci, kh, kw, mode)
                recs.append((src, off, Co, Ci, kh * kw, mode))
                spans.append((id(prm), mode, off, n))
                off += n
        # forward images first, input-gradient images behind them: the two halves can be packed by separate launches
        # (run(stream, 0) before the forward pass, run(side_stream, 1) beside it -- nothing reads a mode-1 image before
        # the backward pass)
        recs.sort(key=lambda r: r[5])
        self.n = len(recs)
        self.n_fwd = sum(1 for r in recs if r[5] == 0)
        # ... and the forward images in two: what the stem, layer1 and stage 2 read (packed on the main lane before the first
        # convolution) and the rest (stage 3 / 4 and the head: ~95 % of the bytes), packed on a side lane beside the stem --
        # the whole forward pack sat alone at the top of every step (0.36-0.42 ms + the f32 split images)
        names = {id(p): n for n, p in model.named_parameters()}
        early = ('hrnet.conv1.', 'hrnet.conv2.', 'hrnet.layer1.', 'hrnet.transition1.', 'hrnet.stage2.', 'conv1.', 'conv2.',
                 'layer1.', 'transition1.', 'stage2.')
        order = [prm for prm, _, _ in table if id(prm) in convs and id(prm) not in skip]
        self.n_early = 0
        for prm in order:
            if names.get(id(prm), '').startswith(early):
                self.n_early += 1
            else:
                break
        self.flat = flat
        self.arena = torch.empty(max(off, 1), dtype=dtype, device=flat.device)
        desc = np.array(recs, dtype=[('src', '<i8'), ('dst', '<i8'), ('Co', '<i4'), ('Ci', '<i4'), ('taps', '<i4'),
                                     ('mode', '<i4')])
        self.desc = torch.from_numpy(desc.view(np.uint8).copy()).to(flat.device)
        for pid, mode, o, n in spans:
            self.views[(pid, mode)] = self.arena[o:o + n]
        self.fn = 'fami_pack_conv_weights_batch' + _SFX[dtype]

    def run(self, stream, part=None):
        """part None: every image; 0: the forward images; 1: the input-gradient images; 'early' / 'late': the forward images of
        the stem .. stage 2 / of everything behind them."""
        lo, hi = {None: (0, self.n), 0: (0, self.n_fwd), 1: (self.n_fwd, self.n), 'early': (0, self.n_early),
                  'late': (self.n_early, self.n_fwd)}[part]
        if hi > lo:
            lib().call_routed(self.route, self.fn, _p(self.flat), _p(self.arena), self.desc.data_ptr() + 32 * lo, hi - lo, stream)


class BucketReducer:
    """Data-parallel gradient exchange over one flat gradient arena (pure host logic + torch.distributed;
    no HIP dependency, so the N>1 path is covered by gloo tests on CPU).

    The arena is cut into fixed-size slices from the TAIL (parameters register head-last, so backward
    completes the tail first).  `hook(done_params)` is what Engine.backward calls when a parameter's last
    gradient contribution has been enqueued; once every parameter overlapping a slice is complete the slice
    is handed to `on_bucket(lo, hi)` (an async all-reduce, or a graph cut during capture)."""

    def __init__(self, grad, table, bucket_elems, process_group=None, payload=None, cast=None, widen=None, algo=None):
        """payload: None (the fp32 slices themselves are reduced in place) or a 16-bit torch dtype: a slice is cast into a
        16-bit mirror of the arena, the mirror slice is all-reduced (half the bytes over xGMI: 129 MB instead of 258.6 MB
        per step for W48) and widened back into the fp32 arena in wait().  cast(src_f32, dst_16) / widen(src_16, dst_f32):
        the device kernels of the caller (Trainer: fami_cast_add_* / fami_widen_*); default = torch copies (CPU tests).
        algo (default FAMI_DDP_ALGO or 'ring'): 'ring' = one all_reduce per slice (the library picks its algorithm; a ring
        over xGMI is bound by ONE 153 GB/s link: ~3 ms for 258 MB); 'mesh' = the slice as reduce_scatter_tensor ->
        all_gather_into_tensor, i.e. every rank owns 1/world of the slice, receives the other ranks' copies of it over
        its 7 point-to-point links at once, sums, and sends the sum back the same way (~0.4 ms for 258 MB on
        the full xGMI mesh).  The remainder of a slice that is not a multiple of `world` (< world elements, at most one
        slice per step) goes through a plain all_reduce.  Replaces engine/defaults/trainer.py:57-58 (nn.DataParallel)."""
        self.payload = payload
        self._cast = cast or (lambda src, dst: dst.copy_(src))
        self._widen = widen or (lambda src, dst: dst.copy_(src))
        self._mirror = None
        self.grad = grad
        self.offset = {id(p): (o, n) for p, o, n in table}
        self.total = grad.numel()
        self.bucket_elems = max(1, int(bucket_elems))
        self.pg = process_group
        self.world = dist.get_world_size(process_group) if dist.is_initialized() else 1
        self.algo = (algo or options.get('FAMI_DDP_ALGO')).lower()
        if self.algo not in ('ring', 'mesh'):
            raise ValueError("FAMI_DDP_ALGO must be 'ring' or 'mesh', not %r" % self.algo)
        self._shards = {}        # (lo, hi) -> this rank's 1/world of the slice (mesh plan; persistent: graph-plan replays reuse it)
        # gloo runs queued collectives on a worker pool: the all-gather of a slice must not start before its
        # reduce-scatter has finished, so the handle is waited for in between.  RCCL orders both on its own stream.
        self._ordered = dist.is_initialized() and dist.get_backend(process_group) == 'nccl'
        self.works = []

    def ranges(self):
        out, hi = [], self.total
        while hi > 0:
            lo = max(0, hi - self.bucket_elems)
            out.append((lo, hi))
            hi = lo
        return out

    def begin(self, on_bucket=None):
        """-> hook for Engine.backward(on_params_done=...)."""
        self._on_bucket = on_bucket or self.allreduce
        self._ranges = self.ranges()
        self._next, self._done_lo, self._pending = 0, self.total, {}
        self.works = []
        return self._hook

    def _hook(self, done_params):
        for p in done_params:
            o, n = self.offset[id(p)]
            self._pending[o] = n
        while self._done_lo in _ends(self._pending):        # advance the contiguous frontier from the tail
            o = _ends(self._pending)[self._done_lo]
            self._done_lo = o
            del self._pending[o]
        while self._next < len(self._ranges) and self._ranges[self._next][0] >= self._done_lo:
            self._on_bucket(*self._ranges[self._next])
            self._next += 1

    def flush(self):
        """Slices whose parameters never receive a gradient (hrnet.final_layer feeds only detached MI terms)."""
        while self._next < len(self._ranges):
            self._on_bucket(*self._ranges[self._next])
            self._next += 1

    def _exchange(self, buf, key):
        """Sum `buf` (a slice of the arena or of its 16-bit mirror) over the ranks, asynchronously -> last work handle."""
        if self.algo == 'ring' or self.world == 1:
            return dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=self.pg, async_op=True)
        n = buf.numel()
        main = n - n % self.world
        wk = None
        if main:
            shard = self._shards.get(key)
            if shard is None or shard.numel() != main // self.world or shard.dtype != buf.dtype:
                shard = self._shards[key] = torch.empty(main // self.world, dtype=buf.dtype, device=buf.device)
            wk = dist.reduce_scatter_tensor(shard, buf[:main], op=dist.ReduceOp.SUM, group=self.pg, async_op=True)
            if self._ordered:
                wk = dist.all_gather_into_tensor(buf[:main], shard, group=self.pg, async_op=True)
            else:
                # (gloo: the gather must follow the scatter's completion -- chained in wait(), not here: the backward hook that
                #  issues the exchange must not block the host enqueue of the rest of the backward pass)
                wk = _Chained(wk, lambda b=buf[:main], sh=shard: dist.all_gather_into_tensor(b, sh, group=self.pg))
        if main < n:
            if wk is not None:
                self.works.append((wk, None))
            wk = dist.all_reduce(buf[main:], op=dist.ReduceOp.SUM, group=self.pg, async_op=True)
        return wk

    def allreduce(self, lo, hi):
        if self.payload is None:
            wk = self._exchange(self.grad[lo:hi], (lo, hi))
            self.works.append((wk, None))
            return wk
        if self._mirror is None:
            self._mirror = torch.empty(self.total, dtype=self.payload, device=self.grad.device)
        buf = self._mirror[lo:hi]
        self._cast(self.grad[lo:hi], buf)
        wk = self._exchange(buf, (lo, hi))
        self.works.append((wk, (lo, hi)))
        return wk

    def wait(self):
        for wk, rng in self.works:
            wk.wait()
            if rng is not None:
                self._widen(self._mirror[rng[0]:rng[1]], self.grad[rng[0]:rng[1]])
        self.works = []


class _Chained:
    """A work handle followed by a blocking step that may only start once it has completed."""

    def __init__(self, work, then):
        self.work, self.then = work, then

    def wait(self):
        self.work.wait()
        self.then()


def _ends(pending):
    return {o + n: o for o, n in pending.items()}


class Trainer:
    """One optimisation step per call: forward, loss, backward, (all-reduce), Adam, PCK of both heatmap outputs -- all
    HIP kernels, no host synchronisation (core fn :104-174).

    loss_scale: gradients of the 16-bit activation modes are seeded with `loss_scale * dLoss` and the flat fp32
    gradient arena is divided by it before Adam (static scaling; fp16's smallest normal is 6e-5 while the MSE seed is
    ~2e-6 * error).  Default: 8192 for fp16, 1 otherwise (bf16 has fp32's exponent range).
    loss_scale='dynamic': torch.amp.GradScaler's rule on the device -- the scale lives in a device vector
    {scale, 1 / scale, growth tracker}, halves (backoff_factor) on a step whose gradients hold inf / NaN (that step is
    skipped and counted) and doubles (growth_factor) after growth_interval clean steps; `scaler` overrides GradScaler's
    defaults (init_scale, growth_factor, backoff_factor, growth_interval).  The seeds read the scale and the unscale
    pass its reciprocal from that vector, so a captured plan keeps replaying while the scale moves.

    max_grad_norm: torch.nn.utils.clip_grad_norm_(parameters, max_grad_norm) between backward and the optimizer, on the
    device: the 2-norm of the whole flat gradient arena (every trainable parameter once) after the data-parallel mean
    and the loss unscale, reduced by a partial-slab kernel (fused into the unscale pass where one runs), then
    coef = min(1, max / (norm + 1e-6)), which every learning-rate group's update kernel multiplies the gradients by on
    load -- the arena is not rewritten.  A non-finite norm skips (and counts) the step; torch would let it through.
    The threshold is a device scalar (set_max_grad_norm): no re-capture.  The total norm has to exist before the first
    update, so the in-backward optimizer split (_find_adam_split) is off while clipping -- or a dynamic scale -- is on,
    as it is for the checked fp16 step.

    accum_steps = N > 1: gradient accumulation.  step() is called once per micro-batch and runs forward, loss, PCK and
    backward exactly as without it (BatchNorm batch statistics, running statistics and batch counters are per micro-batch,
    the seeds are unchanged); N calls make one window and one update.  A second fp32 arena holds the running sum: a call
    at window position k < N - 1 only copies (k = 0) or adds (fami_axpby_f32, alpha = beta = 1) the gradient arena into
    it -- no unscale, no norm, no scale update, no optimizer, no all-reduce.  The call at position N - 1 closes the
    window with ONE pass over both arenas, grad = (accum + grad) * 1 / (N * loss_scale)
    (fami_accum_unscale_check_sumsq_f32: also the inf / NaN check and the sum of squares where the trainer is guarded /
    clips), then the clip coefficient, the scale update and the optimizers as above: `grad` then holds the window's mean
    gradient before clipping, a non-finite value in any micro-batch skips (and counts) the window once, and a dynamic
    scale moves once per window.  Graph mode replays the one captured forward + backward graph of the batch shape at
    every window position and one shape-independent captured tail at the last; the accumulating launches are enqueued
    behind the replay, so a window position never captures.  Data parallel: micro-batches before the last run without
    communication and without bucket hooks; at the last one grad = accum + grad, then the bucketed all-reduce of the
    arena, then the unscale pass with 1 / N folded into its factor, then the optimizers -- for all three plans (overlap,
    serial, eager hooks): the exchange already happens once per N backward passes, and its overlap with the last
    backward pass is deliberately not kept.  The in-backward optimizer split is off.  None and 1: no arena, the launch
    sequence above launch for launch.  Windows always hold N micro-batches and may span epochs (reset_window() drops an
    open one); set_lr / set_max_grad_norm inside a window act at its update.

    ema_decay = d in (0, 1): an exponential moving average of the weights, ema = ema + (1 - d_t) * (param - ema), kept on the
    device in a second fp32 arena `ema` with the parameter arena's layout (it starts as a copy of it, taken after the
    data-parallel broadcast).  Two launches directly behind the optimizers, wherever a step ends -- so inside every
    captured graph that holds them, and once per window under accumulation: fami_ema_prep_f32 advances
    `ema_state` = {updates, d_t, 1 - d_t, apply} and fami_ema_update_f32 makes one pass over both arenas.  The prep reads
    the base group's "this step was applied" scalar (opt.state[2]; that group is stepped last and records a skip), so a
    step skipped for an fp16 overflow or a non-finite norm leaves the average and its update count as they were, with no
    host read-back.  ema_warmup=True: d_t = min(d, (1 + t) / (10 + t)) at update t, so a short run is not dominated by its
    initial weights.  d and the warm-up switch are kernel arguments: set_ema_decay re-captures.  Data-parallel ranks
    exchange nothing for the average: equal parameters give equal averages.  BatchNorm running statistics and batch
    counters are NOT averaged -- they are running averages already -- so the averaged weights are used with the live
    buffers.  ema_weights() puts the average into the model (and takes it out again) by exchanging the two arenas in
    place; ema_state_dict() is the checkpoint entry.  None (default): no arena, none of these launches.

    frozen_bn = 'all' | 'backbone' | prefixes: BatchNorm with frozen statistics (freeze_batchnorm) -- those modules normalise
    with their running statistics (the eval-mode forward: fami_bn_eval_stats_f32 + fami_bn_apply_*), leave them and their
    batch counters untouched and run the one-pass backward fami_bn_eval_bwd_*; gamma / beta keep training unless the caller
    set requires_grad = False on them.  No train-only BatchNorm fusion is taken for a frozen module.  The set of frozen
    modules keys the captured plans next to the optimizer hyper-parameters: a later freeze_batchnorm call re-captures.
    The reference has no such switch, so there is no config key; None (default) leaves every launch as it is.

    The supervision (targets, loss terms and seeds between the forward and the backward pass) lives in one object, `head`
    (head.SupervisionHead: its docstring lists each option's launches, their order and the per-shape buffers).  Its options are
    fixed at construction like mse_weight and baked into the captured plans; the defaults leave the launch sequence as it is.
    joint_weights (needs targets_from_joints): J factors of the target weights, the reference's
    LOSS.USE_DIFFERENT_JOINTS_WEIGHT (heatmaps_process.py:200-201; from_cfg reads the key and passes data.JOINTS_WEIGHT).
    target_encoding='subpixel' (needs targets_from_joints): Gaussians centred at the real-valued joint position, the
    encoding the DARK decode assumes (loss.generate_heatmaps).  The PCK rows take the argmax of the target map: for a joint at
    exactly half a pixel the sub-pixel map's first maximum is the lower pixel where the quantised one has the upper.
    ohkm_topk = k (either kind of target): online hard keypoint mining, loss.JointOHKMMSELoss -- the J row losses of each
    sample are ranked on the device; loss_parts[0] = mse_weight * (1/B) sum_b (1/k) sum_{top-k} mean_p (w (pred - gt))^2, and
    the seeds carry mse_weight / (B L k) on the selected weights.  k = J is the default loss.  PCK and the MI terms are
    untouched.  ohkm_selection() is the last step's selection.

    integral_l1_weight = W_I (needs targets_from_joints; None = none): the integral L1 coordinate term, loss.IntegralL1Loss
    (definition: include/fami.h) -- W_I / (B J) sum_bj w_bj (|cx - tx| / W + |cy - ty| / H) with (cx, cy) the soft-argmax of the
    final map at integral_beta and (tx, ty) = joint / stride.  Its seed accumulates into the heat-map seed's buffer under the
    same loss scale.  It reads the target weights, also where OHKM selects.  loss_parts keeps its 7 entries: the term lives in
    its own device scalar (integral_loss_value(); loss_value() and window_loss_value() include it; under accumulation its
    window sum is a tensor of its own and accum_state_dict() gains a key for it).  integral_coords(): the last step's
    coordinates.  LOSS.INTEGRAL_L1.USE / .WEIGHT in from_cfg.

    structure_cos_weight = W_S (needs targets_from_joints; None = none): the structure term, loss.StructureCosineSimilarity
    (definition: include/fami.h) -- W_S / (B P) sum_bp valid_bp (1 - cos) between the predicted limb (the soft-argmax of the
    final map at integral_beta) and the target limb (joint / stride), over the P limbs of structure_pairs (None:
    data.LIMB_PAIRS); a limb is valid when both its joints have a target weight > 0 and its target is longer than
    structure_min_len heatmap pixels (1.0: a starting value, not tuned on data).  The soft-argmax and the target positions are
    computed once and shared when integral_l1_weight is set as well; its seeds go into the same buffer under the same loss
    scale.  It reads the target weights, also where OHKM selects.  Its device scalar, window sum and checkpoint key are the
    integral term's arrangement: structure_loss_value(); loss_value() and window_loss_value() include it.
    structure_cosines(): the last step's cosines [B,P].  LOSS.STRUCTURE_COSINE.USE / .WEIGHT in from_cfg.
    """

    def __init__(self, model, lr=1e-3, mse_weight=1.0, alpha=0.5, beta=0.1, use_mi=True, bucket_mb=32,
                 process_group=None, use_graph=True, targets_from_joints=False, sigma=3, force_ddp=False,
                 loss_scale=None, pck=True, data_parallel=None, optimizer='adam', momentum=0.0, dampening=0.0,
                 weight_decay=0.0, nesterov=False, lr_groups=None, max_grad_norm=None, scaler=None, accum_steps=None,
                 ema_decay=None, ema_warmup=False, frozen_bn=None, target_encoding='quantised', joint_weights=None,
                 ohkm_topk=None, integral_l1_weight=None, integral_beta=20.0, structure_cos_weight=None, structure_pairs=None,
                 structure_min_len=1.0):
        """optimizer 'adam' (torch.optim.Adam) or 'sgd' (torch.optim.SGD with momentum / dampening / nesterov);
        weight_decay applies to either.  lr_groups: [(name_prefixes, lr)] -- the parameters that leave the base group
        (rate `lr`) for a rate of their own (parameter_groups; TRAIN.LR_SECOND_GROUP).  Trainer.from_cfg reads all of it
        from a reference config.  max_grad_norm / loss_scale='dynamic' / scaler: see the class docstring (the reference
        configuration has no such keys: from_cfg takes them as keyword arguments).  accum_steps: micro-batches per update
        (class docstring; None = 1).  ema_decay / ema_warmup: the moving average of the weights (class docstring; None =
        none).  frozen_bn: None, 'all', 'backbone' or module-name prefixes -- freeze_batchnorm(model, frozen_bn) before
        anything is captured (class docstring; None leaves the model's flags as they are).  target_encoding / joint_weights
        / ohkm_topk: the options of the supervision (class docstring; no config key but joint_weights').
        integral_l1_weight / integral_beta: the integral L1 coordinate term (class docstring; LOSS.INTEGRAL_L1.USE / .WEIGHT;
        None = none).  structure_cos_weight / structure_pairs / structure_min_len: the structure term (class docstring;
        LOSS.STRUCTURE_COSINE.USE / .WEIGHT; None = none; its soft-argmax is the one at integral_beta)."""
        self.head = head = SupervisionHead(
            model, targets_from_joints, sigma, mse_weight, alpha, beta, use_mi, pck, target_encoding, joint_weights, ohkm_topk,
            integral_l1_weight, integral_beta, structure_cos_weight, structure_pairs, structure_min_len)
        self.integral_beta = None if head.integral_l1_weight is None else head.softargmax_beta
        if frozen_bn is not None:
            freeze_batchnorm(model, frozen_bn)
        self._bn_modules = [m for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d)]
        if ema_decay is None and ema_warmup:
            raise ValueError('ema_warmup=True needs an ema_decay')
        self.ema_decay = None if ema_decay is None else _check_ema_decay(ema_decay)
        self.ema_warmup = bool(ema_warmup)
        if accum_steps is not None and (isinstance(accum_steps, bool) or not isinstance(accum_steps, int) or accum_steps < 1):
            raise ValueError('accum_steps is None or an integer >= 1, not %r' % (accum_steps,))
        self.accum_steps = 1 if accum_steps is None else accum_steps
        self.model = model
        self.route = getattr(model, 'route', None)      # kernel-routing state (None: process default), as the model's engines
        self.dev = next(model.parameters()).device
        if self.dev.type != 'cuda':
            raise RuntimeError('Trainer needs the model on the GPU (HIP path only)')
        self.act_dtype = getattr(model, 'act_dtype', torch.float32)
        self.dynamic_scale = isinstance(loss_scale, str)
        if self.dynamic_scale and loss_scale != 'dynamic':
            raise ValueError("loss_scale is None, a number or 'dynamic', not %r" % (loss_scale,))
        if scaler is not None and not self.dynamic_scale:
            raise ValueError("`scaler` configures loss_scale='dynamic'")
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError('max_grad_norm must be positive, not %r' % (max_grad_norm,))
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.scaler_cfg = None
        if self.dynamic_scale:
            # torch.amp.GradScaler's names, defaults and argument checks
            cfg = {'init_scale': 65536.0, 'growth_factor': 2.0, 'backoff_factor': 0.5, 'growth_interval': 2000}
            unknown = set(scaler or ()) - set(cfg)
            if unknown:
                raise ValueError('unknown scaler argument(s): %s' % ', '.join(sorted(unknown)))
            cfg.update(scaler or {})
            if not (cfg['init_scale'] > 0.0 and cfg['growth_factor'] > 1.0 and 0.0 < cfg['backoff_factor'] < 1.0 and
                    int(cfg['growth_interval']) >= 1):
                raise ValueError('scaler needs init_scale > 0, growth_factor > 1, 0 < backoff_factor < 1 and '
                                 'growth_interval >= 1: %r' % (cfg,))
            self.scaler_cfg = cfg
            loss_scale = cfg['init_scale']
        # (with 'dynamic': the INITIAL scale; loss_scale_value() reads the current one)
        self.loss_scale = float(loss_scale if loss_scale is not None else
                                (8192.0 if self.act_dtype == torch.float16 else 1.0))
        self.flat, self.table = flatten_parameters(model)
        # overflow guard of the loss scale / of the gradient norm: a device flag raised by the unscale pass (inf / NaN
        # gradients) or by the clip coefficient (non-finite norm), consumed by the optimizer
        guarded = self.loss_scale != 1.0 or self.dynamic_scale or self.max_grad_norm is not None
        self.overflow = torch.zeros(2, dtype=torch.int32, device=self.dev) if guarded else None   # {raised, skipped steps}
        # device state of the two options: {scale, 1 / scale, growth tracker} and {total norm, coefficient, threshold} + the
        # partial sums of the norm
        self.scaler_state = (torch.tensor([self.loss_scale, 1.0 / self.loss_scale, 0.0], device=self.dev)
                       if self.dynamic_scale else None)
        self._scaler_version = 0
        self.clip = self._partials = None
        if self.max_grad_norm is not None:
            self.clip = torch.tensor([0.0, 1.0, self.max_grad_norm], device=self.dev)
            self._partials = torch.zeros(lib().cdll.fami_sumsq_parts(), device=self.dev)
        # one flat optimizer per learning-rate group; `opt` is the base group's (the only one without lr_groups)
        self.optimizers, self.group_rows = build_optimizers(
            model, self.flat, self.table, optimizer=optimizer, lr=lr, momentum=momentum, dampening=dampening,
            weight_decay=weight_decay, nesterov=nesterov, lr_groups=lr_groups)
        self.opt = self.optimizers[0]
        if self.clip is not None:
            for o in self.optimizers:          # every group multiplies its gradients by the ONE coefficient
                o.set_grad_multiplier(self.clip[1:2])
        # the checked step of several groups: each further group reads a copy of the overflow flag, the base group
        # (stepped last) reads, clears and counts the flag itself
        self._group_flags = (torch.zeros(len(self.optimizers) - 1, 2, dtype=torch.int32, device=self.dev)
                             if self.overflow is not None and len(self.optimizers) > 1 else None)
        self.grad = self.opt.grad
        # gradient accumulation: the running sum of the open window, {open window, last closed window} x the seven loss
        # parts summed over their calls, and the host-side position (micro-batches in the open window)
        self.accum = self._window_loss = None
        self.window_position = 0
        self._tail = None         # (graph of the window-closing tail, optimizer hyper version): one for every batch shape
        if self.accum_steps > 1:
            self.accum = torch.zeros_like(self.grad)
            self._window_loss = torch.zeros(2, 7, device=self.dev)
        self._adam_split = self._find_adam_split(model)
        self.views = {id(p): self.grad[o:o + n].view(p.shape) for p, o, n in self.table}
        # merged parameters (engine.CatParam): adjacent in the arena by construction -- one gradient view spanning the parts
        self.cats = []
        if hasattr(model, 'merged_predictors'):
            offs = {id(p): o for p, o, n in self.table}
            for pair in model.merged_predictors().values():
                for c in pair:
                    if c.adjacent() and c.requires_grad and id(c.parts[0]) in offs:
                        o = offs[id(c.parts[0])]
                        self.views[id(c)] = self.grad[o:o + c.numel()].view(c.shape)
                        self.cats.append(c)
        self.pg = process_group
        self.world = dist.get_world_size(process_group) if (process_group is not None or dist.is_initialized()) else 1
        if data_parallel is False:          # a single-process trainer inside an initialised process group (tests, tools)
            self.world = 1
        if self.world > 1 and process_group is None:
            self.pg = dist.group.WORLD
        # force_ddp: run the bucketed all-reduce path even with one rank (exercises the hooks / RCCL stream ordering
        # on a single GPU; an all-reduce over one rank is the identity)
        self.ddp = self.world > 1 or (force_ddp and dist.is_initialized())
        # FAMI_DDP_PAYLOAD = f32 (default) | bf16 | f16: gradient bytes on the wire (the sum over ranks is then taken in
        # that type; master gradients, the 1/world scale and Adam stay fp32).  The reference all-reduces fp32 gradients
        # (nn.DataParallel, trainer.py:57-58) and so does the default here in every compute mode: a 16-bit wire format
        # halves the bytes (129 MB instead of 258.6 MB per step for W48) but sums over ranks with 8 / 11 significand bits,
        # and no multi-GPU convergence run has validated that yet -- opt in with FAMI_DDP_PAYLOAD.
        self.payload_name = options.get('FAMI_DDP_PAYLOAD')
        pay = {'f32': None, 'bf16': torch.bfloat16, 'f16': torch.float16}[self.payload_name]
        if pay == torch.float16 and self.overflow is None:
            # without the loss-scale guard an fp16 sum that overflows on the wire would reach Adam as inf
            raise ValueError('FAMI_DDP_PAYLOAD=f16 needs the overflow guard of a loss-scaled (fp16) model; use bf16')
        sfx = {torch.bfloat16: 'bf16', torch.float16: 'f16'}.get(pay)
        self.reducer = BucketReducer(
            self.grad, self.table, bucket_mb * (1 << 20) // 4, self.pg, payload=pay,
            cast=lambda src, dst: self._lc('fami_cast_add_' + sfx, _p(src), _p(dst), src.numel(), 0, _stream(self.dev)),
            widen=lambda src, dst: self._lc('fami_widen_' + sfx, _p(src), _p(dst), src.numel(), _stream(self.dev)))
        self.reducer.world = self.world
        self.packer = WeightPacker(model, self.flat, self.table, self.act_dtype, cats=self.cats, route=self.route)
        # data-parallel launch plan: 'overlap' (default) = hipGraph segments cut at the bucket boundaries with each
        # bucket's all-reduce issued between two segment replays (graph replay AND overlap with the rest of backward);
        # 'serial' = one graph for forward + backward, then every all-reduce; FAMI_DDP_GRAPH=0 = no graphs at all
        # (eager launches, all-reduces fired from the Engine.backward hooks)
        self.ddp_plan = options.get('FAMI_DDP_PLAN')
        self.use_graph = use_graph and (not self.ddp or options.flag('FAMI_DDP_GRAPH'))
        self._cache = {}          # batch shapes -> (plan, static inputs, static outputs, optimizer hyper version)
        head.place(self.dev, self.accum_steps > 1)
        self.scalar_terms = head.terms       # the terms kept beside loss_parts (head.ScalarTerm): integral first, structure second
        if hasattr(model, '_ensure_nbt'):
            model._ensure_nbt(self.dev)      # BatchNorm counters move into their arena BEFORE any snapshot is taken
        if self.ddp:
            self.broadcast_parameters()
        # the moving average of the weights: a second parameter arena and {updates, decay_t, 1 - decay_t, apply}
        self.ema = self.ema_state = None
        self._ema_version = 0
        self._ema_swapped = False       # inside ema_weights(): `flat` holds the average, `ema` the raw weights
        if self.ema_decay is not None:
            self.ema = self.flat.detach().clone()
            self.ema_state = torch.zeros(4, device=self.dev)
            self._set_ema_updates(0)

    @classmethod
    def from_cfg(cls, cfg, model, **trainer_kw):
        """A Trainer with the optimizer the reference's build_optimizer makes of `cfg` (optimizer_kwargs); `trainer_kw`
        takes the other Trainer arguments and wins over the config."""
        kw = optimizer_kwargs(cfg)
        if cfg.get('LOSS', {}).get('USE_DIFFERENT_JOINTS_WEIGHT', False):      # datasets/zoo/base.py:46, mppe_config.py:240
            from .data import JOINTS_WEIGHT
            if 'joint_weights' not in trainer_kw and cfg['MODEL']['NUM_JOINTS'] != len(JOINTS_WEIGHT):
                raise ValueError('LOSS.USE_DIFFERENT_JOINTS_WEIGHT: the only vector at hand is PoseTrack\'s for %d joints, the '
                                 'model has %d -- pass joint_weights=' % (len(JOINTS_WEIGHT), cfg['MODEL']['NUM_JOINTS']))
            kw['joint_weights'] = JOINTS_WEIGHT
        integral = cfg.get('LOSS', {}).get('INTEGRAL_L1', {})      # mppe_config.py:217-219, core fn :61-69
        if integral.get('USE', False):
            kw['integral_l1_weight'] = integral.get('WEIGHT', 1.0)
        structure = cfg.get('LOSS', {}).get('STRUCTURE_COSINE', {})      # mppe_config.py:225-227, core fn :62-70
        if structure.get('USE', False):
            kw['structure_cos_weight'] = structure.get('WEIGHT', 1.0)
        kw.update(trainer_kw)
        return cls(model, **kw)

    def _lc(self, name, *args):
        """a library entry point under this trainer's route (weight packs and plans must see what its engines see)"""
        return lib().call_routed(self.route, name, *args)

    # ------------------------------------------------------------------ data parallel
    def broadcast_parameters(self):
        dist.broadcast(self.flat, src=0, group=self.pg)
        for b in self.model.buffers():
            if b.dtype.is_floating_point:
                dist.broadcast(b, src=0, group=self.pg)

    def measure_allreduce_ms(self, reps=3):
        """Wall time of one bucketed all-reduce of the whole gradient arena with nothing else running (reporting only;
        the arena content is scaled back afterwards)."""
        if not self.ddp:
            return 0.0
        import time
        torch.cuda.synchronize(self.dev)
        best = None
        for _ in range(reps):
            dist.barrier(group=self.pg)
            torch.cuda.synchronize(self.dev)
            t0 = time.perf_counter()
            for lo, hi in self.reducer.ranges():
                self.reducer.allreduce(lo, hi)
            self.reducer.wait()
            torch.cuda.synchronize(self.dev)
            dt = (time.perf_counter() - t0) * 1e3
            best = dt if best is None else min(best, dt)
            self.grad.mul_(1.0 / self.world)
        return best

    def _dcn_bwd_images(self):
        """[(weight, persistent image buffer, (Co, C, kh, kw, G))] of the model's DCN layers (built once)."""
        if getattr(self, '_dcn_imgs', None) is None:
            from .zoo.alignment_v15 import DeformConv2d
            G = getattr(self.model, 'G', None)
            imgs = []
            lib().bind(self.route)       # (the image size follows the route's plan of the register-fed backward kernel)
            if G is not None:
                for m in self.model.modules():
                    if isinstance(m, DeformConv2d):
                        Co, C, kh, kw = m.weight.shape
                        n = lib().cdll.fami_dcn_packed_weight_bwd_elems(Co, C, kh, kw, G)
                        nf = lib().cdll.fami_dcn_packed_weight_elems(Co, C, kh, kw, G)
                        imgs.append((m.weight, torch.empty(n, device=self.dev), (Co, C, kh, kw, G),
                                     torch.empty(nf, device=self.dev)))
            self._dcn_imgs = imgs
        return self._dcn_imgs

    # ------------------------------------------------------------------ the step (eager launch sequence)
    def _forward_backward(self, kf_x, sup_x, target, weight, on_bucket=None, fused_opt=False):
        """Enqueue forward, loss and backward of one batch.  fused_opt (set only by _single_step): the Adam update may be enqueued
        from INSIDE the backward pass in two parts (_find_adam_split) -- the call then mutates the parameters, and _single_step
        enqueues only the moving average behind it.  Direct callers (tools, tests) get a pure gradient computation."""
        model = self.model
        eng = Engine(self.dev, grad_views=self.views, dtype=self.act_dtype,
                     deterministic=getattr(model, 'deterministic', None), route=self.route)
        self.last_nfused = eng.nfused       # (tools read the counters; not the engine itself: its callbacks point back here, and a
                                            #  Trainer kept alive by that cycle is collected at a random time -- e.g. inside the next capture)
        if on_bucket is not None:
            eng.persist_lanes = False       # bucket hooks fire between forked regions: keep a join per module
        early = {'ev': None}
        split = self._backward_split() if (fused_opt and on_bucket is None) else None
        if split is not None:
            # Adam in two parts (see _find_adam_split): the scalars now, everything but the stem stretch when backward reaches the
            # stage-2 boundary (side lane), the stem stretch behind the backward pass
            for o in self.optimizers:
                o.prep(eng.stream)

            def on_mark(name):
                if name == 'stage2' and early['ev'] is None:
                    eng.flush_reduces()
                    eng.sync_wgrad_lane()
                    n = self.flat.numel()

                    def upd(st):
                        for o in self.optimizers:
                            o.apply(0, split[0], st)
                            o.apply(split[1], n, st)
                    early['ev'] = eng.side_launch(upd)
            eng.on_mark = on_mark
        # conv weight images of this step: the forward orientation in one launch now, the input-gradient orientation in a
        # second launch on a side lane beside the forward pass (first read by the backward pass, which waits for it)
        # ... and the DCN layers' backward weight images + their fixed-point scale bound (a one-workgroup reduction): they
        # depend on the weights only, and packed inside the backward closures they sat on the head's serial chain
        dcn = self._dcn_bwd_images()

        from .engine import _SFX
        pack_fwd_fn = 'fami_dcn_pack_weight' + _SFX[self.act_dtype]

        def pack_dcn_fwd(st):
            # the DCN layers' FORWARD weight images (three small launches per layer) sat on the head's serial chain too:
            # packed on a side lane at the start of the step, joined before the head
            for w, _, geo, fbuf in dcn:
                self._lc(pack_fwd_fn, _p(w.data), _p(fbuf), *geo, st)

        def pack_bwd(st):
            self.packer.run(st, 1)
            for w, buf, geo, _ in dcn:
                self._lc('fami_dcn_pack_weight_bwd_f32', _p(w.data), _p(buf), *geo, st)
        if eng.use_lanes:
            # (round 5: starting the late / input-gradient packs at stage 2 / 3 on the weight-gradient stream instead of beside the stem
            #  stretch measured no gain -- bf16 20.26 vs 20.23 ms, f32 45.92 vs 45.72; all packing removed is worth 0.37 / 0.72 ms)
            if self.packer.n_early > 0:
                self.packer.run(eng.stream, 'early')
                eng.late_weights_ready = eng.side_launch(lambda st: self.packer.run(st, 'late'))   # HRNetBody.run waits before stage 3
            else:
                self.packer.run(eng.stream, 0)
            packed_fwd = eng.side_launch(pack_dcn_fwd) if dcn else None
            packed_bwd = eng.side_launch(pack_bwd)
        else:
            self.packer.run(eng.stream)
            pack_dcn_fwd(eng.stream)
            for w, buf, geo, _ in dcn:
                self._lc('fami_dcn_pack_weight_bwd_f32', _p(w.data), _p(buf), *geo, eng.stream)
            packed_fwd = packed_bwd = None
        eng.prepacked = self.packer.views
        eng.prepacked_dcn_bwd = {id(w): buf for w, buf, _, _ in dcn}
        eng.prepacked_dcn_fwd = {id(w): fbuf for w, _, _, fbuf in dcn}
        eng.dcn_fwd_ready = packed_fwd          # event the first DCN forward waits for
        target, weight, joints = self.head.targets(eng, kf_x, target, weight)
        outs, _ = model._body(eng, kf_x, sup_x)
        model._advance_bn_counters(eng)
        seed = self.head.forward(eng, kf_x, outs, target, weight, joints)
        # the loss scale of the seeds: a host factor, or (dynamic) the device scalar the scale update rewrites
        ls, ls_dev = (1.0, self.scaler_state[0:1]) if self.dynamic_scale else (self.loss_scale, None)
        seeded = seed(ls, ls_dev)       # noqa: F841  (the seed buffer, held until the backward pass is enqueued)
        hook = None
        if on_bucket is not None:
            def bucket_ready(lo, hi):
                eng.sync_wgrad_lane()       # the slice's weight gradients live on the engine's wgrad stream
                return on_bucket(lo, hi)
            hook = self.reducer.begin(bucket_ready)
        if packed_bwd is not None:
            eng.wait_main(packed_bwd)
        eng.backward(on_params_done=hook)
        if split is not None:
            for o in self.optimizers:
                if early['ev'] is not None:
                    o.apply(split[0], split[1], eng.stream)
                else:
                    o.apply(0, self.flat.numel(), eng.stream)
            if early['ev'] is not None:
                eng.wait_main(early['ev'])
        self.conv_flops = eng.conv_flops        # nn.Conv2d FLOPs of one step (forward + both gradients; reporting)
        if on_bucket is not None:
            self._flushing = True
            try:
                self.reducer.flush()
            finally:
                self._flushing = False
        return outs

    _flushing = False
    conv_flops = 0

    def ohkm_selection(self):
        """OHKM: the joints the last step's loss counted, a device bool tensor [B,J] (None without ohkm_topk or before the
        first step): the selected weights are non-zero there.  A joint of weight 0 that fills one of the k places -- a
        sample with fewer than k visible joints -- adds nothing to loss or gradient and reads False."""
        return self.head.ohkm_selection()

    def integral_coords(self):
        """integral_l1_weight: the soft-argmax coordinates the last step's loss saw, a device tensor [B,J,2] in heatmap pixels
        (None without the option or before the first step)."""
        return self.head.integral_coords()

    def structure_cosines(self):
        """structure_cos_weight: the cosine of every limb of the last step, a device tensor [B,P], NaN where the limb was not
        valid (loss.limb_cosines on the coordinates, target positions and target weights the step's loss saw; None without the
        option or before the first step).  Logging only: it launches outside the captured plan."""
        return self.head.structure_cosines()

    def skipped_steps(self):
        """Optimizer steps skipped so far because the loss-scaled gradients held inf / NaN (fp16 mode; synchronises).
        The scale is static: a count that keeps growing means the scale is too large for this model."""
        return 0 if self.overflow is None else int(self.overflow[1].item())

    def _find_adam_split(self, model):
        """(lo, hi): the arena range of the stem / layer1 / first-transition parameters, whose gradients are the LAST the backward
        pass completes.  Everything outside it is final when backward reaches the boundary of stage 2 (modules.HRNetBody.run marks
        it), so its Adam update can run on a side lane beside the rest of the backward pass instead of behind it (the one-launch
        Adam is 0.33 ms of pure HBM traffic at the end of every step).  None: no such split (fp16's checked step, data-parallel
        plans, a frozen backbone; gradient clipping, which needs the total norm before any update; a dynamic loss scale; gradient
        accumulation, whose update follows the last backward pass of a window)."""
        if self.loss_scale != 1.0 or self.dynamic_scale or self.max_grad_norm is not None or self.accum_steps > 1:
            return None
        hr = getattr(model, 'hrnet', None)
        if hr is None or not hasattr(hr, 'stage2') or not hasattr(hr, 'conv1'):
            return None
        off = {id(p): o for p, o, n in self.table}
        first = [p for p in hr.stage2.parameters() if id(p) in off]
        if id(hr.conv1.weight) not in off or not first:
            return None
        lo, hi = off[id(hr.conv1.weight)], min(off[id(p)] for p in first)
        return (lo, hi) if 0 <= lo < hi else None

    def _update(self, fold=False):
        """Everything between "the gradient arena holds this step's raw gradients" and the end of the step -- wherever a step
        ends, eager or inside a capture: the one pass over the gradient arena (or none), the clip coefficient and the
        loss-scale update, every group's optimizer step, the moving average.  fold: the accumulation arena is added inside
        the pass (the single-process call that closes a window)."""
        self._grad_pass(fold)
        self._coef_and_scale_update(_stream(self.dev))
        self._step_optimizers()
        self._ema_step()

    def _step_optimizers(self):
        """every group's step (prep + its runs); one group: exactly FlatAdam.step / FlatSGD.step"""
        for k, o in enumerate(self.optimizers[1:]):
            flag = None
            if self._group_flags is not None:
                flag = self._group_flags[k]
                flag[0].copy_(self.overflow[0])
            o.step(flag)
        self.opt.step(self.overflow)

    def _backward_split(self):
        """the arena range a _forward_backward(fused_opt=True) without bucket hooks splits the optimizers around
        (_find_adam_split), None where it enqueues none: the one condition both it and _single_step behind it go by"""
        return None if self.ddp else self._adam_split

    def _opt_tensors(self):
        """the parameter arena and every optimizer's device state (shared arenas once), with the loss-scaler vector, the
        clip vector and the moving average with its state vector where they exist: what a capture's warm-up steps must not
        leave changed"""
        out, seen = [self.flat] + [t for t in (self.scaler_state, self.clip, self.ema, self.ema_state) if t is not None], set()
        for o in self.optimizers:
            for t in o.tensors():
                if id(t) not in seen:
                    seen.add(id(t))
                    out.append(t)
        return out

    def _frozen_key(self):
        """which BatchNorm modules have frozen statistics right now: part of what keys a captured plan"""
        return tuple(k for k, m in enumerate(self._bn_modules) if getattr(m, 'frozen_stats', False))

    def frozen_bn_names(self):
        """-> the names of the model's BatchNorm modules with frozen statistics (the 'frozen_bn' checkpoint entry)"""
        return frozen_batchnorm_names(self.model)

    def _hyper_version(self):
        return tuple(o.hyper_version for o in self.optimizers) + (self._scaler_version, self._ema_version,
                                                                  self._frozen_key())

    def _grad_factor(self):
        """the host factor of the gradient pass, 1 / (world * accum_steps * loss_scale): the data-parallel mean, the mean over
        a window's micro-batches and the static loss scale (a dynamic one is read from the device: 1 here)"""
        return 1.0 / ((self.world if self.ddp else 1) * self.accum_steps * (1.0 if self.dynamic_scale else self.loss_scale))

    def _grad_pass(self, fold):
        """The one pass over the gradient arena in front of the optimizers, chosen by: guarded (an overflow flag exists),
        clipping, dynamic scale, fold.  grad = (grad [+ accum]) * factor [* the device's 1 / scale], with the inf / NaN check
        where the trainer is guarded and the sum of squares of what was written where it clips (a null flag / slab pointer
        switches either off); the read-only reduction when clipping has nothing to multiply; no launch when there is
        nothing to do.  The clip coefficient and the scale update behind it (_coef_and_scale_update) must see the overflow
        flag before the optimizers' checked prep clears it, once per step."""
        s, n, f = _stream(self.dev), self.grad.numel(), self._grad_factor()
        inv = _p(self.scaler_state[1:2]) if self.dynamic_scale else None
        flag, slab = _p(self.overflow), _p(self._partials)            # (null: unguarded / not clipping)
        if fold:
            self._lc('fami_accum_unscale_check_sumsq_f32', _p(self.grad), _p(self.accum), n, f, inv, flag, slab, s)
        elif self.dynamic_scale or (self.clip is not None and f != 1.0):
            self._lc('fami_unscale_check_sumsq_f32', _p(self.grad), n, f, inv, flag, slab, s)
        elif self.clip is not None:
            self._lc('fami_sumsq_f32', _p(self.grad), n, slab, s)
        elif self.overflow is not None:
            # static loss scaling (fp16): the same pass also looks for inf / NaN; Adam then skips the step
            self._lc('fami_unscale_check_f32', _p(self.grad), n, f, flag, s)
        elif f != 1.0:
            self._lc('fami_axpby_f32', _p(self.grad), None, _p(self.grad), n, f, 0.0, s)

    def _coef_and_scale_update(self, s):
        """the clip coefficient from the slab, then the loss-scale update: both read the overflow flag the pass in front of them
        raised, before the optimizers' checked prep clears it"""
        if self.clip is not None:
            self._lc('fami_clip_coef_f32', _p(self._partials), self._partials.numel(), _p(self.clip[2:3]), _p(self.clip[0:2]),
                     _p(self.overflow), s)
        if self.dynamic_scale:
            c = self.scaler_cfg
            self._lc('fami_loss_scale_update_f32', _p(self.scaler_state), _p(self.overflow), float(c['growth_factor']),
                     float(c['backoff_factor']), int(c['growth_interval']), s)

    def set_max_grad_norm(self, v):
        """A new clip threshold, written into the device scalar the coefficient kernel reads: captured plans keep replaying
        (like set_lr).  Clipping itself is switched on at construction."""
        if self.clip is None:
            raise ValueError('this Trainer was built without max_grad_norm')
        if not float(v) > 0.0:
            raise ValueError('max_grad_norm must be positive, not %r' % (v,))
        self.max_grad_norm = float(v)
        self.clip[2] = self.max_grad_norm

    def grad_norm(self):
        """Total 2-norm of the last step's gradients before clipping (host float; forces a sync -- logging only)."""
        return None if self.clip is None else float(self.clip[0].item())

    def clip_coef(self):
        """The factor the last step's gradients were multiplied by, min(1, max_grad_norm / (norm + 1e-6)) (host float;
        forces a sync -- logging only)."""
        return None if self.clip is None else float(self.clip[1].item())

    def loss_scale_value(self):
        """The current loss scale (host float; with a dynamic scale it forces a sync -- logging only)."""
        return float(self.scaler_state[0].item()) if self.dynamic_scale else self.loss_scale

    def scaler_state_dict(self):
        """torch.amp.GradScaler.state_dict() of the dynamic loss scale (synchronises)."""
        scale, _, tracker = self.scaler_state.tolist()
        c = self.scaler_cfg
        return {'scale': scale, 'growth_factor': float(c['growth_factor']), 'backoff_factor': float(c['backoff_factor']),
                'growth_interval': int(c['growth_interval']), '_growth_tracker': int(tracker)}

    def load_scaler_state_dict(self, sd):
        """The inverse.  Growth / backoff factor and interval are kernel arguments of the captured plan: a change re-captures."""
        c = self.scaler_cfg
        new = {'growth_factor': float(sd['growth_factor']), 'backoff_factor': float(sd['backoff_factor']),
               'growth_interval': int(sd['growth_interval'])}
        if any(c[k] != v for k, v in new.items()):
            c.update(new)
            self._scaler_version += 1
        scale = float(sd['scale'])
        self.scaler_state.copy_(torch.tensor([scale, 1.0 / scale, float(sd['_growth_tracker'])]))

    # ------------------------------------------------------------------ moving average of the weights (ema_decay)
    def _ema_step(self):
        """behind the optimizers, wherever a step ends: the scalars (gated by the base group's applied / skipped scalar),
        then the one pass over both arenas"""
        if self.ema is None:
            return
        s = _stream(self.dev)
        self._lc('fami_ema_prep_f32', _p(self.ema_state), _p(self.opt.state[2:3]), self.ema_decay, int(self.ema_warmup), s)
        self._lc('fami_ema_update_f32', _p(self.ema), _p(self.flat), self.flat.numel(), _p(self.ema_state), s)

    def _require_ema(self):
        if getattr(self, 'ema', None) is None:
            raise ValueError('this Trainer was built without ema_decay')
        if getattr(self, '_ema_swapped', False):
            raise RuntimeError('inside ema_weights(): the two arenas are exchanged')

    def _set_ema_updates(self, t):
        """ema_state after `t` applied updates, in the kernel's own fp32 arithmetic (fami_ema_prep_f32)"""
        d = torch.tensor(self.ema_decay, dtype=torch.float32)
        if self.ema_warmup and t > 0:
            tt = torch.tensor(float(t), dtype=torch.float32)
            d = torch.minimum(d, (1.0 + tt) / (10.0 + tt))
        self.ema_state.copy_(torch.stack([torch.tensor(float(t)), d, 1.0 - d, torch.tensor(1.0 if t > 0 else 0.0)]))

    def set_ema_decay(self, v, warmup=None):
        """A new decay (and, optionally, warm-up switch).  Both are kernel arguments of the captured plan: a change
        re-captures on the next step(), like set_hyper of the optimizers."""
        self._require_ema()
        new = (_check_ema_decay(v), self.ema_warmup if warmup is None else bool(warmup))
        if new != (self.ema_decay, self.ema_warmup):
            self.ema_decay, self.ema_warmup = new
            self._ema_version += 1

    def ema_updates(self):
        """Updates the average has received: applied optimizer steps since construction / reset_ema() (host int; forces
        a sync -- logging only)."""
        return None if self.ema is None else int(self.ema_state[0].item())

    def ema_decay_value(self):
        """The decay of the last update -- below ema_decay while the warm-up ramp is active (host float; forces a sync --
        logging only)."""
        return None if self.ema is None else float(self.ema_state[1].item())

    def reset_ema(self):
        """Restart the average from the current weights: ema = flat, 0 updates (in place: captured plans keep replaying)."""
        self._require_ema()
        with torch.no_grad():
            self.ema.copy_(self.flat)
        self._set_ema_updates(0)

    @contextlib.contextmanager
    def ema_weights(self):
        """Context manager: inside it every trainable parameter of `model` reads its averaged value -- model(...) under
        torch.no_grad(), evaluate.predict / evaluate_loop and model.state_dict() all see the average, together with the
        LIVE BatchNorm buffers (class docstring).  Entry exchanges the parameter arena and `ema` in place
        (fami_swap_f32: one pass, no third arena), exit exchanges them back: both are then bitwise what they were.
        step(), save_checkpoint, the ema_* state methods and a nested ema_weights() raise RuntimeError inside."""
        self._require_ema()
        n, s = self.flat.numel(), _stream(self.dev)
        self._lc('fami_swap_f32', _p(self.flat), _p(self.ema), n, s)
        self._ema_swapped = True
        try:
            yield self
        finally:
            self._lc('fami_swap_f32', _p(self.flat), _p(self.ema), n, _stream(self.dev))
            self._ema_swapped = False

    def _ema_rows(self):
        """[(state_dict key, parameter, offset, elements)] of the arena, in table order"""
        names = {id(p): k for k, p in self.model.named_parameters()}
        return [(names[id(p)][7:] if names[id(p)].startswith('module.') else names[id(p)], p, off, n)
                for p, off, n in self.table]

    def ema_state_dict(self):
        """The 'ema' checkpoint entry: {'decay', 'warmup', 'updates', 'params': {state_dict key of each trainable parameter:
        host fp32 tensor}} (synchronises).  {**model.state_dict(), **entry['params']} is a state_dict of the averaged model."""
        self._require_ema()
        params = {k: self.ema[off:off + n].view(p.shape).detach().cpu().clone() for k, p, off, n in self._ema_rows()}
        return {'decay': float(self.ema_decay), 'warmup': bool(self.ema_warmup), 'updates': int(self.ema_state[0].item()),
                'params': params}

    def check_ema_state_dict(self, sd):
        """ValueError unless the entry names exactly this Trainer's trainable parameters, with their shapes; loads nothing."""
        self._require_ema()
        rows = self._ema_rows()
        params = sd['params']
        missing = [k for k, _, _, _ in rows if k not in params]
        extra = sorted(set(params) - {k for k, _, _, _ in rows})
        if missing or extra:
            raise ValueError("'ema' entry mismatch: missing %s unexpected %s" % (missing[:5], extra[:5]))
        for k, p, _, _ in rows:
            if tuple(params[k].shape) != tuple(p.shape):
                raise ValueError("'ema' entry %s has shape %s, the parameter %s" % (k, tuple(params[k].shape), tuple(p.shape)))
        _check_ema_decay(sd['decay'])
        if int(sd['updates']) < 0:
            raise ValueError("'ema' entry with %d updates" % int(sd['updates']))

    def load_ema_state_dict(self, sd):
        """The inverse of ema_state_dict (checked first: a refused entry loads nothing).  Decay and warm-up switch are taken
        from the entry; where they differ from this Trainer's, a captured plan re-captures."""
        self.check_ema_state_dict(sd)
        self.set_ema_decay(sd['decay'], sd.get('warmup', False))
        with torch.no_grad():
            for k, p, off, n in self._ema_rows():
                self.ema[off:off + n].copy_(sd['params'][k].reshape(-1).to(torch.float32))
        self._set_ema_updates(int(sd['updates']))

    # ------------------------------------------------------------------ gradient accumulation (accum_steps > 1)
    def _accumulate(self):
        """window position k < N - 1, behind the backward pass: accum = grad (k = 0) or accum = accum + grad"""
        self._lc('fami_axpby_f32', _p(self.grad), _p(self.accum) if self.window_position else None, _p(self.accum),
                 self.grad.numel(), 1.0, 1.0, _stream(self.dev))

    def _exchange_window(self):
        """data parallel, a window's last call: grad = accum + grad, then every bucket's all-reduce (outside any graph)"""
        self._lc('fami_axpby_f32', _p(self.accum), _p(self.grad), _p(self.grad), self.grad.numel(), 1.0, 1.0, _stream(self.dev))
        for lo, hi in self.reducer.ranges():
            self.reducer.allreduce(lo, hi)
        self.reducer.wait()

    def _window_call_done(self, closing):
        """the loss parts of this call into the window sum (one 7-element launch; row 0: the open window, row 1: the last
        closed one), every scalar term into a sum of its own, and the host-side position"""
        for value, w, n in [(self.loss_parts, self._window_loss, 7)] + [(t.value, t.window, 1) for t in self.scalar_terms]:
            self._lc('fami_axpby_f32', _p(value), _p(w[0]) if self.window_position else None, _p(w[1 if closing else 0]),
                     n, 1.0, 1.0, _stream(self.dev))
        self.window_position = 0 if closing else self.window_position + 1

    def reset_window(self):
        """Drop an open window: the next call is position 0 (which overwrites the accumulation arena; no launch here)."""
        self.window_position = 0

    def window_loss_value(self):
        """Mean over the last closed window of what loss_value() reports per call (host float; forces a sync -- logging
        only).  None without accumulation."""
        if self._window_loss is None:
            return None
        return sum((t.window[1].item() / self.accum_steps for t in self.scalar_terms),
                   self._total_loss((self._window_loss[1] / self.accum_steps).tolist()))

    def accum_state_dict(self):
        """The 'grad_accum' checkpoint entry: {'steps': N, 'position': k} and, inside a window (k > 0), the accumulation
        arena and the open window's loss sum on the host (synchronises); with integral_l1_weight / structure_cos_weight also the
        open window's sum of that term under the term's own key (head.ScalarTerm.key)."""
        sd = {'steps': self.accum_steps, 'position': self.window_position}
        if self.window_position > 0:
            sd['arena'] = self.accum.detach().cpu().clone()
            sd['loss_sum'] = self._window_loss[0].detach().cpu().clone()
            for t in getattr(self, 'scalar_terms', ()):      # (getattr: checkpoint code borrows this method for host objects)
                sd[t.key] = t.window[0].detach().cpu().clone()
        return sd

    def load_accum_state_dict(self, sd):
        """The inverse, into a Trainer with the same accum_steps (ValueError otherwise)."""
        if int(sd['steps']) != self.accum_steps:
            raise ValueError('the checkpoint was written with accum_steps=%d, this Trainer has accum_steps=%d' %
                             (int(sd['steps']), self.accum_steps))
        k = int(sd['position'])
        if not 0 <= k < self.accum_steps:
            raise ValueError('window position %d outside a window of %d micro-batches' % (k, self.accum_steps))
        if k > 0:
            self.accum.copy_(sd['arena'])
            self._window_loss[0].copy_(sd['loss_sum'])
            for t in getattr(self, 'scalar_terms', ()):
                if t.key not in sd:
                    raise ValueError('the checkpoint was written inside a window without ' + t.without)
                t.window[0].copy_(sd[t.key])
        self.window_position = k

    def _accum_eager_step(self, kf_x, sup_x, target, weight):
        closing = self.window_position == self.accum_steps - 1
        outs = self._forward_backward(kf_x, sup_x, target, weight)
        if not closing:
            self._accumulate()
        else:
            if self.ddp:
                self._exchange_window()
            self._update(fold=not self.ddp)      # (behind the exchange the arena already is the window's sum)
        self._window_call_done(closing)
        return outs

    def _single_step(self, kf_x, sup_x, target, weight):
        """A whole step of a single process without accumulation (eager, or inside the one captured graph).  With an
        in-backward optimizer split the gradient pass (none: the split is off wherever one is needed) and the optimizers
        were enqueued inside the backward pass: the moving average is what remains of the update."""
        outs = self._forward_backward(kf_x, sup_x, target, weight, fused_opt=True)
        if self._backward_split() is not None:
            self._ema_step()
        else:
            self._update()
        return outs

    def _eager_step(self, kf_x, sup_x, target, weight):
        if self.accum_steps > 1:
            return self._accum_eager_step(kf_x, sup_x, target, weight)
        if not self.ddp:
            return self._single_step(kf_x, sup_x, target, weight)
        outs = self._forward_backward(kf_x, sup_x, target, weight, on_bucket=self.reducer.allreduce)
        self.reducer.wait()
        self._update()
        return outs

    # ------------------------------------------------------------------ hipGraph capture / replay
    def _capture(self, kf_x, sup_x, target, weight):
        """Capture with the cyclic garbage collector off: a collection that starts inside a capture may destroy an older Trainer's
        graph (Engine / Trainer objects are reference cycles through their callbacks, so `del trainer` leaves them to the collector),
        and destroying a graph while a stream captures in the global mode aborts the process (hipErrorStreamCaptureUnsupported out
        of ~CUDAGraph).  torch.cuda.graph() no longer collects on entry in this PyTorch, so it is done here."""
        import gc
        was = gc.isenabled()
        gc.collect()
        gc.disable()
        try:
            return self._capture_plan(kf_x, sup_x, target, weight)
        finally:
            if was:
                gc.enable()

    def _warm_up(self, run, times, state, buffers):
        """`times` runs of `run` on a side stream before a capture (allocator + pack caches), rolled back.  state: the
        parameters, every optimizer's device state and the scaler / clip / moving-average tensors (_opt_tensors) and the
        overflow vector {raised, skipped steps} are restored; buffers: the module buffers are."""
        keep = []
        if state:
            keep += self._opt_tensors() + ([] if self.overflow is None else [self.overflow])
        if buffers:
            keep += list(self.model.buffers())
        snap = [t.clone() for t in keep]
        side = torch.cuda.Stream(self.dev)
        side.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(side):
            for _ in range(times):
                run()
        torch.cuda.current_stream(self.dev).wait_stream(side)
        torch.cuda.synchronize(self.dev)
        for dst, src in zip(keep, snap):
            dst.copy_(src)
        torch.cuda.synchronize(self.dev)

    def _capture_plan(self, kf_x, sup_x, target, weight):
        st = {'kf': kf_x.clone(), 'sup': sup_x.clone(), 'target': target.clone(), 'weight': weight.clone()}
        if self.accum_steps > 1:
            return self._capture_accum_plan(st)
        batch = (st['kf'], st['sup'], st['target'], st['weight'])
        # The warm-up steps must not count as training steps: the parameters, Adam state and module buffers (BN running
        # statistics, batch counters) are restored afterwards, so the first step() of a graph-mode Trainer is exactly one
        # optimisation step, like the eager one.
        self._warm_up(lambda: self._eager_step(*batch), 2, state=True, buffers=True)
        if not self.ddp:
            g = torch.cuda.CUDAGraph()
            # (round 6 probe: capturing on a high-priority stream -- lane 0 is the step's critical path -- changes nothing:
            #  bf16 18.75 vs 18.70 ms, f32 44.78 vs 44.78, profiles/r06/ab_lane0_high_priority_*.txt)
            with torch.cuda.graph(g):
                outs = self._single_step(*batch)
            plan = [('graph', g)]
        elif self.ddp_plan == 'serial':
            # graph 1 = forward + backward, then the bucketed all-reduce of the flat gradient arena (RCCL, outside any
            # graph), then graph 2 = 1/world scale + Adam
            pool = torch.cuda.graph_pool_handle()
            g1 = torch.cuda.CUDAGraph()
            # thread_local: RCCL's watchdog thread may query events while this thread captures
            with torch.cuda.graph(g1, pool=pool, capture_error_mode='thread_local'):
                outs = self._forward_backward(*batch)
            plan = [('graph', g1)]
            plan += [('allreduce', r) for r in self.reducer.ranges()]
            plan.append(('wait', None))
            g2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g2, pool=pool, capture_error_mode='thread_local'):
                self._update()
            plan.append(('graph', g2))
        else:
            outs, plan = self._capture_overlap(st)
        entry = (plan, st, outs, self._hyper_version())
        return entry

    def _capture_accum_plan(self, st):
        """accum_steps > 1: ONE graph of forward + loss + backward for this batch shape, replayed at every window position (the
        accumulating launches and the exchange follow the replay, uncaptured), and the shape-independent tail
        (_capture_tail), captured the first time any shape is.  The warm-up runs the gradient computation alone: it never
        touches the accumulation arena, the window position or the window loss sum, so a shape first seen in the middle of
        a window (the smaller last batch of an epoch) leaves the open window as it was; module buffers (BN running
        statistics, batch counters) are restored, and the gradient arena is rewritten by the replay that follows."""
        batch = (st['kf'], st['sup'], st['target'], st['weight'])
        self._warm_up(lambda: self._forward_backward(*batch), 2, state=False, buffers=True)
        # (thread_local: RCCL's watchdog thread may query events while this thread captures)
        kw = {'capture_error_mode': 'thread_local'} if self.ddp else {}
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, **kw):
            outs = self._forward_backward(*batch)
        if self._tail is None or self._tail[1] != self._hyper_version():
            self._tail = (self._capture_tail(kw), self._hyper_version())
        return ([('graph', g)], st, outs, self._hyper_version())

    def _capture_tail(self, kw):
        """The graph a window's last call replays behind its backward pass (and, data parallel, behind the exchange): the
        closing pass, coefficient, scale update and optimizers.  Its one warm-up run is rolled back (parameters, optimizer
        state, scaler and clip vectors, overflow flag and count); it only reads the accumulation arena."""
        self._warm_up(lambda: self._update(fold=not self.ddp), 1, state=True, buffers=False)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, **kw):
            self._update(fold=not self.ddp)
        return g

    def _capture_overlap(self, st):
        """Data-parallel plan with graph replay AND overlap: the launch sequence of forward + backward is captured into
        one hipGraph per gradient bucket -- a segment ends where the backward tape has enqueued the last contribution
        to a bucket (BucketReducer's frontier; only outside forked stream-lane regions, so no cross-segment event) --
        and at replay the bucket's RCCL all-reduce is issued between two segment launches: it runs on RCCL's stream
        beside the next segment's kernels.  The tail segment is followed by wait + (1/world scale, Adam)."""
        pool = torch.cuda.graph_pool_handle()
        plan = []
        cap = torch.cuda.Stream(self.dev)
        cap.wait_stream(torch.cuda.current_stream(self.dev))
        torch.cuda.synchronize(self.dev)
        late = []
        with torch.cuda.stream(cap):
            cur = [torch.cuda.CUDAGraph()]
            cur[0].capture_begin(pool=pool, capture_error_mode='thread_local')
            mark = [lib().ncalls]

            def cut(lo, hi):
                if self._flushing:              # buckets without a gradient: nothing was enqueued since the last cut
                    late.append((lo, hi))
                    return
                if lib().ncalls == mark[0]:     # two buckets completed by the same tape entry: no empty segment
                    plan.append(('allreduce', (lo, hi)))
                    return
                cur[0].capture_end()
                plan.append(('graph', cur[0]))
                plan.append(('allreduce', (lo, hi)))
                cur[0] = torch.cuda.CUDAGraph()
                cur[0].capture_begin(pool=pool, capture_error_mode='thread_local')
                mark[0] = lib().ncalls

            try:
                outs = self._forward_backward(st['kf'], st['sup'], st['target'], st['weight'], on_bucket=cut)
                # a (possibly tiny) tail always exists: the stem's gradients complete after the last bucket boundary
                self._lc('fami_axpby_f32', _p(self.loss_parts), None, _p(self.loss_parts), 7, 1.0, 0.0, _stream(self.dev))
            finally:
                cur[0].capture_end()
            plan.append(('graph', cur[0]))
            plan += [('allreduce', r) for r in late]
            plan.append(('wait', None))
            g2 = torch.cuda.CUDAGraph()
            g2.capture_begin(pool=pool, capture_error_mode='thread_local')
            try:
                self._update()
            finally:
                g2.capture_end()
            plan.append(('graph', g2))
        torch.cuda.current_stream(self.dev).wait_stream(cap)
        torch.cuda.synchronize(self.dev)
        return outs, plan

    def step(self, kf_x, sup_x, target, weight):
        """-> (final_hm, kf_bb_hm, ...) of this step; self.loss_parts holds [mse*W, mi_1..mi_6] on device, self.acc
        the PCK rows.  Graph mode keeps one captured plan per batch shape: the DataLoader of the reference has no
        drop_last, so the last batch of an epoch is usually smaller (datasets/zoo/build.py:32-50).  With accum_steps = N > 1
        a call is one micro-batch; the N-th of a window updates the parameters (class docstring)."""
        if self._ema_swapped:
            raise RuntimeError('step() inside ema_weights(): the parameter arena holds the averaged weights')
        weight = weight.reshape(weight.shape[0], -1).float().contiguous()
        target = target.float().contiguous()
        if not (kf_x.shape[0] == sup_x.shape[0] == target.shape[0] == weight.shape[0]):
            raise ValueError('batch sizes differ: kf %s sup %s target %s weight %s' %
                             (tuple(kf_x.shape), tuple(sup_x.shape), tuple(target.shape), tuple(weight.shape)))
        self.head.shape = (target.shape[0], target.shape[1])       # (here: a replay does not pass through _forward_backward)
        if not self.use_graph:
            return self._eager_step(kf_x, sup_x, target, weight)
        key = (tuple(kf_x.shape), tuple(sup_x.shape), tuple(target.shape), tuple(weight.shape))
        entry = self._cache.get(key)
        if entry is None or entry[3] != self._hyper_version():
            entry = self._cache[key] = self._capture(kf_x, sup_x, target, weight)
        plan, st, outs, _ = entry
        st['kf'].copy_(kf_x, non_blocking=True)
        st['sup'].copy_(sup_x, non_blocking=True)
        st['target'].copy_(target, non_blocking=True)
        st['weight'].copy_(weight, non_blocking=True)
        if self.accum_steps > 1:
            closing = self.window_position == self.accum_steps - 1
            plan[0][1].replay()
            if not closing:
                self._accumulate()
            else:
                if self.ddp:
                    self._exchange_window()
                self._tail[0].replay()
            self._window_call_done(closing)
            return outs
        for kind, obj in plan:
            if kind == 'graph':
                obj.replay()
            elif kind == 'allreduce':
                self.reducer.allreduce(*obj)
            else:
                self.reducer.wait()
        return outs

    def plan_summary(self):
        """{'graphs': n, 'allreduces': n} of the most recently captured plan (reporting)."""
        if not self._cache:
            return {'graphs': 0, 'allreduces': len(self.reducer.ranges()) if self.ddp else 0}
        plan = list(self._cache.values())[-1][0]
        return {'graphs': sum(1 for k, _ in plan if k == 'graph'), 'allreduces': sum(1 for k, _ in plan if k == 'allreduce')}

    def loss_value(self):
        """Total loss of the last step (host float; forces a sync -- logging only)."""
        return sum((t.value.item() for t in self.scalar_terms), self._total_loss(self.loss_parts.tolist()))

    def structure_loss_value(self):
        """The structure cosine term of the last step, weight included (host float; forces a sync -- logging only); 0.0 without
        structure_cos_weight."""
        return 0.0 if self.structure_loss is None else self.structure_loss.item()

    def integral_loss_value(self):
        """The integral L1 term of the last step, weight included (host float; forces a sync -- logging only); 0.0 without
        integral_l1_weight."""
        return 0.0 if self.integral_loss is None else self.integral_loss.item()

    def _total_loss(self, p):
        """[mse * W, mi_1..mi_6] -> the loss the reference optimises (core fn :119-148)"""
        a, b = self.alpha, self.beta
        mi = a * (-b * p[1] + b * p[2] + p[3] - p[4] + p[5] - p[6]) if self.use_mi else 0.0
        return p[0] + mi

    def accuracy(self):
        """PCK of the last step as the reference's `accuracy` returns it, for (final_hm, kf_bb_hm):
        -> [(acc[J+1] ndarray, avg_acc, cnt), (...)]  (host values; forces a sync -- logging only)."""
        if self.acc is None:
            return None
        rows = self.acc.cpu().numpy().astype('float64')
        J = rows.shape[1] - 3
        return [(r[:J + 1].copy(), float(r[J + 1]), int(r[J + 2])) for r in rows]


# the head's options (as it checked them) and its device results of the last step, read-only on the Trainer: loss_parts
# [mse * W, mi_1..mi_6], integral_loss / structure_loss [1] (None without the term), acc [2, J+3] (PCK rows; None before a step)
for _name in ('targets_from_joints', 'sigma', 'mse_weight', 'alpha', 'beta', 'use_mi', 'pck', 'subpixel', 'joint_weights', 'ohkm_topk',
              'integral_l1_weight', 'structure_cos_weight', 'structure_pairs', 'structure_min_len', 'structure_eps', 'loss_parts',
              'integral_loss', 'structure_loss', 'acc'):
    setattr(Trainer, _name, property(lambda self, _name=_name: getattr(self.head, _name)))
