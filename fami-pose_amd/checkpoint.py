"""Checkpoint / pretrained-weight compatibility with the reference.

File format of engine/defaults/checkpoints.py:45-67: ``epoch_{n}_state.pth`` holding
``{'begin_epoch': n, 'state_dict': model.state_dict() (module.-prefix stripped), 'optimizer': [optim.state_dict()]}``;
`resume` (:70-107) loads it back and returns ``begin_epoch + 1``; `get_latest_checkpoint` (:17-31) picks the highest
``epoch_N``.  The module tree of this repo has the reference's state_dict keys, so the model part is a plain
``state_dict``; the optimizer part converts between the flat-arena Adam of train.py and a ``torch.optim.Adam``
state_dict (per-parameter ``step`` / ``exp_avg`` / ``exp_avg_sq``, parameters numbered in ``model.parameters()`` order
restricted to ``requires_grad``, as posetimation/optimizer/optimizer.py:18-22,66-68 builds it).

SGD (train.FlatSGD, TRAIN.OPTIMIZER 'sgd') converts to and from a ``torch.optim.SGD`` state_dict: per-parameter
``momentum_buffer`` once a step with momentum has run, no per-parameter state otherwise.  torch's SGD keeps no step
count; a loaded buffer puts the flat SGD past its first step, so the next update takes the running momentum rule.

Learning-rate groups (Trainer lr_groups, TRAIN.LR_SECOND_GROUP): the reference builds a list of two Adams
(optimizer.py:18-55,69-72) and saves a list of two state dicts, each numbering only its own parameters; `resume`
matches them to the optimizers by parameter count (checkpoints.py:85-99).  A Trainer with groups writes and reads
exactly that list.  The single-group Adam format is the one `adam_state_dict` writes.  A state of the other optimizer
kind, or a parameter count that matches no group, raises instead of loading a partial state.

A Trainer with a dynamic loss scale (loss_scale='dynamic') adds one entry, ``'loss_scaler'``, in the layout of
``torch.amp.GradScaler.state_dict()`` (scale, growth_factor, backoff_factor, growth_interval, _growth_tracker), and
`resume` restores it; a checkpoint without the entry leaves a dynamic Trainer at its initial scale.  Without a dynamic
scale the file has exactly the three keys above.  max_grad_norm is a hyper-parameter of the run, not state: not saved.

A Trainer with gradient accumulation (accum_steps = N > 1) adds ``'grad_accum'``: ``{'steps': N, 'position': k}`` with k the
micro-batches in the open window and, when k > 0, ``'arena'`` (the accumulation arena, host fp32) and ``'loss_sum'`` (the
open window's seven loss parts), so a run saved inside a window continues bit for bit.  `resume` restores the entry into
a Trainer with the same accum_steps and raises ValueError on any other; a checkpoint without the entry starts an
accumulating Trainer at position 0.  Trainers without accumulation write today's keys exactly.

A Trainer with a moving average of the weights (ema_decay) adds ``'ema'``: ``{'decay', 'warmup', 'updates', 'params': {name:
host fp32 tensor}}`` with `name` the ``state_dict`` key of each trainable parameter (Trainer.ema_state_dict), so
``{**ckpt['state_dict'], **ckpt['ema']['params']}`` is a state_dict of the averaged model -- for a model of this repository
or of the reference.  BatchNorm buffers are not averaged: that dict takes them from ``'state_dict'``.  `resume` restores the
entry into an EMA Trainer; a parameter name or shape that does not match raises ValueError before anything is loaded.  An
EMA Trainer resuming a file without the entry restarts its average from the loaded weights (reset_ema: `resume` copies into
the parameters in place, so the average taken at construction would be stale).  A Trainer without an EMA ignores the entry
and writes exactly the keys above.

A Trainer with frozen BatchNorm statistics (frozen_bn / train.freeze_batchnorm; the flags live on the model's modules) adds
``'frozen_bn'``: the list of the frozen modules' names in ``named_modules()`` order.  `resume` into a model whose frozen set
differs -- none included -- raises ValueError naming both sets, before anything is loaded.  A file without the entry says nothing about the set (pretrained
weights, a run that trained the statistics) and loads into any Trainer.  Without the option the keys are unchanged.
"""
import os
import os.path as osp

import torch


def get_latest_checkpoint(checkpoint_save_folder):
    if not osp.isdir(checkpoint_save_folder):
        return None
    best, best_idx = None, None
    for name in sorted(os.listdir(checkpoint_save_folder)):
        if not name.endswith('.pth'):
            continue
        try:
            idx = int(name.split('_')[1])          # "epoch_{n}_state.pth"
        except (IndexError, ValueError):
            continue
        if best_idx is None or idx > best_idx:
            best, best_idx = osp.join(checkpoint_save_folder, name), idx
    return best


def _strip_module(sd):
    return {(k[7:] if k.startswith('module.') else k): v for k, v in sd.items()}


def adam_state_dict(trainer):
    """Flat-arena Adam (train.FlatAdam) -> torch.optim.Adam.state_dict() layout."""
    opt = trainer.opt
    step = float(opt.state[0].item())
    state = {}
    for i, (p, off, n) in enumerate(trainer.table):
        state[i] = {'step': torch.tensor(step), 'exp_avg': opt.m[off:off + n].view(p.shape).detach().cpu().clone(),
                    'exp_avg_sq': opt.v[off:off + n].view(p.shape).detach().cpu().clone()}
    group = {'lr': float(opt.state[1].item()), 'initial_lr': float(getattr(opt, 'initial_lr', opt.lr)), 'betas': tuple(opt.betas), 'eps': opt.eps, 'weight_decay': opt.wd,
             'amsgrad': False, 'maximize': False, 'foreach': None, 'capturable': False, 'differentiable': False,
             'fused': None, 'params': list(range(len(trainer.table)))}
    return {'state': state, 'param_groups': [group]}


def load_adam_state_dict(trainer, sd):
    """torch.optim.Adam.state_dict() (e.g. from a reference checkpoint) -> flat-arena Adam."""
    opt = trainer.opt
    if len(sd['param_groups'][0]['params']) != len(trainer.table):
        raise ValueError('optimizer state has %d parameters, the model has %d trainable ones' %
                         (len(sd['param_groups'][0]['params']), len(trainer.table)))
    steps = set()
    with torch.no_grad():
        opt.m.zero_()
        opt.v.zero_()
        for i, (p, off, n) in enumerate(trainer.table):
            st = sd['state'].get(i)
            if st is None:
                continue
            opt.m[off:off + n].copy_(st['exp_avg'].reshape(-1).to(opt.m.device))
            opt.v[off:off + n].copy_(st['exp_avg_sq'].reshape(-1).to(opt.v.device))
            steps.add(float(st['step']))
        if len(steps) > 1:
            raise ValueError('per-parameter step counts differ; the flat Adam keeps one')
        g = sd['param_groups'][0]
        # betas / eps / weight decay are kernel arguments baked into a captured hipGraph: set_hyper bumps the
        # optimizer's hyper_version and a graph-mode Trainer re-captures on its next step()
        opt.set_hyper(betas=g['betas'], eps=g['eps'], weight_decay=g['weight_decay'])
        t = steps.pop() if steps else 0.0
        opt.lr = float(g['lr'])
        # torch writes `initial_lr` once a scheduler has been attached; a checkpoint without it was never scheduled
        opt.initial_lr = float(g.get('initial_lr', g['lr']))
        opt.state.copy_(torch.tensor([t, g['lr'], 1.0 - opt.betas[0] ** t, 1.0 - opt.betas[1] ** t]))


def _kind(sd):
    g = sd['param_groups'][0]
    return 'adam' if 'betas' in g else 'sgd' if 'momentum' in g else 'unknown'


def _group_state_dict(opt, rows):
    """One flat optimizer (a learning-rate group over the table rows `rows`) -> torch.optim.Adam / SGD.state_dict() of
    a torch optimizer built on just those parameters."""
    step = float(opt.state[0].item())
    state = {}
    if opt.kind == 'adam':
        for i, (p, off, n) in enumerate(rows):
            state[i] = {'step': torch.tensor(step), 'exp_avg': opt.m[off:off + n].view(p.shape).detach().cpu().clone(),
                        'exp_avg_sq': opt.v[off:off + n].view(p.shape).detach().cpu().clone()}
        group = {'lr': float(opt.state[1].item()), 'initial_lr': float(opt.initial_lr), 'betas': tuple(opt.betas),
                 'eps': opt.eps, 'weight_decay': opt.wd, 'amsgrad': False, 'maximize': False, 'foreach': None,
                 'capturable': False, 'differentiable': False, 'fused': None, 'params': list(range(len(rows)))}
    else:
        if opt.buf is not None and step >= 1:          # torch creates the buffers at the first step with momentum
            for i, (p, off, n) in enumerate(rows):
                state[i] = {'momentum_buffer': opt.buf[off:off + n].view(p.shape).detach().cpu().clone()}
        group = {'lr': float(opt.state[1].item()), 'initial_lr': float(opt.initial_lr), 'momentum': opt.momentum,
                 'dampening': opt.dampening, 'weight_decay': opt.wd, 'nesterov': opt.nesterov, 'maximize': False,
                 'foreach': None, 'differentiable': False, 'fused': None, 'params': list(range(len(rows)))}
    return {'state': state, 'param_groups': [group]}


def _load_group(opt, rows, sd):
    """torch.optim.Adam / SGD.state_dict() -> one flat optimizer over the table rows `rows` (arenas outside the rows,
    which other groups may share, are left alone)."""
    g = sd['param_groups'][0]
    if _kind(sd) != opt.kind:
        raise ValueError('optimizer state of kind %s cannot load into a %s optimizer' % (_kind(sd), opt.kind))
    if len(g['params']) != len(rows):
        raise ValueError('optimizer state has %d parameters, the group has %d trainable ones' % (len(g['params']), len(rows)))
    with torch.no_grad():
        if opt.kind == 'adam':
            opt.set_hyper(betas=g['betas'], eps=g['eps'], weight_decay=g['weight_decay'])
            steps = set()
            for i, (p, off, n) in enumerate(rows):
                st = sd['state'].get(i)
                m, v = opt.m[off:off + n], opt.v[off:off + n]
                if st is None:
                    m.zero_()
                    v.zero_()
                    continue
                m.copy_(st['exp_avg'].reshape(-1).to(m.device))
                v.copy_(st['exp_avg_sq'].reshape(-1).to(v.device))
                steps.add(float(st['step']))
            if len(steps) > 1:
                raise ValueError('per-parameter step counts differ; the flat Adam keeps one')
            t = steps.pop() if steps else 0.0
            vec = [t, g['lr'], 1.0 - opt.betas[0] ** t, 1.0 - opt.betas[1] ** t]
        else:
            # momentum and friends are kernel arguments: set_hyper bumps hyper_version (a graph-mode Trainer re-captures)
            opt.set_hyper(momentum=g['momentum'], dampening=g['dampening'], weight_decay=g['weight_decay'],
                          nesterov=g['nesterov'])
            seen = False
            for i, (p, off, n) in enumerate(rows):
                st = sd['state'].get(i)
                b = st.get('momentum_buffer') if st is not None else None
                if opt.buf is None:
                    continue
                if b is None:
                    opt.buf[off:off + n].zero_()
                else:
                    opt.buf[off:off + n].copy_(b.reshape(-1).to(opt.buf.device))
                    seen = True
            vec = [1.0 if seen else 0.0, g['lr'], 1.0]        # step >= 1: the next update takes the running rule
        opt.lr = float(g['lr'])
        opt.initial_lr = float(g.get('initial_lr', g['lr']))
        opt.state.copy_(torch.tensor(vec))


def _groups(trainer):
    opts = getattr(trainer, 'optimizers', None) or [trainer.opt]
    rows = getattr(trainer, 'group_rows', None) or [list(range(len(trainer.table)))]
    return opts, [[trainer.table[i] for i in r] for r in rows]


def optimizer_state_dicts(trainer):
    """A Trainer's optimizer part of the checkpoint: [adam_state_dict] for the single-group Adam, else one torch state
    dict per learning-rate group (the reference's list of optimizers, base group first)."""
    opts, rows = _groups(trainer)
    if len(opts) == 1 and opts[0].kind == 'adam':
        return [adam_state_dict(trainer)]
    return [_group_state_dict(o, r) for o, r in zip(opts, rows)]


def load_optimizer_state_dicts(trainer, sds):
    """The inverse of optimizer_state_dicts; consumes the dicts it loads from the list `sds`.  Several groups take their
    dicts by parameter count, as the reference's resume does (checkpoints.py:85-99)."""
    opts, rows = _groups(trainer)
    if not sds:
        raise ValueError('the checkpoint holds no optimizer state')
    if len(opts) == 1:
        sd = sds.pop(0)
        if _kind(sd) != opts[0].kind:
            raise ValueError('optimizer state of kind %s cannot load into a %s optimizer' % (_kind(sd), opts[0].kind))
        if opts[0].kind == 'adam':
            load_adam_state_dict(trainer, sd)
        else:
            _load_group(opts[0], rows[0], sd)
        return
    for k, (o, r) in enumerate(zip(opts, rows)):
        match = next((sd for sd in sds if len(sd['param_groups'][0]['params']) == len(r)), None)
        if match is None:
            raise ValueError('no optimizer state in the checkpoint has the %d parameters of learning-rate group %d' %
                             (len(r), k))
        _load_group(o, r, match)
        sds.remove(match)


def save_checkpoint(epoch, save_folder, model, optimizer, **kwargs):
    """`optimizer`: a train.Trainer (flat Adam / SGD, one state dict per learning-rate group) or any torch optimizer /
    list of them (reference signature)."""
    opts = optimizer if isinstance(optimizer, list) else [optimizer]
    if any(getattr(o, '_ema_swapped', False) for o in opts):
        raise RuntimeError('save_checkpoint inside ema_weights(): the model holds the averaged weights')
    os.makedirs(save_folder, exist_ok=True)
    path = osp.join(save_folder, 'epoch_{}_state.pth'.format(epoch))
    sd = {k: v.detach().cpu() for k, v in _strip_module(model.state_dict()).items()}
    osd = []
    for o in opts:
        osd.extend(optimizer_state_dicts(o) if hasattr(o, 'table') else [o.state_dict()])
    ckpt = {'begin_epoch': epoch, 'state_dict': sd, 'optimizer': osd}
    dyn = [o for o in opts if getattr(o, 'dynamic_scale', False)]
    if dyn:
        ckpt['loss_scaler'] = dyn[0].scaler_state_dict()
    acc = [o for o in opts if getattr(o, 'accum_steps', 1) > 1]
    if acc:
        ckpt['grad_accum'] = acc[0].accum_state_dict()
    ema = [o for o in opts if getattr(o, 'ema', None) is not None]
    if ema:
        ckpt['ema'] = ema[0].ema_state_dict()
    from .train import frozen_batchnorm_names
    frozen = [k[7:] if k.startswith('module.') else k for k in frozen_batchnorm_names(model)]
    if frozen:
        ckpt['frozen_bn'] = frozen
    torch.save(ckpt, path)
    return path


def resume(model, optimizer, checkpoint_file, **kwargs):
    ckpt = torch.load(checkpoint_file, map_location='cpu')
    begin_epoch = ckpt['begin_epoch'] + 1
    opts = optimizer if isinstance(optimizer, list) else [optimizer]
    if 'grad_accum' in ckpt:          # checked before anything is loaded: a refused resume leaves model and trainer as they were
        for o in opts:
            if hasattr(o, 'table') and int(ckpt['grad_accum']['steps']) != getattr(o, 'accum_steps', 1):
                raise ValueError('the checkpoint was written with accum_steps=%d, this Trainer has accum_steps=%d' %
                                 (int(ckpt['grad_accum']['steps']), getattr(o, 'accum_steps', 1)))
    if 'ema' in ckpt:                 # likewise: names and shapes are checked before the model is touched
        for o in opts:
            if getattr(o, 'ema', None) is not None:
                o.check_ema_state_dict(ckpt['ema'])
    if 'frozen_bn' in ckpt:           # likewise: a run with another frozen set is another run
        from .train import frozen_batchnorm_names
        own = [k[7:] if k.startswith('module.') else k for k in frozen_batchnorm_names(model)]
        if list(ckpt['frozen_bn']) != own:
            raise ValueError('the checkpoint was written with frozen_bn=%r, this model has frozen_bn=%r' %
                             (list(ckpt['frozen_bn']), own))
    sd = _strip_module(ckpt['state_dict'])
    sd = {(k[7:] if k.startswith('preact.') else k): v for k, v in sd.items()}
    with torch.no_grad():
        own = model.state_dict()
        missing = [k for k in own if k not in sd]
        extra = [k for k in sd if k not in own]
        if missing or extra:
            raise RuntimeError('state_dict mismatch: missing %s unexpected %s' % (missing[:5], extra[:5]))
        for k, v in sd.items():          # in place: parameters may be views into the trainer's flat arena
            own[k].copy_(v.to(own[k].device))
    osds = list(ckpt['optimizer'])
    for o in opts:
        if not osds:
            break
        if hasattr(o, 'table'):
            load_optimizer_state_dicts(o, osds)
        else:
            o.load_state_dict(osds.pop(0))
    if 'loss_scaler' in ckpt:
        for o in opts:
            if getattr(o, 'dynamic_scale', False):
                o.load_scaler_state_dict(ckpt['loss_scaler'])
    for o in opts:
        if getattr(o, 'accum_steps', 1) > 1:
            if 'grad_accum' in ckpt:
                o.load_accum_state_dict(ckpt['grad_accum'])
            else:
                o.reset_window()
    for o in opts:
        if getattr(o, 'ema', None) is not None:
            if 'ema' in ckpt:
                o.load_ema_state_dict(ckpt['ema'])
            else:
                o.reset_ema()          # the parameters were just overwritten in place: the average restarts from them
    return model, optimizer, begin_epoch
