"""A record of the library launches a Trainer.step() call makes, in a form two source trees can be compared by.

The recorder depends only on what every tree has: `lib().call` and `lib().call_routed` (every launch of the project goes
through one of the two; Engine.call does too), wrapped on the instance, and `trainer._forward_backward`, wrapped on the
instance to tell inside from outside.  Kept: every call made outside `_forward_backward`, and of the calls made inside it
only the optimizer launches (`fami_adam_*` / `fami_sgd_*`: the in-backward split).

One record is [name, [arguments], stream, capturing]:
* integers exactly, floats as float.hex();
* pointers as symbols: `name+byte offset` for a pointer into a named tensor of the Trainer, 'NULL', or '?';
* the stream (the last argument of an entry point whose prototype ends in fami_stream_t) as 'current' or 'other', by
  comparison with torch.cuda.current_stream(dev) at the moment of the call;
* whether torch.cuda.is_current_stream_capturing() was true.

CONFIGS holds the ten Trainer configurations of tests/test_train_launches_gpu.py; its data-parallel child
(tests/_ddp_single_rank_launches.py) builds three of them from the same table."""
import contextlib
import ctypes
import re

import torch

HRNET = [(('hrnet',), 1e-5)]
# number -> (compute mode, Trainer options)
CONFIGS = {
    1: (None, {}),
    2: (None, dict(lr_groups=HRNET)),
    3: (None, dict(optimizer='sgd', lr=0.01, momentum=0.9)),
    4: ('f16', {}),
    5: (None, dict(max_grad_norm=1.0)),
    6: ('f16', dict(loss_scale='dynamic')),
    7: ('f16', dict(max_grad_norm=1.0, loss_scale='dynamic', ema_decay=0.5, lr_groups=HRNET)),
    8: (None, dict(accum_steps=2)),
    9: ('f16', dict(accum_steps=2, max_grad_norm=1.0, ema_decay=0.5)),
    10: (None, dict(ema_decay=0.5)),
}
NAMED = ('flat', 'grad', 'accum', 'ema', 'ema_state', 'overflow', 'clip', '_partials', 'scaler_state', '_group_flags',
         'loss_parts', '_window_loss', 'integral_loss', 'structure_loss')
# (`acc` stays unnamed: the cases of tests/golden/engine_launches.json were recorded with it as an ordinal)
HEAD_BUFFERS = ('sel_w', 'coords', 'stats', 'txy', 'gcoords', 'tw')      # per batch shape: `coords[2x17]`
INSIDE = ('fami_adam_', 'fami_sgd_')


def _with_stream():
    """the entry points whose last parameter is a fami_stream_t (include/fami.h)"""
    from fami_pose_amd._lib import HEADER_PATH
    src = re.sub(r'/\*.*?\*/', ' ', open(HEADER_PATH).read(), flags=re.S)
    return {m.group(1) for m in re.finditer(r'\b(fami_\w+)\s*\(([^;{]*?)\)\s*;', src, flags=re.S)
            if m.group(2).split(',')[-1].split()[:1] == ['fami_stream_t']}


def _head_named(tr):
    """[(symbol, tensor)] of the supervision head's private tensors, under one set of symbols on both kinds of tree: one whose
    Trainer owns a head object (`tr.head`: joint weights, limb pairs, the scalar terms' window sums, one record of buffers per
    batch shape), and the tree the head fixtures were recorded on, which keeps the same tensors on the Trainer itself"""
    head = getattr(tr, 'head', None)
    if head is not None:
        named = [('_joint_w', head.joint_w), ('_pairs_dev', head.pairs_dev)] + [('_window_' + t.name, t.window) for t in head.terms]
        for (B, J), r in head.bufs.items():
            named += [('%s[%dx%d]' % (k, B, J), getattr(r, k)) for k in HEAD_BUFFERS]
        return named
    named = [(k, getattr(tr, k, None)) for k in ('_joint_w', '_pairs_dev', '_window_integral', '_window_structure')]
    for attr, fields in (('_sel_w', ('sel_w',)), ('_int_bufs', ('coords', 'stats', 'txy')), ('_struct_bufs', ('gcoords', 'tw'))):
        for (B, J), ts in getattr(tr, attr, {}).items():
            named += [('%s[%dx%d]' % (k, B, J), t) for k, t in zip(fields, ts if isinstance(ts, tuple) else (ts,))]
    return named


def _spans(tr):
    """[(symbol, first byte, one past the last)] of the Trainer's named tensors, in lookup order"""
    named = [(k, getattr(tr, k, None)) for k in NAMED] + _head_named(tr)
    for i, o in enumerate(tr.optimizers):
        named += [('opt%d.%s' % (i, k), getattr(o, k, None)) for k in ('m', 'v', 'buf', 'state')]
    return [(k, t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for k, t in named if torch.is_tensor(t)]


def _symbol(spans, ptr):
    if not ptr:
        return 'NULL'
    for k, lo, hi in spans:
        if lo <= ptr < hi:
            return '%s+%d' % (k, ptr - lo)
    return '?'


@contextlib.contextmanager
def recording(tr):
    """-> a list that receives the records of everything `tr` launches inside the block (take them with `drain`)."""
    from fami_pose_amd._lib import lib
    L, log, depth, streamed = lib(), [], [0], _with_stream()

    def note(name, args):
        if depth[0] and not name.startswith(INSIDE):
            return
        spans, types, out = _spans(tr), L.protos[name][1], []
        assert len(types) == len(args), name
        stream = None
        if name in streamed:
            stream = 'current' if (args[-1] or 0) == torch.cuda.current_stream(tr.dev).cuda_stream else 'other'
            args, types = args[:-1], types[:-1]
        for a, t in zip(args, types):
            if t is ctypes.c_void_p:
                out.append(_symbol(spans, a))
            elif t in (ctypes.c_float, ctypes.c_double):
                out.append(float(a).hex())
            else:
                out.append(int(a))
        log.append([name, out, stream, bool(torch.cuda.is_current_stream_capturing())])

    call, call_routed, fb = L.call, L.call_routed, tr._forward_backward

    def inside(*a, **kw):
        depth[0] += 1
        try:
            return fb(*a, **kw)
        finally:
            depth[0] -= 1

    L.call = lambda name, *a: (note(name, a), call(name, *a))[1]
    L.call_routed = lambda route, name, *a: (note(name, a), call_routed(route, name, *a))[1]
    tr._forward_backward = inside
    try:
        yield log
    finally:
        del L.call, L.call_routed, tr._forward_backward


def drain(log):
    out = list(log)
    del log[:]
    return out


def record_steps(tr, batch):
    """the records of the first accum_steps + 1 step() calls of a fresh Trainer, one list per call"""
    out = []
    with recording(tr) as log:
        for _ in range(tr.accum_steps + 1):
            tr.step(*batch)
            out.append(drain(log))
    torch.cuda.synchronize(tr.dev)
    return out
