"""A record of everything an Engine enqueues -- every library launch, every event record, every stream wait -- in a form two
source trees can be compared by.  tests/_launch_log.py pins the Trainer's launches around the gradient computation; this
module pins the gradient computation itself: which entry points, with which arguments and buffers, on which stream lane,
ordered by which events.

The recorder depends only on what every tree has: `lib().call` / `lib().call_routed` (wrapped on the instance; Engine.call,
acall, flush_reduces and the running-statistics batch all pass through them), `torch.cuda.Event.record` and
`torch.cuda.Stream.wait_event` (Python-level methods, wrapped on the class; wait_stream / record_event pass through them),
and `Engine.__init__` (wrapped on the class to mark where an Engine's rows begin, to read its `nfused` counters and to hold
its `_keep` list until the call is over).  All four are restored when the recording ends.

One row is
* ['<entry point>', [arguments], stream]: integers exactly, floats as float.hex(), pointers by name (below), the stream (the
  last argument of an entry point whose prototype ends in fami_stream_t) apart;
* ['record', event, stream]: every Event.record takes the next event number of the case and leaves it on the event object;
* ['wait', stream, event]: 'unrecorded' for an event recorded before the case began.
A stream is the ordinal of the first appearance of its handle within the CASE.

A pointer is `name+byte offset` into a named tensor of the Trainer (tests/_launch_log.py), 'NULL', or the ordinal of the
first appearance of its value within the step() call.  The Engine keeps every buffer of a step alive in `_keep`, and the
recorder keeps the `_keep` lists of a call's Engines (a capture's warm-up runs) until the call returns, so distinct buffers
have distinct addresses within a call.  Pointer-valued words of host arrays handed to an entry point -- the pointer arrays
of fami_fuse_sum / fami_concat_channels / fami_split_channels, `ptrs` of fami_add_batch_f32 and
fami_bn_running_update_batch_f32, the two pointers heading each descriptor of fami_wgrad_reduce_batch -- go through the
same map, so the record shows which buffer pairs with which; a descriptor buffer the library fills after the call
(`desc_out`) is 'desc'.  Known property: a tree that frees a temporary earlier or later (a buffer outside `_keep`) can
change these ordinals without changing the work.  That is a false failure, never a false pass.

What a case starts from is set by `fresh_case`: Engine._zero_arenas emptied (the arena is sized by the steps before), the
class-level stream pools emptied and torch's shared capture stream dropped.  torch hands streams out of a 32-entry
round-robin pool, so whether a Trainer's warm-up or capture stream IS a cached lane stream -- and the re-pick loops of the
Engine then choose others -- depends on how many streams the process has made before; with the pools empty every stream of
a case is a fresh consecutive draw, and the ordinals do not depend on which tests ran first.

A full record is some thousands of rows per call; `summary` keeps the row count, the count per row name and a sha256 per
block of 64 rows.  `python tests/_engine_log.py --dump DIR` writes the full records as text, one row per line, one file per
case: run it in two checkouts and diff."""
import contextlib
import ctypes
import functools
import hashlib
import json
import os
import sys

import torch

from _launch_log import _spans, _symbol, _with_stream

S, H, W, B = 2, 160, 288, 2     # image 288 wide x 160 high, heatmap 72 x 40 (tests/test_engine_launches_gpu.py says why)
BLOCK = 64

# key -> (compute mode, deterministic, use_graph, environment, Trainer options)
CASES = {
    'f32': (None, False, False, {}, {}),
    'bf16': ('bf16', False, False, {}, {}),
    'f32-det': (None, True, False, {}, {}),
    'f16-det': ('f16', True, False, {}, {}),
    'bf16-fuse-bn': ('bf16', False, False, {'FAMI_FUSE_BN': '1'}, {}),
    'f32-no-fuse-no-xbn': (None, False, False, {'FAMI_FUSE_BN': '0', 'FAMI_XBN': '0'}, {}),
    'bf16-no-lanes': ('bf16', False, False, {'FAMI_LANES': '0'}, {}),
    'bf16-two-predictors': ('bf16', False, False, {'FAMI_MERGE_PREDICTORS': '0'}, {}),
    'f32-frozen-bn': (None, False, False, {}, {'frozen_bn': 'all'}),
    'bf16-no-bn-in': ('bf16', False, False, {'FAMI_BN_IN': '0'}, {}),
    'f32-graph': (None, False, True, {}, {}),
    'bf16-graph': ('bf16', False, True, {}, {}),
}
INFERENCE = {'infer-f32': None, 'infer-bf16': 'bf16'}
# the data-parallel plans with one rank (tests/_ddp_single_rank_engine_launches.py): the 'bf16' case under each
DDP_PLANS = {'ddp-overlap-bf16': {'FAMI_DDP_PLAN': 'overlap'}, 'ddp-eager-hooks-bf16': {'FAMI_DDP_GRAPH': '0'}}

# host arrays of longs whose every word is a pointer
_LONG_POINTERS = ('fami_add_batch_f32', 'fami_bn_running_update_batch_f32')
_DESC_POINTERS = 2            # struct ReduceDesc (csrc/conv.hip): part, dw, then eight ints


class Recorder:
    def __init__(self, spans_of):
        self.spans_of = spans_of      # () -> the named spans, asked per launch (a Trainer creates tensors as it goes)
        self.rows, self.marks = [], []
        self.nfused = None            # the counters of the Engine created last
        self.streams, self.pointers, self.events = {}, {}, 0
        self.held = []

    def stream(self, handle):
        return self.streams.setdefault(int(handle or 0), len(self.streams))

    def pointer(self, spans, p):
        name = _symbol(spans, p)
        return self.pointers.setdefault(p, len(self.pointers)) if name == '?' else name

    def drain(self):
        """-> (rows of the call that just ended, the row index at which each of its Engines was created)"""
        out = (self.rows, self.marks)
        self.rows, self.marks, self.pointers, self.held = [], [], {}, []
        return out


@contextlib.contextmanager
def recording(spans_of=lambda: []):
    from fami_pose_amd._lib import lib
    from fami_pose_amd.engine import Engine
    L, rec, streamed = lib(), Recorder(spans_of), _with_stream()
    reduce_longs = L.cdll.fami_wgrad_reduce_desc_longs()

    def array(name, spans, a):
        kind = a._type_
        if kind is ctypes.c_void_p:
            return [rec.pointer(spans, v) for v in a]
        if kind is ctypes.c_int:
            return [int(v) for v in a]
        if kind is ctypes.c_float:
            return [float(v).hex() for v in a]
        assert kind is ctypes.c_long, (name, kind)
        if name == 'fami_wgrad_reduce_batch':
            return [rec.pointer(spans, v) if i % reduce_longs < _DESC_POINTERS else int(v) for i, v in enumerate(a)]
        if name in _LONG_POINTERS:
            return [rec.pointer(spans, v) for v in a]
        assert len(a) == reduce_longs, name      # desc_out: one descriptor, filled by the library after the call
        return 'desc'

    def note(name, args):
        spans, types, out = rec.spans_of(), L.protos[name][1], []
        assert len(types) == len(args), name
        stream = None
        if name in streamed:
            stream = rec.stream(args[-1])
            args, types = args[:-1], types[:-1]
        for a, t in zip(args, types):
            if isinstance(a, ctypes.Array):
                out.append(array(name, spans, a))
            elif t is ctypes.c_void_p:
                out.append(rec.pointer(spans, a))
            elif t in (ctypes.c_float, ctypes.c_double):
                out.append(float(a).hex())
            else:
                out.append(int(a))
        rec.rows.append([name, out, stream])

    token = object()
    call, call_routed = L.call, L.call_routed
    ev_record, wait_event, init = torch.cuda.Event.record, torch.cuda.Stream.wait_event, Engine.__init__

    def record(self, stream=None):
        st = torch.cuda.current_stream() if stream is None else stream
        self._engine_log = (token, rec.events)
        rec.rows.append(['record', rec.events, rec.stream(st.cuda_stream)])
        rec.events += 1
        return ev_record(self, stream)

    def wait(self, event):
        seen = getattr(event, '_engine_log', None)
        rec.rows.append(['wait', rec.stream(self.cuda_stream), seen[1] if seen is not None and seen[0] is token else 'unrecorded'])
        return wait_event(self, event)

    @functools.wraps(init)
    def engine_init(self, *a, **kw):
        rec.marks.append(len(rec.rows))
        init(self, *a, **kw)
        rec.nfused = self.nfused
        rec.held.append(getattr(self, '_keep', None))

    L.call = lambda name, *a: (note(name, a), call(name, *a))[1]
    L.call_routed = lambda route, name, *a: (note(name, a), call_routed(route, name, *a))[1]
    torch.cuda.Event.record, torch.cuda.Stream.wait_event, Engine.__init__ = record, wait, engine_init
    try:
        yield rec
    finally:
        del L.call, L.call_routed
        torch.cuda.Event.record, torch.cuda.Stream.wait_event, Engine.__init__ = ev_record, wait_event, init


def fresh_case():
    """what a case starts from (the module docstring says why)"""
    from fami_pose_amd.engine import Engine
    Engine._zero_arenas.clear()
    Engine._side_pool.clear()
    Engine._wgrad_pool.clear()
    if getattr(torch.cuda.graph, 'default_capture_stream', None) is not None:
        torch.cuda.graph.default_capture_stream = None


@functools.lru_cache(None)
def _state():
    from oracle import model as om
    return om.realistic_init_(om.AlignmentOracle(om.make_cfg(48), True, S, (H, W)), 5).state_dict()


def model(dev, mode):
    import fami_pose_amd as fp
    m = fp.build_model(fp.default_cfg(48, image_size=(W, H), num_sup=S), 'train')
    m.load_state_dict(_state())
    m = m.to(dev)
    return m if mode is None else m.set_compute_dtype(mode)


def batch(dev, seed=9):
    gen = torch.Generator().manual_seed(seed)
    kf, sup = torch.randn(B, 3, H, W, generator=gen), torch.randn(B, 3 * S, H, W, generator=gen)
    joints = torch.rand(B, 17, 2, generator=gen) * torch.tensor([W, H], dtype=torch.float32)
    vis = (torch.rand(B, 17, generator=gen) < 0.8).float()
    return tuple(t.to(dev) for t in (kf, sup, joints, vis))


def record_trainer(dev, key, graph=None, cases=CASES, **kw):
    """-> ([(rows, marks) of the first two step() calls of a fresh Trainer], its last Engine's counters, which are the Trainer's
    last_nfused); the environment of the case has been set by the caller.  cases: the table `key` is looked up in."""
    from fami_pose_amd.train import Trainer
    mode, det, use_graph, _, opts = cases[key]
    fresh_case()
    m = model(dev, mode)
    if det:
        m.set_deterministic(True)
    tr = Trainer(m, use_graph=use_graph if graph is None else graph, targets_from_joints=True, **opts, **kw)
    bt, calls = batch(dev), []
    with recording(lambda: _spans(tr)) as rec:
        for _ in range(2):
            tr.step(*bt)
            calls.append(rec.drain())
    torch.cuda.synchronize(dev)
    assert tr.last_nfused == rec.nfused
    return calls, dict(rec.nfused)


def record_inference(dev, key):
    """two forwards of the frozen model in eval mode through runtime.EngineModule (an Engine with record=False each)"""
    fresh_case()
    m = model(dev, INFERENCE[key]).eval().requires_grad_(False)
    kf, sup = batch(dev)[:2]
    calls = []
    with recording() as rec, torch.no_grad():
        for _ in range(2):
            m(kf, sup)
            calls.append(rec.drain())
    torch.cuda.synchronize(dev)
    return calls, dict(rec.nfused)


def digest(rows):
    return hashlib.sha256(json.dumps(rows, sort_keys=True, separators=(',', ':')).encode()).hexdigest()


def summary(calls, counters):
    out = []
    for rows, marks in calls:
        names = {}
        for r in rows:
            names[r[0]] = names.get(r[0], 0) + 1
        out.append({'rows': len(rows), 'engines': marks, 'names': names,
                    'blocks': [digest(rows[i:i + BLOCK]) for i in range(0, len(rows), BLOCK)]})
    return {'image': [W, H], 'counters': counters, 'calls': out}


@contextlib.contextmanager
def environment(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _dump(dev, out):
    import gc
    os.makedirs(out, exist_ok=True)
    for key in list(CASES) + list(INFERENCE):
        with environment(CASES[key][3] if key in CASES else {}):
            calls = (record_trainer(dev, key) if key in CASES else record_inference(dev, key))[0]
        with open(os.path.join(out, key + '.txt'), 'w') as f:
            for k, (rows, marks) in enumerate(calls):
                f.write('# call %d: %d rows, engines at %s\n' % (k, len(rows), marks))
                f.writelines(json.dumps(r) + '\n' for r in rows)
        gc.collect()
        torch.cuda.synchronize(dev)
        gc.collect()
        print('wrote', key, flush=True)


if __name__ == '__main__':
    os.environ.setdefault('HIP_FORCE_DEV_KERNARG', '1')
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert len(sys.argv) == 3 and sys.argv[1] == '--dump', 'usage: python tests/_engine_log.py --dump DIR'
    _dump(torch.device('cuda:0'), sys.argv[2])
