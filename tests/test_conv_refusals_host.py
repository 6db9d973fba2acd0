"""Every refusal the fami_conv2d_* entry points can reach BEFORE any HIP call, on a machine without a GPU: the return code and
the exact fami_last_error() text of each, against tests/golden/conv_refusals.json (recorded from the library of the commit
named inside the file with tools/gen_conv_refusals_golden.py, which runs this module's table).

A case is an entry point, the argument vector of a call that would be accepted (built from the parameter names of
include/fami.h: one dummy non-null address for every required tensor, N = 1, 8 x 8, 16 -> 16 channels, 3 x 3, stride 1, pad 1)
and ONE thing wrong with it.  The accepted vector itself is never called.  Read against csrc/conv.hip, no case reaches a launch:
  - forward and input gradient check pointers, geometry, the 16-bit statistics shapes and the 2 GiB limits before any route;
  - the weight gradients check theirs behind the routes, so their cases are the ones every route declines first: a null tensor
    (each route asks for all four), kernel size 8 / stride 3 / dilation 0 (the plans of conv_wg16.hip / conv_wgs3.hip take k = 1 | 3,
    stride 1 | 2, pad == dil * (k - 1) / 2), and the 2 GiB case on a 5 x 5 kernel (no staged route takes 5 x 5; the per-tap plan's
    workspace figure is passed, so the size check is reached); fami_conv2d_wgrad_defer_xbn_* has a fixed 3 x 3 geometry whose
    routes come before the size check: no 2 GiB case for it;
  - fami_conv2d_bwd_pair_* runs its input gradient first: only refusals of the entry point itself and of that input gradient.
Codes: -1 bad argument, -2 unsupported shape.  -3 (a HIP error) would mean a case reached the runtime: refused by the test."""
import ctypes
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'conv_refusals.json')
TYPES = ['f32', 'bf16', 'f16']
HUGE_N = 1 << 21          # N * 8 * 8 * 16 channels: 2^32 bytes in 16-bit storage, 2^33 in fp32; 2^27 pixels (below the 2^31 pixel limit)

# values of an accepted call, by parameter name (pointers not listed: one dummy non-null address; OPTIONAL ones: null)
SCALARS = dict(N=1, H=8, W=8, Ci=16, Co=16, kh=3, kw=3, stride=1, pad=1, dil=1, relu=0, accumulate=0, out_f32=0, acc_dx=0, acc_dw=0,
               ws_bytes=1 << 30, xP=64, xmomentum=0.1, xeps=1e-5, stream=None)
OPTIONAL = {'bias', 'addend', 'pivot_src', 'xrunning_mean', 'xrunning_var'}
PAIR_OPTIONAL = {'z', 'yrelu', 'mean', 'invstd', 'gamma', 'beta', 'slots', 'xmean', 'xinvstd', 'xgamma', 'xbeta'}      # (of fami_conv2d_bwd_pair_*)
BNIN_SHAPE = dict(N=20, H=96, W=72, Ci=48, Co=48)          # the layer-1 shape of the W48 backbone: fami_conv2d_fwd_bnin_ok takes it


def prototypes():
    """{name: [(parameter, is_pointer)]} of the fami_conv2d_* compute entry points, from include/fami.h"""
    src = re.sub(r'/\*.*?\*/', ' ', open(os.path.join(ROOT, 'include', 'fami.h')).read(), flags=re.S)
    out = {}
    for m in re.finditer(r'\bint\s+(fami_conv2d_(?:fwd|fwd_stats|fwd_xbn|fwd_bnin|dgrad|dgrad_bnstats|wgrad|wgrad_defer|wgrad_defer_xbn|bwd_pair)'
                         r'_(?:f32|bf16|f16))\s*\(([^;{]*?)\)\s*;', src, flags=re.S):
        out[m.group(1)] = [(a.split()[-1].lstrip('*'), '*' in a) for a in (p.strip() for p in m.group(2).split(','))]
    return out


def table():
    """[(case id, entry point, {parameter: value} overrides of the accepted call)]"""
    cases = []
    for name, params in sorted(prototypes().items()):
        kind, dt = re.match(r'fami_conv2d_(\w+)_(f32|bf16|f16)$', name).groups()
        names = [p for p, _ in params]
        add = lambda what, **ov: cases.append(('%s[%s]' % (name, what), name, ov))
        pair, wgrad = kind == 'bwd_pair', kind.startswith('wgrad')
        shape = BNIN_SHAPE if kind == 'fwd_bnin' else {}
        # the tensors the first check of the call's own path asks for, null in turn
        first = {'fwd': ['x', 'wp', 'y'], 'fwd_stats': ['x', 'wp', 'y'], 'fwd_xbn': ['z', 'wp', 'y'], 'fwd_bnin': ['z', 'wp', 'y'],
                 'dgrad': ['dy', 'wp', 'dx'], 'dgrad_bnstats': ['dy', 'wp', 'dx'], 'wgrad': ['x', 'dy', 'dw', 'workspace'],
                 'wgrad_defer': ['x', 'dy', 'dw', 'workspace'], 'wgrad_defer_xbn': ['z', 'dy', 'dw', 'workspace'],
                 'bwd_pair': ['dy', 'wpd', 'dx']}[kind]
        for p in first:
            add('null ' + p, **{p: None}, **shape)
        # arguments the entry point itself requires
        if 'desc_out' in names:
            add('null desc_out', desc_out=None)
        if kind == 'fwd_stats':
            add('null slots', slots=None)
        if kind in ('fwd_xbn', 'fwd_bnin'):
            for p in ['xslots', 'xgamma', 'xbeta', 'xmean', 'xinvstd'] + (['a_out'] if kind == 'fwd_bnin' else []):
                add('null ' + p, **{p: None}, **shape)
            add('xP 0', xP=0, **shape)
        if kind == 'fwd_bnin':
            add('shape fami_conv2d_fwd_bnin_ok rejects')          # (the 8 x 8, 16 -> 16 call)
        if kind == 'wgrad_defer_xbn' or (pair and dt == 'f32'):
            on = dict(xmean='ptr') if pair else {}
            for p in ['xmean', 'xinvstd', 'xgamma', 'xbeta'][1 if pair else 0:]:
                add('null ' + p, **dict(on, **{p: None}))
        if kind == 'dgrad_bnstats' or (pair and dt != 'f32'):
            on = dict(slots='ptr', z='ptr', yrelu='ptr', mean='ptr', invstd='ptr', gamma='ptr', beta='ptr') if pair else {}
            for p in ['z', 'mean', 'invstd', 'gamma', 'beta'] + ([] if pair else ['slots']):
                add('statistics, null ' + p, **dict(on, **{p: None}))
            add('relu 3', **dict(on, relu=3))
            add('relu -1', **dict(on, relu=-1))
            add('relu 1 without yrelu', **dict(on, relu=1, yrelu=None))
        # geometry
        if 'kh' in names:
            add('kernel size 8', kh=8, kw=8)
            add('stride 3', stride=3)
            add('dilation 0', dil=0)
            if wgrad:
                add('tensor >= 2 GiB', N=HUGE_N, kh=5, kw=5, pad=2, ws_bytes='workspace')
            else:
                add('tensor >= 2 GiB', N=HUGE_N)
        elif kind == 'fwd_xbn':
            add('tensor >= 2 GiB', N=HUGE_N)
        # 16-bit statistics epilogues: channel counts that are no multiple of 4, a ReLU / fp32 output with statistics
        if dt != 'f32':
            if kind in ('fwd_stats', 'fwd_xbn'):
                add('statistics with Co % 4', Co=18)
            if kind == 'dgrad_bnstats':
                add('statistics with Ci % 4', Ci=18)
            if pair:
                add('statistics with Ci % 4', slots='ptr', z='ptr', yrelu='ptr', mean='ptr', invstd='ptr', gamma='ptr', beta='ptr', Ci=18)
    return cases


def run(L, cases=None):
    """-> {case id: [return code, fami_last_error() text]}.  L: fami_pose_amd._lib.lib()"""
    protos = prototypes()
    buf = ctypes.create_string_buffer(8192)
    dummy = (ctypes.addressof(buf) + 4095) & ~4095          # page-aligned, inside the buffer: nothing may read or write it anyway
    desc = (ctypes.c_long * 64)()
    out = {}
    for cid, name, ov in cases or table():
        pair = '_bwd_pair_' in name
        args = []
        for p, is_ptr in protos[name]:
            if p in ov:
                v = ov[p]
                if v == 'ptr':
                    v = dummy
                elif v == 'workspace':
                    g = {k: ov.get(k, SCALARS[k]) for k in ('N', 'H', 'W', 'Ci', 'Co', 'kh', 'kw', 'stride', 'pad', 'dil')}
                    v = L.cdll.fami_conv2d_wgrad_workspace(*g.values())
                    assert v > 0
            elif is_ptr:
                v = None if (p in OPTIONAL or (pair and p in PAIR_OPTIONAL)) else (desc if p == 'desc_out' else dummy)
            else:
                v = SCALARS[p]
            args.append(v)
        L.bind(None)
        rc = getattr(L.cdll, name)(*args)
        out[cid] = [rc, L.cdll.fami_last_error().decode()]
    return out


def test_the_table_covers_every_entry_point_and_refusal_kind():
    protos, cases = prototypes(), table()
    assert len(protos) == 29          # 9 f32 (no fwd_bnin) + 10 bf16 + 10 f16
    assert {n for _, n, _ in cases} == set(protos)
    ids = [c for c, _, _ in cases]
    assert len(ids) == len(set(ids))
    for what in ('null x]', 'kernel size 8', 'stride 3', 'dilation 0', 'tensor >= 2 GiB', 'Co % 4', 'Ci % 4', 'null slots', 'relu 3',
                 'relu 1 without yrelu', 'null desc_out', 'null xslots', 'xP 0', 'fami_conv2d_fwd_bnin_ok rejects'):
        assert any(what in c for c in ids), what
    for _, name, ov in cases:          # a pair call never leaves its input gradient acceptable
        if '_bwd_pair_' in name:
            assert ov and 'x' not in ov and 'dw' not in ov and 'workspace' not in ov, ov


def test_every_refusal_keeps_its_code_and_text():
    from fami_pose_amd._lib import lib
    L = lib()
    L.cdll.fami_tune_reset()
    gold = json.load(open(GOLDEN))
    assert re.fullmatch(r'[0-9a-f]{7,40}', gold['commit'])
    got = run(L)
    assert set(got) == set(gold['cases']), sorted(set(got) ^ set(gold['cases']))
    for cid, (rc, text) in got.items():
        assert rc in (-1, -2), 'case %s was not refused before the runtime: %d, %s' % (cid, rc, text)
        assert [rc, text] == gold['cases'][cid], (cid, rc, text, gold['cases'][cid])
        assert text.startswith('fami_conv2d_')
