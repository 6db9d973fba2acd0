"""The host half of csrc/align.hip on a machine without a GPU, against tests/golden/align_host.json (recorded from the library of
the commit named inside the file with tools/gen_align_host_golden.py, which runs this module's tables):

  refusals  every refusal an exported entry point of align.hip can reach BEFORE any HIP call: the return code and the exact
            fami_last_error() text.  A case is an entry point, the argument vector of a call that would be accepted (built from
            the parameter names of include/fami.h: one dummy non-null address per tensor, B = 2, 9 x 10, C = 8, G = 2, Co = 16,
            3 x 3, stride 1, pad = dil = 1) and ONE thing wrong with it.  The accepted vector itself is never called.
  queries   the size / layout queries over a table of geometries under seven settings of fami_dcn_tune, and that no query
            writes a DCN field of the route it is asked under.

Codes: -1 bad argument, -2 unsupported shape.  -3 (a HIP error) would mean a case reached the runtime: refused by the test.

Left out, because the first refusal lies behind a launch (read against csrc/align.hip):
  - fami_shift_bilinear_bwd_*: "workspace required for gt" with gsrc given (the source gradient is launched first); the case
    here passes gsrc = null;
  - fami_dcn_bwd_det_* / fami_dcn_bwd_det_om_* with gx given: the accumulator is zeroed and max|dy| taken before the arguments of
    the backward itself are looked at; their argument cases pass gx = null (the deterministic `col` layout, nothing launched
    before the checks);
  - every refusal of the HIP runtime itself (FAMI_CHECK_LAUNCH)."""
import ctypes
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'align_host.json')
TYPES = ['f32', 'bf16', 'f16']
DCN_FIELDS = ['dcn_gather', 'dcn_abl', 'dcn_win_r', 'dcn_ksplit', 'dcn_pf', 'dcn_bwd2', 'dcn_bwd2_cap', 'dcn_bwd2_stage', 'dcn_bwd_abl',
              'dcn_bwd_scatter']
DCN_DEFAULTS = [-1, 0, 0, 1, 0, 1, 36, 1, 0, -1]

SCALARS = dict(B=2, H=9, W=10, C=8, Co=16, G=2, kh=3, kw=3, stride=1, pad=1, dil=1, acc_src=0, acc_t=0, acc_off=0, acc_om=0, acc_x=0,
               elem_bytes=4, accumulate=0, stream=None)
OPTIONAL = {'bias', 'msk', 'gmsk', 'goff', 'gom', 'col', 'gsrc', 'gt'}          # null in the accepted call
FAMILIES = ['shift_bilinear_fwd', 'shift_bilinear_bwd', 'dcn_fwd', 'dcn_fwd_om', 'dcn_bwd', 'dcn_bwd_om', 'dcn_bwd_det', 'dcn_bwd_det_om']
PLAIN = ['fami_dcn_pack_weight_f32', 'fami_dcn_pack_weight_bf16', 'fami_dcn_pack_weight_f16', 'fami_dcn_pack_weight_bwd_f32',
         'fami_dcn_col_dw_unpermute_f32']
QUERIES = ['fami_dcn_packed_weight_elems', 'fami_dcn_packed_weight_bwd_elems', 'fami_dcn_bwd_col_width', 'fami_dcn_bwd_col_permuted',
           'fami_dcn_bwd_det_workspace', 'fami_shift_workspace']


def prototypes():
    """{name: [(parameter, is_pointer)]} of the exported entry points of align.hip, from include/fami.h"""
    src = re.sub(r'/\*.*?\*/', ' ', open(os.path.join(ROOT, 'include', 'fami.h')).read(), flags=re.S)
    out = {}
    for m in re.finditer(r'\b(?:int|long)\s+(fami_(?:shift|dcn)_\w+)\s*\(([^;{]*?)\)\s*;', src, flags=re.S):
        out[m.group(1)] = [(a.split()[-1].lstrip('*'), '*' in a) for a in (p.strip() for p in m.group(2).split(','))]
    return out


def refusal_table():
    """[(case id, entry point, fami_dcn_tune code or None, {parameter: value} overrides of the accepted call)]"""
    cases = []

    def add(name, what, tune=None, **ov):
        cases.append(('%s[%s]' % (name, what), name, tune, ov))

    for dt in TYPES:
        n = 'fami_shift_bilinear_fwd_' + dt
        for p in ('src', 't', 'out'):
            add(n, 'null ' + p, **{p: None})
        add(n, 'B 0', B=0)
        add(n, 'C % 4', C=6)
        n = 'fami_shift_bilinear_bwd_' + dt
        for p in ('gout', 'src', 't'):
            add(n, 'null ' + p, **{p: None})
        add(n, 'B 0', B=0)
        add(n, 'C % 4', C=6)
        add(n, 'null workspace with gt', gt='ptr', ws=None)
        for om in ('', '_om'):
            off = 'om' if om else 'off'
            n = 'fami_dcn_fwd%s_%s' % (om, dt)
            for p in ('x', off, 'wp', 'y'):
                add(n, 'null ' + p, **{p: None})
            geometry = [('B 0', dict(B=0)), ('G 0', dict(G=0)), ('C % G', dict(G=3)), ('cg % 4', dict(G=4)), ('Co > 96', dict(Co=112))]
            for what, ov in geometry:
                add(n, what, **ov)
            add(n, 'P >= 2^31', B=1 << 25)
            add(n, 'C*kh*kw too large for the LDS column tile', tune=0, C=264)
            n = 'fami_dcn_bwd%s_%s' % (om, dt)
            for p in ('x', off, 'dy', 'wpb'):
                add(n, 'null ' + p, **{p: None})
            for what, ov in geometry:
                add(n, what, **ov)
            add(n, 'frame too large', W=1 << 20)
            add(n, 'tile does not fit LDS', C=16, Co=20, pad=40, dil=40)
            n = 'fami_dcn_bwd_det%s_%s' % (om, dt)
            add(n, 'null workspace', ws=None)
            add(n, 'null dy', dy=None)
            for p in ('x', off, 'wpb'):
                add(n, 'no gx, null ' + p, gx=None, **{p: None})
            for what, ov in geometry:
                add(n, 'no gx, ' + what, gx=None, **ov)
    for n in PLAIN[:4]:
        for p in ('w_oihw', 'wpb' if 'bwd' in n else 'wp'):
            add(n, 'null ' + p, **{p: None})
        for what, ov in (('G 0', dict(G=0)), ('C % G', dict(G=3)), ('cg % 4', dict(G=4))):
            add(n, what, **ov)
    n = PLAIN[4]
    add(n, 'null dwp', dwp=None)
    add(n, 'null dw', dw=None)
    add(n, 'geometry the register-fed plan rejects', Co=20)
    add(n, 'register-fed kernel switched off', tune=2048)
    return cases


# (C, G, Co): the head's, the two geometries of tests/test_align_exact_gpu.py, the head's with other output widths
GEOMETRIES = [(48, 12, 48), (8, 2, 16), (16, 2, 20), (48, 12, 16), (48, 12, 20), (48, 12, 96)]
SETTINGS = [('default', []), ('2048', [2048]), ('512', [512]), ('514', [514]), ('1024+1', [1025]), ('4096+24', [4096 + 24]), ('4096+64', [4096 + 64])]


def query_table():
    """[(query id, entry point, argument tuple)]"""
    q = []
    for C, G, Co in GEOMETRIES:
        q.append(('fami_dcn_packed_weight_elems(Co=%d,C=%d,G=%d)' % (Co, C, G), 'fami_dcn_packed_weight_elems', (Co, C, 3, 3, G)))
        q.append(('fami_dcn_packed_weight_bwd_elems(Co=%d,C=%d,G=%d)' % (Co, C, G), 'fami_dcn_packed_weight_bwd_elems', (Co, C, 3, 3, G)))
        for dil in (1, 3, 7):
            for stride in (1, 2):
                for esz in (4, 2):
                    for det in (0, 1):
                        for fn in ('fami_dcn_bwd_col_width', 'fami_dcn_bwd_col_permuted'):
                            q.append(('%s(C=%d,Co=%d,G=%d,stride=%d,dil=%d,esz=%d,det=%d)' % (fn, C, Co, G, stride, dil, esz, det), fn,
                                      (C, Co, G, 3, 3, stride, dil, esz, det)))
    for B, H, W, C in ((2, 9, 10, 8), (4, 96, 72, 48)):
        q.append(('fami_dcn_bwd_det_workspace(%d,%d,%d,%d)' % (B, H, W, C), 'fami_dcn_bwd_det_workspace', (B, H, W, C)))
    for B in (1, 2, 20):
        q.append(('fami_shift_workspace(%d)' % B, 'fami_shift_workspace', (B,)))
    return q


def dcn_fields(route):
    return [getattr(route, f) for f in DCN_FIELDS]


def run_refusals(L, cases=None):
    """-> {case id: [return code, fami_last_error() text]}.  L: fami_pose_amd._lib.lib()"""
    protos = prototypes()
    buf = ctypes.create_string_buffer(8192)
    dummy = (ctypes.addressof(buf) + 4095) & ~4095          # page-aligned, inside the buffer: nothing may read or write it anyway
    out = {}
    L.bind(None)
    for cid, name, tune, ov in cases or refusal_table():
        args = []
        for p, is_ptr in protos[name]:
            if p in ov:
                v = dummy if ov[p] == 'ptr' else ov[p]
            elif is_ptr:
                v = None if p in OPTIONAL else dummy
            else:
                v = SCALARS[p]
            args.append(v)
        L.cdll.fami_dcn_tune(-1)
        try:
            if tune is not None:
                L.cdll.fami_dcn_tune(tune)
            rc = getattr(L.cdll, name)(*args)
            out[cid] = [rc, L.cdll.fami_last_error().decode()]
        finally:
            L.cdll.fami_dcn_tune(-1)
    return out


def run_queries(L):
    """-> ({setting: {query id: value}}, [what a query or a reset left wrong in the route])"""
    route = L.new_route()
    prev = getattr(L._tls, 'bound', None)
    L.bind(route)
    out, wrong = {}, []
    try:
        for sname, codes in SETTINGS:
            L.cdll.fami_dcn_tune(-1)
            if dcn_fields(route) != DCN_DEFAULTS:
                wrong.append('before %s: fami_dcn_tune(-1) left %s' % (sname, dcn_fields(route)))
            for c in codes:
                L.cdll.fami_dcn_tune(c)
            before = dcn_fields(route)
            if codes and before == DCN_DEFAULTS:
                wrong.append('setting %s wrote no field' % sname)
            res = {}
            for qid, fn, args in query_table():
                res[qid] = int(getattr(L.cdll, fn)(*args))
                if dcn_fields(route) != before:
                    wrong.append('%s under %s: fields %s -> %s' % (qid, sname, before, dcn_fields(route)))
                    before = dcn_fields(route)
            out[sname] = res
            L.cdll.fami_dcn_tune(-1)
            if dcn_fields(route) != DCN_DEFAULTS:
                wrong.append('after %s: fami_dcn_tune(-1) left %s' % (sname, dcn_fields(route)))
    finally:
        L.bind(prev)
    return out, wrong


def test_the_refusal_table_covers_every_entry_point_and_refusal_kind():
    protos, cases = prototypes(), refusal_table()
    compute = ['fami_%s_%s' % (f, dt) for f in FAMILIES for dt in TYPES] + PLAIN
    assert set(protos) == set(compute) | set(QUERIES) | {'fami_dcn_tune'}, sorted(set(protos) ^ (set(compute) | set(QUERIES) | {'fami_dcn_tune'}))
    assert {n for _, n, _, _ in cases} == set(compute)          # (fami_dcn_tune and the queries refuse nothing)
    ids = [c for c, _, _, _ in cases]
    assert len(ids) == len(set(ids))
    for what in ('null x]', 'null om]', 'null dy]', 'null wpb]', 'B 0', 'G 0', 'C % G', 'cg % 4', 'Co > 96', 'C % 4', 'null workspace with gt',
                 'null workspace]', 'too large for the LDS column tile', 'register-fed plan rejects', 'frame too large', 'P >= 2^31'):
        assert any(what in c for c in ids), what
    for _, name, _, ov in cases:          # a deterministic call with gx would launch before it looks at its arguments
        if '_bwd_det' in name and not ({'ws', 'dy'} & set(ov)):
            assert 'gx' in ov and ov['gx'] is None, (name, ov)
        if 'shift_bilinear_bwd' in name and ov.get('gt') == 'ptr':
            assert 'gsrc' not in ov


def test_every_refusal_keeps_its_code_and_text():
    from fami_pose_amd._lib import lib
    L = lib()
    gold = json.load(open(GOLDEN))
    assert re.fullmatch(r'[0-9a-f]{7,40}', gold['commit'])
    got = run_refusals(L)
    assert set(got) == set(gold['refusals']), sorted(set(got) ^ set(gold['refusals']))
    for cid, (rc, text) in got.items():
        assert rc in (-1, -2), 'case %s was not refused before the runtime: %d, %s' % (cid, rc, text)
        assert [rc, text] == gold['refusals'][cid], (cid, rc, text, gold['refusals'][cid])
        assert text.startswith('fami_')


def test_every_query_keeps_its_value_and_writes_no_route_field():
    from fami_pose_amd._lib import lib
    L = lib()
    gold = json.load(open(GOLDEN))
    got, wrong = run_queries(L)
    assert not wrong, wrong
    assert set(got) == set(gold['queries']) == {s for s, _ in SETTINGS}
    for sname, res in got.items():
        assert res == gold['queries'][sname], (sname, sorted(k for k in res if res[k] != gold['queries'][sname].get(k))[:10])
    # the settings are not all alike: the table sees the knobs it turns
    d = got['default']
    assert got['2048'] != d and got['4096+24'] != d and got['1024+1'] != d
