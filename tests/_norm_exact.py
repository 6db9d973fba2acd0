"""Helpers of tests/test_norm_exact_gpu.py (and of tools/norm_digests.py): integer operands of a [P, C] BatchNorm whose
every sum and every output is exact in any order, the fp64 reference, and the launches of the fami_bn_* /
fami_channel_sum_* entry points into guarded, poisoned buffers (tests/_conv_exact.Arena).

How the backward stays exact: dx = gamma*invstd*(dz - mean(dz) - xhat*mean(dz*xhat)) is exact only if the two means are, so
the operands are built until sum dz = k1*P and sum dz*xhat = k2*P per channel with small integers k1, k2 (k2 even): random
integers first, then the deficit is spread over the rows where xhat = +-invstd (moves both sums) and over the rows where
xhat = 0 (moves sum dz alone).  mean is an integer, invstd in {0.5, 1, 2}, gamma an integer with gamma*invstd an integer,
beta in {1, 2}; the ReLU mask is the one of y = (x - mean)*invstd*gamma + beta itself, so relu 1 (mask from y) and relu 2
(mask recomputed from x) see the same dz.  Masked rows of dy carry non-zero garbage.  No mean is exactly 0, neither the
given one nor the batch mean of x: the kernels form a mean as pivot + (sum of (x - pivot)) * (1 / P) in fp64, which lands
within 1e-16 of the pivot's magnitude -- the exact fp32 value of any other mean, but 6e-17 instead of a 0.  No number below is a tolerance but the
two the issue sets for the statistics entry points (1 fp32 ulp on mean / invstd, 1e-5 on the running statistics)."""
import ctypes
import functools

import torch

from _conv_exact import Arena, DT, EXACT16, EXACT32, mismatch

EPS, MOM = float(torch.tensor(1e-5, dtype=torch.float32)), float(torch.tensor(0.1, dtype=torch.float32))   # as the C ABI's floats carry them
EPS_SLOTS = 0.25        # host-written slot rows: var + 0.25 in {4, 1, 0.25}, so invstd comes out as exactly 0.5, 1 or 2
# (P, C, fami_bn_tune_small argument or None)
CASES = [
    (1, 4, None),         # P = 1: the `P > 1` guard of the unbiased variance
    (100, 16, None),      # one-launch small kernels, idle threads
    (701, 48, None),      # 33 648 elements, just past the small-tensor threshold: 21 rows, 4 idle threads, 5 workgroups, main loop once + tail
    (8300, 4, None),      # 256 rows per workgroup
    (300, 1024, None),    # one row per workgroup
    (8200, 384, None),    # 513 row groups: the BN_MAXG cap and the Gp = 511 branch
    (701, 48, -(1000 + 2)),   # the bn2_maxg cap of the two-launch statistics grids
]


def case_id(c):
    return '%dx%d%s' % (c[0], c[1], '' if c[2] is None else '-maxg2')


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g, dtype=torch.int64).double()


def _spread(total, n):
    """n integers that sum to the integer `total`, as even as possible"""
    total = int(total)
    base, rem = divmod(total, n)
    out = torch.full((n,), float(base), dtype=torch.float64)
    out[:rem] += 1
    return out


class Case:
    """Operands and fp64 references of one [P, C] shape, on the CPU; integers=False: seeded random floats (digests only)."""

    def __init__(self, P, C, integers=True):
        self.P, self.C, self.integers = P, C, integers
        g = torch.Generator().manual_seed(1000003 * P + C)
        if not integers:
            self._floats(g)
            return
        self.invstd = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (C,), generator=g)]
        sign = _ints(g, (C,), 0, 1) * 2 - 1
        self.mean = sign * _ints(g, (C,), 1, 3)           # never 0: see the docstring
        sign = _ints(g, (C,), 0, 1) * 2 - 1
        self.gamma = torch.where(self.invstd == 0.5, 2 * sign, sign * _ints(g, (C,), 1, 2))
        self.beta = _ints(g, (C,), 1, 2)
        d = _ints(g, (P, C), -4, 4)                       # x - mean
        if P >= 3:
            d[1] = 0
            d[2] = torch.sign(self.gamma)
        if P >= 4:
            d[P - 1] += ((d + self.mean).sum(0) == 0)      # no batch mean of exactly 0 either
        self.x = d + self.mean
        self.xhat = d * self.invstd
        self.res, self.y0 = _ints(g, (P, C), -4, 4), _ints(g, (P, C), -4, 4)
        self.dx0, self.dres0 = _ints(g, (P, C), -4, 4), _ints(g, (P, C), -4, 4)
        self.dgamma0, self.dbeta0, self.sum0 = _ints(g, (C,), -4, 4), _ints(g, (C,), -4, 4), _ints(g, (C,), -4, 4)
        self.rm0, self.rv0 = _ints(g, (C,), -2, 2), _ints(g, (C,), 1, 3)
        self.ybn = d * (self.invstd * self.gamma) + self.beta          # the BatchNorm output before the ReLU
        mask = self.ybn > 0
        dz = _ints(g, (P, C), -3, 3) * mask
        k1, k2 = _ints(g, (C,), -1, 2), 2 * _ints(g, (C,), -1, 1)
        if P >= 3:
            for c in range(C):
                unit = ((d[:, c] == torch.sign(self.gamma[c])) & mask[:, c]).nonzero()[:, 0]
                zero = ((d[:, c] == 0) & mask[:, c]).nonzero()[:, 0]
                assert len(unit) and len(zero)
                step = float(torch.sign(self.gamma[c]) * self.invstd[c])            # xhat of a `unit` row
                need = (k2[c] * P - (dz[:, c] * self.xhat[:, c]).sum()) / step
                assert need == need.round()
                dz[unit, c] += _spread(need, len(unit))
                dz[zero, c] += _spread(k1[c] * P - dz[:, c].sum(), len(zero))
        self.dz = dz
        self.sum_dz, self.sum_dzx = dz.sum(0), (dz * self.xhat).sum(0)
        self.c1, self.c2 = self.sum_dz / P, self.sum_dzx / P
        if P >= 3:
            assert torch.equal(self.c1, k1) and torch.equal(self.c2, k2)
        garbage = _ints(g, (P, C), 1, 3) * (_ints(g, (P, C), 0, 1) * 2 - 1)
        self.dy = torch.where(mask, dz, garbage)           # what the mask must remove is never zero
        self.yrelu = self.ybn.clamp(min=0)
        gi = self.gamma * self.invstd
        self.dx_train = gi * (dz - self.c1 - self.xhat * self.c2)
        self.dx_eval = dz * gi
        # batch statistics of x (statistics entry points) and the sums around the pivot x[0]
        self.bmean, self.bvar = self.x.mean(0), self.x.var(0, unbiased=False)
        # host-written forward slot rows: mean = pivot + k, var + EPS_SLOTS = 1 / invstd^2
        self.pivot = _ints(g, (C,), -3, 3)
        k = self.mean - self.pivot
        self.slot_var = 1.0 / (self.invstd * self.invstd) - EPS_SLOTS
        self.slot_s, self.slot_q = k * P, (self.slot_var + k * k) * P

    def _floats(self, g):
        P, C = self.P, self.C
        r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
        self.x = r(P, C) * (0.5 + torch.rand(C, generator=g, dtype=torch.float64)) + r(C)
        self.bmean, self.bvar = self.x.mean(0), self.x.var(0, unbiased=False)
        self.mean, self.invstd = self.bmean.float().double(), (1.0 / torch.sqrt(self.bvar + EPS)).float().double()
        self.gamma, self.beta = 1.0 + 0.1 * r(C), 0.1 * r(C)
        self.res, self.y0, self.dx0, self.dres0 = r(P, C), r(P, C), r(P, C), r(P, C)
        self.dgamma0, self.dbeta0, self.sum0 = r(C), r(C), r(C)
        self.rm0, self.rv0 = 0.1 * r(C), 0.5 + torch.rand(C, generator=g, dtype=torch.float64)
        self.ybn = (self.x - self.mean) * self.invstd * self.gamma + self.beta
        self.yrelu = self.ybn.clamp(min=0)
        self.dy = r(P, C)
        self.dz = self.dy * (self.ybn > 0)
        self.pivot = self.x[0].float().double()
        dlt = self.x - self.pivot
        self.slot_s, self.slot_q = dlt.sum(0), (dlt * dlt).sum(0)
        self.sum_dz, self.sum_dzx = self.dz.sum(0), (self.dz * (self.x - self.mean) * self.invstd).sum(0)

    # ---- expected results (fp64), integer cases
    def want_y(self, relu, res):
        r = self.ybn + self.res if res else self.ybn.clone()
        return r.clamp(min=0) if relu else r

    def acc(self, t, prior, on):
        return t + prior if on else t


@functools.lru_cache(maxsize=None)
def make_case(P, C, integers=True):
    return Case(P, C, integers)


def assert_bounds(c, dtype):
    """On the reference alone, before any launch: every sum (and every sum of magnitudes, so every partial sum in any order)
    below 2^24; every activation-typed operand and output exactly representable in the storage type, 16-bit ones within 256."""
    P = c.P
    for t in (c.dz.abs().sum(0), (c.dz * c.xhat).abs().sum(0), c.dy.abs().sum(0), (c.dy * c.xhat).abs().sum(0),
              (c.x - c.x[0]).abs().sum(0), ((c.x - c.x[0]) ** 2).sum(0), c.x.abs().sum(0) + c.sum0.abs(),
              c.sum_dz.abs() + c.dbeta0.abs(), c.sum_dzx.abs() + c.dgamma0.abs(), c.slot_s.abs(), c.slot_q.abs()):
        assert t.max().item() < EXACT32, (P, c.C, t.max().item())
    acts = [c.x, c.dy, c.dz, c.yrelu, c.res, c.y0, c.dx0, c.dres0, c.dz + c.dres0, c.dx_train, c.dx_train + c.dx0, c.dx_eval,
            c.dx_eval + c.dx0] + [c.want_y(r, s) for r in (0, 1) for s in (0, 1)]
    for t in acts:
        if dtype != torch.float32:
            assert t.abs().max().item() <= EXACT16, (P, c.C, t.abs().max().item())
        assert torch.equal(t.to(dtype).double(), t), (P, c.C)


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp(min=1e-30)).item()


def ulp_off(got, want64):
    """None, or a text: got (fp32, device) must lie within one fp32 ulp (the spacing at the value) of want64"""
    g = got.detach().cpu()
    w = want64.float().abs()
    ulp = (torch.nextafter(w, torch.full_like(w, float('inf'))) - w).double()
    ok = (g.double() - want64).abs() <= ulp
    if bool(ok.all()):
        return None
    i = int((~ok).nonzero()[0, 0])
    return '%d of %d channels off by more than 1 ulp; first c = %d: kernel %r, fp64 %r' % (int((~ok).sum()), g.numel(), i, g[i].item(), want64[i].item())


class Runner:
    """One case in one storage type on the device.  Every method launches into fresh guarded outputs and returns
    [(label, output tensor, expected fp64 tensor or None, kind)], kind 'exact' | 'ulp' | 'rel' | 'written'."""

    def __init__(self, L, dev, dt, c):
        self.L, self.dev, self.dt, self.c = L, dev, dt, c
        self.dtype, self.sfx = DT[dt], '_' + dt
        self.st = torch.cuda.current_stream(dev).cuda_stream
        A = self.A = Arena(dev)
        f32 = torch.float32
        for n in ('x', 'dy', 'dz', 'yrelu', 'res'):
            setattr(self, n, A.operand(getattr(c, n), self.dtype))
        for n in ('mean', 'invstd', 'gamma', 'beta', 'pivot'):
            setattr(self, n, A.operand(getattr(c, n), f32))
        self.small = bool(L.cdll.fami_bn_is_small(c.P, c.C))
        torch.cuda.synchronize(dev)

    # ---- plumbing
    def _act(self, prior, name):
        return self.A.output((self.c.P, self.c.C), self.dtype, prior, name)

    def _vec(self, prior, name):
        return self.A.output((self.c.C,), torch.float32, prior, name)

    def _ws(self, nbytes, name='workspace'):
        return self.A.output((max(nbytes // 4, 1),), torch.float32, None, name)

    def _slots(self, rows=None):
        """zeroed slot rows + pivots; rows = (s, q, pivot): written by the host, split over the first two rows"""
        C = self.c.C
        nb = self.L.cdll.fami_bn_slots_bytes(C)
        assert nb % 8 == 0 and nb >= 8 * 2 * C * 8 + 4 * C
        sl = self.A.output((nb // 8,), torch.float64, 0.0, 'slots')
        if rows is not None:
            s, q, piv = rows
            v = sl[:8 * 2 * C].view(8, 2, C)
            v[0, 0], v[0, 1] = (s - 1).to(self.dev), (q - 2).to(self.dev)
            v[1, 0], v[1, 1] = 1.0, 2.0
            if piv is not None:
                sl[8 * 2 * C:].view(torch.float32)[:C] = piv.float().to(self.dev)
        return sl

    @staticmethod
    def _p(t):
        return None if t is None else t.data_ptr()

    def _stat_checks(self, tag, mean, invstd, rm, rv, eps):
        c = self.c
        unb = c.bvar * c.P / (c.P - 1) if c.P > 1 else c.bvar
        return [(tag + ' mean', mean, c.bmean, 'ulp'), (tag + ' invstd', invstd, 1.0 / torch.sqrt(c.bvar + eps), 'ulp'),
                (tag + ' running_mean', rm, (1 - MOM) * c.rm0 + MOM * c.bmean, 'rel'),
                (tag + ' running_var', rv, (1 - MOM) * c.rv0 + MOM * unb, 'rel')]

    # ---- forward
    def stats(self):
        c = self.c
        mean, invstd, rm, rv = self._vec(None, 'mean'), self._vec(None, 'invstd'), self._vec(c.rm0, 'rm'), self._vec(c.rv0, 'rv')
        ws = self._ws(self.L.cdll.fami_bn_workspace(c.C))
        self.L.call('fami_bn_stats' + self.sfx, self.x.data_ptr(), c.P, c.C, mean.data_ptr(), invstd.data_ptr(), rm.data_ptr(),
                    rv.data_ptr(), MOM, EPS, ws.data_ptr(), self.st)
        return self._stat_checks('stats', mean, invstd, rm, rv, EPS)

    def train_fwd(self, two, relu, res):
        """fami_bn_train_fwd_* (two = 0) / fami_bn_train_fwd2_* (two = 1)"""
        c = self.c
        y = self._act(None, 'y')
        mean, invstd, rm, rv = self._vec(None, 'mean'), self._vec(None, 'invstd'), self._vec(c.rm0, 'rm'), self._vec(c.rv0, 'rv')
        tail = self._slots() if two else self._ws(self.L.cdll.fami_bn_workspace(c.C))
        self.L.call('fami_bn_train_fwd%s%s' % ('2' if two else '', self.sfx), self.x.data_ptr(), self._p(self.res if res else None),
                    y.data_ptr(), self.gamma.data_ptr(), self.beta.data_ptr(), mean.data_ptr(), invstd.data_ptr(), rm.data_ptr(),
                    rv.data_ptr(), c.P, c.C, relu, MOM, EPS, tail.data_ptr(), self.st)
        tag = 'train_fwd%s(relu=%d res=%d)' % ('2' if two else '', relu, res)
        return self._stat_checks(tag, mean, invstd, rm, rv, EPS) + [(tag + ' y', y, None, 'written')]

    def finalize_slots(self):
        """slot rows as a convolution epilogue leaves them: sums of (x - pivot), (x - pivot)^2 of the real x"""
        c = self.c
        dlt = c.x - c.pivot
        sl = self._slots((dlt.sum(0), (dlt * dlt).sum(0), c.pivot))
        mean, invstd, rm, rv = self._vec(None, 'mean'), self._vec(None, 'invstd'), self._vec(c.rm0, 'rm'), self._vec(c.rv0, 'rv')
        self.L.call('fami_bn_finalize_slots_f32', sl.data_ptr(), c.P, c.C, mean.data_ptr(), invstd.data_ptr(), rm.data_ptr(),
                    rv.data_ptr(), MOM, EPS, self.st)
        return self._stat_checks('finalize_slots', mean, invstd, rm, rv, EPS)

    def apply(self, relu, res):
        c = self.c
        y = self._act(None, 'y')
        self.L.call('fami_bn_apply' + self.sfx, self.x.data_ptr(), self.mean.data_ptr(), self.invstd.data_ptr(), self.gamma.data_ptr(),
                    self.beta.data_ptr(), self._p(self.res if res else None), y.data_ptr(), c.P, c.C, relu, self.st)
        return [('apply(relu=%d res=%d) y' % (relu, res), y, c.want_y(relu, res) if c.integers else None, 'exact')]

    def apply_slots(self, relu, res):
        """host-written slot rows and pivots whose mean / invstd are exactly the case's"""
        c = self.c
        sl = self._slots((c.slot_s, c.slot_q, c.pivot))
        y = self._act(None, 'y')
        mean, invstd, rm, rv = self._vec(None, 'mean'), self._vec(None, 'invstd'), self._vec(c.rm0, 'rm'), self._vec(c.rv0, 'rv')
        eps = EPS_SLOTS if c.integers else EPS
        self.L.call('fami_bn_apply_slots' + self.sfx, self.x.data_ptr(), self._p(self.res if res else None), y.data_ptr(),
                    self.gamma.data_ptr(), self.beta.data_ptr(), mean.data_ptr(), invstd.data_ptr(), rm.data_ptr(), rv.data_ptr(),
                    c.P, c.C, relu, MOM, eps, sl.data_ptr(), self.st)
        tag = 'apply_slots(relu=%d res=%d)' % (relu, res)
        if not c.integers:
            return [(tag + ' ' + n, t, None, 'exact') for n, t in (('y', y), ('mean', mean), ('invstd', invstd), ('rm', rm), ('rv', rv))]
        unb = c.slot_var * c.P / (c.P - 1) if c.P > 1 else c.slot_var
        return [(tag + ' y', y, c.want_y(relu, res), 'exact'), (tag + ' mean', mean, c.mean, 'exact'), (tag + ' invstd', invstd, c.invstd, 'exact'),
                (tag + ' running_mean', rm, (1 - MOM) * c.rm0 + MOM * c.mean, 'rel'), (tag + ' running_var', rv, (1 - MOM) * c.rv0 + MOM * unb, 'rel')]

    # ---- backward: form 'bwd' | 'bwd2' | 'eval' | 'eval_nosums' | 'slots'
    def bwd(self, form, relu, acc, dres):
        c, L = self.c, self.L
        masked = relu != 0
        g = self.dy if masked else self.dz            # without a mask the gradient is dz itself (zero where the ReLU cut)
        if form == 'slots':
            assert relu == 0
        dx = self._act(c.dx0 if acc else None, 'dx')
        dr = self._act(c.dres0 if acc else None, 'dres') if dres else None
        sums = form != 'eval_nosums'
        dgamma = self._vec(c.dgamma0 if acc else None, 'dgamma') if sums else None
        dbeta = self._vec(c.dbeta0 if acc else None, 'dbeta') if sums else None
        y = self.yrelu if (relu == 1 or (relu == 2 and self.small)) else None      # relu 2 reads no y (the one-launch kernel does)
        accs = (acc, acc, acc)
        if form in ('bwd', 'eval', 'eval_nosums'):
            ws = self._ws(L.cdll.fami_bn_workspace(c.C)) if sums else None
            x, mean = (self.x, self.mean) if sums else (None, None)                 # no sums: x / mean / ws are not read
            L.call('fami_bn_%s%s' % ('bwd' if form == 'bwd' else 'eval_bwd', self.sfx), g.data_ptr(), self._p(x), self._p(y), self._p(mean),
                   self.invstd.data_ptr(), self.gamma.data_ptr(), dx.data_ptr(), self._p(dgamma), self._p(dbeta), self._p(dr), c.P, c.C,
                   relu, *accs, self._p(ws), self.st)
        elif form == 'bwd2':
            L.call('fami_bn_bwd2' + self.sfx, g.data_ptr(), self.x.data_ptr(), self._p(y), self.mean.data_ptr(), self.invstd.data_ptr(),
                   self.gamma.data_ptr(), self.beta.data_ptr(), dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), self._p(dr), c.P, c.C,
                   relu, *accs, self._slots().data_ptr(), self.st)
        else:
            sl = self._slots((c.sum_dz, c.sum_dzx, None))
            L.call('fami_bn_bwd_apply_slots' + self.sfx, g.data_ptr(), self.x.data_ptr(), self.mean.data_ptr(), self.invstd.data_ptr(),
                   self.gamma.data_ptr(), self.beta.data_ptr(), dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), self._p(dr), c.P, c.C,
                   *accs, sl.data_ptr(), self.st)
        tag = '%s(relu=%d acc=%d dres=%d)' % (form, relu, acc, dres)
        I = c.integers
        want_dx = (c.dx_eval if form.startswith('eval') else c.dx_train) if I else None
        out = [(tag + ' dx', dx, c.acc(want_dx, c.dx0, acc) if I else None, 'exact')]
        if dres:
            out.append((tag + ' dres', dr, c.acc(c.dz, c.dres0, acc) if I else None, 'exact'))
        if sums:
            out += [(tag + ' dgamma', dgamma, c.acc(c.sum_dzx, c.dgamma0, acc) if I else None, 'exact'),
                    (tag + ' dbeta', dbeta, c.acc(c.sum_dz, c.dbeta0, acc) if I else None, 'exact')]
        return out

    def channel_sum(self, acc):
        c = self.c
        out = self._vec(c.sum0 if acc else None, 'channel_sum')
        ws = self._ws(self.L.cdll.fami_channel_sum_workspace(c.C))
        self.L.call('fami_channel_sum' + self.sfx, self.x.data_ptr(), c.P, c.C, out.data_ptr(), acc, ws.data_ptr(), self.st)
        return [('channel_sum(acc=%d)' % acc, out, c.acc(c.x.sum(0), c.sum0, acc) if c.integers else None, 'exact')]

    def running_update(self, batch):
        """fami_bn_running_update_f32 / the batched form with two entries on the same buffers (applied in order)"""
        c = self.c
        rm, rv = self._vec(c.rm0, 'rm'), self._vec(c.rv0, 'rv')
        if batch:
            ptrs = (ctypes.c_long * 8)(*([rm.data_ptr(), rv.data_ptr(), self.mean.data_ptr(), self.invstd.data_ptr()] * 2))
            meta = (ctypes.c_float * 8)(*([float(c.C), float(c.P), MOM, EPS] * 2))
            self.L.call('fami_bn_running_update_batch_f32', ptrs, meta, 2, self.st)
        else:
            self.L.call('fami_bn_running_update_f32', rm.data_ptr(), rv.data_ptr(), self.mean.data_ptr(), self.invstd.data_ptr(), c.C, c.P,
                        MOM, EPS, self.st)
        tag = 'running_update%s' % ('_batch' if batch else '')
        return [(tag + ' running_mean', rm, None, 'written'), (tag + ' running_var', rv, None, 'written')]

    # ---- the sets
    def run_deterministic(self):
        """the entry points whose sums are taken in a fixed order (bit-reproducible on any operands)"""
        out = self.stats() + self.apply(0, 0) + self.apply(1, 1) + self.apply_slots(0, 0) + self.apply_slots(1, 1)
        out += self.bwd('bwd', 1, 0, 1) + self.bwd('bwd', 0, 1, 1) + self.bwd('bwd', 1, 0, 0)
        out += self.bwd('eval', 1, 0, 1) + self.bwd('eval', 0, 1, 1) + self.bwd('eval_nosums', 1, 0, 1) + self.bwd('eval_nosums', 0, 1, 0)
        out += self.bwd('slots', 0, 0, 1) + self.bwd('slots', 0, 1, 0)
        out += self.train_fwd(0, 1, 1) + self.finalize_slots()
        out += self.channel_sum(0) + self.channel_sum(1) + self.running_update(0) + self.running_update(1)
        return out

    def run_atomic(self):
        """the two-launch forms: fp64 slot atomics in arrival order (exact on the integer operands)"""
        out = self.train_fwd(1, 0, 0) + self.train_fwd(1, 1, 1)
        out += self.bwd('bwd2', 0, 1, 1) + self.bwd('bwd2', 1, 0, 1) + self.bwd('bwd2', 2, 0, 0)
        return out

    def failures(self, checks):
        """texts of every check that fails (integer cases), guard zones included"""
        torch.cuda.synchronize(self.dev)
        fails = []
        for nm, got, want, kind in checks:
            if kind == 'written' or want is None:
                m = None if not bool(torch.isnan(got.float()).any()) else '%d elements unwritten or NaN' % int(torch.isnan(got.float()).sum())
            elif kind == 'exact':
                m = mismatch(got, want, '(p,c)' if got.dim() == 2 else '(c,)')
            elif kind == 'ulp':
                m = ulp_off(got, want)
            else:
                e = relerr(got, want)
                m = None if e < 1e-5 else 'relative error %.3e >= 1e-5' % e
            if m:
                fails.append('%s: %s' % (nm, m))
        return fails + self.A.touched()
