"""fami_ema_prep_f32, fami_ema_update_f32 and fami_swap_f32 through the C ABI on the MI355X.

The update is ema = rn(ema + rn(w * rn(p - ema))) bit for bit against three fp32 torch operations on the device (w read
back from the state vector), p and the guard elements around both arrays untouched, for every head / tail length and for
equal and unequal 16-byte alignment of the two arrays.  Against float64 the error per update is at most
3 * 2^-24 * max(|p|, |ema|) per element: three roundings, each at most half an ulp (2^-24 relative) of a value no larger
than 2 max (the difference, which w <= 1/2 halves again), max (the product) and max (the sum, a convex combination).
The prep is the warm-up schedule and the skip gate; the swap is bitwise, NaN payloads included."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

W48 = 64655204
LENGTHS = [1, 3, 5, 1023, 4099, (1 << 20) + 1]
OFFSETS = [(0, 0), (1, 1), (2, 2), (0, 1), (1, 0), (2, 1)]        # (first, second) array: floats behind a 16-byte boundary
DECAYS = [0.5, 0.999, 0.9999]
GUARD = 1234.5


def _st(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _randn(n, dev, seed, scale=1.0):
    return torch.empty(n, device=dev).normal_(generator=torch.Generator(device=dev).manual_seed(seed)).mul_(scale)


def _at(src, off, dev):
    """(buffer, view): a copy of src whose first element sits `off` floats behind a 16-byte boundary, with at least four
    guard elements in front of it and behind it (the idea of tests/test_accum_gpu.py::_at, plus the guards)"""
    buf = torch.full((src.numel() + 12,), GUARD, device=dev)
    assert buf.data_ptr() % 16 == 0
    out = buf[4 + off:4 + off + src.numel()]
    out.copy_(src)
    assert out.data_ptr() % 16 == 4 * off
    return buf, out


def _guards_intact(buf, view):
    lo = (view.data_ptr() - buf.data_ptr()) // 4
    front, back = buf[:lo], buf[lo + view.numel():]
    return front.numel() >= 4 and back.numel() >= 4 and bool((front == GUARD).all()) and bool((back == GUARD).all())


def _prep(st, gate, decay, warmup, dev):
    from fami_pose_amd._lib import lib
    lib().call('fami_ema_prep_f32', st.data_ptr(), None if gate is None else gate.data_ptr(), decay, int(warmup), _st(dev))


def _update(ema, p, st, dev):
    from fami_pose_amd._lib import lib
    lib().call('fami_ema_update_f32', ema.data_ptr(), p.data_ptr(), ema.numel(), st.data_ptr(), _st(dev))


def _swap(a, b, dev):
    from fami_pose_amd._lib import lib
    lib().call('fami_swap_f32', a.data_ptr(), b.data_ptr(), a.numel(), _st(dev))


def _check_update(dev, n, eoff, poff, decay):
    e0, p0 = _randn(n, dev, 11 + n % 7, 4.0), _randn(n, dev, 23 + n % 5, 4.0)
    ebuf, e = _at(e0, eoff, dev)
    pbuf, p = _at(p0, poff, dev)
    st = torch.zeros(4, device=dev)
    _prep(st, None, decay, False, dev)
    assert st[3].item() == 1.0 and st[0].item() == 1.0
    w = st[2]
    want = e0 + w * (p0 - e0)                  # three fp32 operations, each its own kernel: three roundings
    _update(e, p, st, dev)
    assert torch.equal(e, want), (n, eoff, poff, decay)
    assert torch.equal(p, p0)
    assert _guards_intact(ebuf, e) and _guards_intact(pbuf, p)
    ref = e0.double() + w.double() * (p0.double() - e0.double())
    err = (e.double() - ref).abs()
    bound = 3 * 2.0 ** -24 * torch.maximum(p0.abs(), e0.abs()).double()
    worst = (err / bound).max().item()
    assert worst <= 1.0, (n, eoff, poff, decay, worst)
    return worst


@pytest.mark.parametrize('eoff,poff', OFFSETS)
@pytest.mark.parametrize('n', LENGTHS)
def test_update_is_three_rounded_operations_bitwise(dev, n, eoff, poff):
    worst = max(_check_update(dev, n, eoff, poff, d) for d in DECAYS)
    print('n %d ema+%d p+%d: worst error / bound %.3f' % (n, eoff, poff, worst))


def test_update_on_the_w48_arena(dev):
    print('W48 arena: worst error / bound %.3f' % _check_update(dev, W48, 0, 0, 0.999))


def test_prep_counts_updates_and_keeps_the_decay_without_warmup(dev):
    for decay in DECAYS:
        st = torch.zeros(4, device=dev)
        for t in (1, 2, 3):
            _prep(st, None, decay, False, dev)
            d32 = np.float32(decay)
            assert st.tolist() == [float(t), float(d32), float(np.float32(1.0) - d32), 1.0]


def test_prep_warmup_schedule(dev):
    st = torch.zeros(4, device=dev)
    for t in range(1, 11):
        _prep(st, None, 0.999, True, dev)
        tt = np.float32(t)
        want = min(np.float32(0.999), (np.float32(1.0) + tt) / (np.float32(10.0) + tt))
        got = st.tolist()
        assert got[0] == float(t) and got[3] == 1.0
        assert got[1] == pytest.approx(float(want), rel=1e-6)
        assert got[2] == float(np.float32(1.0) - np.float32(got[1]))          # ONE fp32 subtraction of what was stored
    assert got[1] < 0.999                          # still on the ramp: (1 + 10) / (10 + 10)


def test_gate_skips_and_a_skipped_update_changes_no_byte(dev):
    st = torch.zeros(4, device=dev)
    _prep(st, None, 0.999, True, dev)
    _prep(st, None, 0.999, True, dev)
    before = st.clone()
    gate = torch.zeros(1, device=dev)
    _prep(st, gate, 0.999, True, dev)
    assert torch.equal(st[0:3], before[0:3]) and st[3].item() == 0.0
    n = 4099
    e0, p0 = _randn(n, dev, 5), _randn(n, dev, 6)
    for eoff, poff in ((0, 0), (1, 2)):
        ebuf, e = _at(e0, eoff, dev)
        pbuf, p = _at(p0, poff, dev)
        _update(e, p, st, dev)
        assert torch.equal(e.view(torch.int32), e0.view(torch.int32)) and torch.equal(p, p0)
        assert _guards_intact(ebuf, e) and _guards_intact(pbuf, p)
    # a non-zero gate applies: an Adam bias correction (any value in (0, 1]) and SGD's 1.0
    for g in (0.1, 1.0):
        gate.fill_(g)
        t = st[0].item()
        _prep(st, gate, 0.999, True, dev)
        assert st[0].item() == t + 1 and st[3].item() == 1.0
    ebuf, e = _at(e0, 0, dev)
    pbuf, p = _at(p0, 0, dev)
    _update(e, p, st, dev)
    assert torch.equal(e, e0 + st[2] * (p0 - e0)) and not torch.equal(e, e0)


def _bits(n, dev, seed):
    """n floats of random bit patterns: NaNs with payloads, infinities, denormals"""
    gen = torch.Generator(device=dev).manual_seed(seed)
    t = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), dtype=torch.int64, device=dev, generator=gen).to(torch.int32)
    if n >= 5:
        t[0], t[n - 1], t[n // 2] = 0x7fc00001, -8388608, 0x7f800000        # quiet NaN with a payload, -inf, +inf
    return t


def _check_swap(dev, n, aoff, boff):
    a0, b0 = _bits(n, dev, 3 + n % 11), _bits(n, dev, 5 + n % 13)
    abuf, a = _at(a0.view(torch.float32), aoff, dev)
    bbuf, b = _at(b0.view(torch.float32), boff, dev)
    assert torch.equal(a.view(torch.int32), a0) and torch.equal(b.view(torch.int32), b0)
    _swap(a, b, dev)
    assert torch.equal(a.view(torch.int32), b0) and torch.equal(b.view(torch.int32), a0), (n, aoff, boff)
    assert _guards_intact(abuf, a) and _guards_intact(bbuf, b)
    _swap(a, b, dev)
    assert torch.equal(a.view(torch.int32), a0) and torch.equal(b.view(torch.int32), b0)
    assert _guards_intact(abuf, a) and _guards_intact(bbuf, b)


@pytest.mark.parametrize('aoff,boff', OFFSETS)
@pytest.mark.parametrize('n', LENGTHS)
def test_swap_exchanges_bit_for_bit(dev, n, aoff, boff):
    _check_swap(dev, n, aoff, boff)


def test_swap_on_the_w48_arena(dev):
    _check_swap(dev, W48, 0, 0)


def test_bad_arguments_are_refused(dev):
    from fami_pose_amd._lib import FamiError, lib
    a, b, st = torch.zeros(8, device=dev), torch.zeros(8, device=dev), torch.zeros(4, device=dev)
    s = _st(dev)
    for decay in (0.0, 1.0, -0.1, 1.5, float('nan')):
        with pytest.raises(FamiError):
            lib().call('fami_ema_prep_f32', st.data_ptr(), None, decay, 0, s)
    with pytest.raises(FamiError):
        lib().call('fami_ema_prep_f32', None, None, 0.5, 0, s)
    for args in ((None, b.data_ptr(), 8, st.data_ptr()), (a.data_ptr(), None, 8, st.data_ptr()),
                 (a.data_ptr(), b.data_ptr(), 0, st.data_ptr()), (a.data_ptr(), b.data_ptr(), -3, st.data_ptr()),
                 (a.data_ptr(), b.data_ptr(), 8, None)):
        with pytest.raises(FamiError):
            lib().call('fami_ema_update_f32', *args, s)
    for args in ((None, b.data_ptr(), 8), (a.data_ptr(), None, 8), (a.data_ptr(), b.data_ptr(), 0),
                 (a.data_ptr(), b.data_ptr(), -1), (a.data_ptr(), a.data_ptr() + 16, 8)):      # the last: overlapping
        with pytest.raises(FamiError):
            lib().call('fami_swap_f32', *args, s)
    assert not st.any() and not a.any() and not b.any()
