"""fami_accum_unscale_check_sumsq_f32, the pass that closes a gradient-accumulation window, through the C ABI on the MI355X:
g = rn(rn(acc + g) * mul) bit for bit against two fp32 torch operations on the device, its slab bit for bit against
fami_sumsq_f32 of what it wrote, the whole of it bit for bit against the two launches it replaces
(fami_axpby_f32(acc, g, g, 1, 1), then fami_unscale_check_sumsq_f32), and the inf / NaN flag.

The norm bound is the derived one of tests/test_clip_gpu.py: the slab has the layout and the addition order of
sumsq_kernel, whose longest chain of fp32 additions is k = ceil(ceil(n4 / parts) / 256) + 11; the norm is then within
(k + 3) 2^-24 of the float64 norm of the same data."""
import pytest
import torch

pytestmark = pytest.mark.gpu

W48 = 64655204
LENGTHS = [1, 3, 5, 1023, 4099, (1 << 20) + 1, W48]
OFFSETS = [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1)]      # (g, acc): equal and unequal alignment
FACTORS = [1.0, 1.0 / 3.0, 2.0 ** -13]
NAME = 'fami_accum_unscale_check_sumsq_f32'


def _st(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _parts():
    from fami_pose_amd._lib import lib
    return lib().cdll.fami_sumsq_parts()


def _bound(t):
    n = t.numel()
    head = min(n, ((16 - t.data_ptr() % 16) % 16) // 4)
    chunk = -(-((n - head) // 4) // _parts())
    return (-(-chunk // 256) + 2 + 1 + 6 + 2 + 3) * 2.0 ** -24


def _randn(n, dev, seed, scale=1.0):
    return torch.empty(n, device=dev).normal_(generator=torch.Generator(device=dev).manual_seed(seed)).mul_(scale)


def _at(src, off, dev):
    """a copy of src whose first element sits `off` floats behind a 16-byte boundary"""
    buf = torch.empty(src.numel() + 4, device=dev)
    assert buf.data_ptr() % 16 == 0
    out = buf[off:off + src.numel()]
    out.copy_(src)
    return out


def _fused(g, acc, f, fdev, flag, parts, dev):
    from fami_pose_amd._lib import lib
    lib().call(NAME, g.data_ptr(), acc.data_ptr(), g.numel(), f, None if fdev is None else fdev.data_ptr(),
               None if flag is None else flag.data_ptr(), None if parts is None else parts.data_ptr(), _st(dev))


def _sumsq(g, dev):
    from fami_pose_amd._lib import lib
    parts = torch.full((_parts(),), float('nan'), device=dev)
    lib().call('fami_sumsq_f32', g.data_ptr(), g.numel(), parts.data_ptr(), _st(dev))
    return parts


def _norm(parts, dev):
    from fami_pose_amd._lib import lib
    clip, mx = torch.zeros(2, device=dev), torch.ones(1, device=dev)
    flag = torch.zeros(2, dtype=torch.int32, device=dev)
    lib().call('fami_clip_coef_f32', parts.data_ptr(), parts.numel(), mx.data_ptr(), clip.data_ptr(), flag.data_ptr(), _st(dev))
    return clip[0].item()


@pytest.mark.parametrize('goff,aoff', OFFSETS)
@pytest.mark.parametrize('n', LENGTHS)
def test_bitwise_against_two_torch_operations_and_the_two_launch_form(dev, n, goff, aoff):
    """every f, with and without fdev: the arena is (acc + g) * mul as two fp32 torch operations, acc is untouched, the slab
    is fami_sumsq_f32 of the result and its norm within the bound, and arena, slab and flag are those of the two-launch form"""
    from fami_pose_amd._lib import lib
    g0, a0 = _randn(n, dev, 31 + n % 7, 8.0), _randn(n, dev, 47 + n % 5, 8.0)
    acc = _at(a0, aoff, dev)
    dev3 = torch.tensor([0.3], device=dev)
    for f in FACTORS:
        for fdev in (None, dev3):
            f32 = torch.tensor(f, dtype=torch.float32, device=dev)
            mul = f32 if fdev is None else f32 * fdev[0]              # one fp32 product, as the kernel forms it
            want = (a0 + g0) * mul
            g = _at(g0, goff, dev)
            assert g.data_ptr() % 16 == 4 * goff and acc.data_ptr() % 16 == 4 * aoff
            flag = torch.zeros(2, dtype=torch.int32, device=dev)
            parts = torch.full((_parts(),), float('nan'), device=dev)
            _fused(g, acc, f, fdev, flag, parts, dev)
            assert torch.equal(g, want), (n, goff, aoff, f, fdev is not None)
            assert torch.equal(acc, a0)
            assert flag.tolist() == [0, 0]
            assert torch.equal(parts, _sumsq(g, dev))
            ref = g.double().norm().item()
            err = abs(_norm(parts, dev) - ref) / ref if ref > 0 else 0.0
            assert err <= _bound(g), (err, _bound(g))
            # the two launches of the parent commit
            h = _at(g0, goff, dev)
            flag2 = torch.zeros(2, dtype=torch.int32, device=dev)
            parts2 = torch.full((_parts(),), float('nan'), device=dev)
            lib().call('fami_axpby_f32', acc.data_ptr(), h.data_ptr(), h.data_ptr(), n, 1.0, 1.0, _st(dev))
            lib().call('fami_unscale_check_sumsq_f32', h.data_ptr(), n, f, None if fdev is None else fdev.data_ptr(),
                       flag2.data_ptr(), parts2.data_ptr(), _st(dev))
            assert torch.equal(g, h) and torch.equal(parts, parts2) and torch.equal(flag, flag2)
    print('n %d g+%d acc+%d: last norm error %.3g (bound %.3g)' % (n, goff, aoff, err, _bound(g)))


@pytest.mark.parametrize('n', [5, 4099, (1 << 20) + 1])
@pytest.mark.parametrize('case', ['inf_in_acc', 'opposite_infs', 'overflow_after_mul'])
def test_flag_is_raised_like_the_two_launch_form(dev, case, n):
    """inf only in acc; +inf in g with -inf in acc (NaN); a finite sum that the multiplier takes past fp32's largest"""
    from fami_pose_amd._lib import lib
    g0, a0 = _randn(n, dev, 61), _randn(n, dev, 62)
    spot = n - 1 if n < 4099 else 4097           # the scalar tail / inside the vector body
    f = 0.5
    if case == 'inf_in_acc':
        a0[spot] = float('inf')
    elif case == 'opposite_infs':
        g0[spot], a0[spot] = float('inf'), float('-inf')
    else:
        g0[spot], a0[spot], f = 1.5e38, 1.5e38, 2.0
    g, acc = _at(g0, 0, dev), _at(a0, 0, dev)
    flag = torch.zeros(2, dtype=torch.int32, device=dev)
    parts = torch.zeros(_parts(), device=dev)
    _fused(g, acc, f, None, flag, parts, dev)
    assert flag.tolist() == [1, 0]
    want = (a0 + g0) * torch.tensor(f, dtype=torch.float32, device=dev)
    assert not torch.isfinite(want[spot]) and torch.isfinite(a0[spot] + g0[spot]) == (case == 'overflow_after_mul')
    assert torch.equal(torch.nan_to_num(g, nan=7.0), torch.nan_to_num(want, nan=7.0))
    h = _at(g0, 0, dev)
    flag2 = torch.zeros(2, dtype=torch.int32, device=dev)
    lib().call('fami_axpby_f32', acc.data_ptr(), h.data_ptr(), h.data_ptr(), n, 1.0, 1.0, _st(dev))
    lib().call('fami_unscale_check_sumsq_f32', h.data_ptr(), n, f, None, flag2.data_ptr(), None, _st(dev))
    assert torch.equal(flag, flag2)


@pytest.mark.parametrize('n', [3, 1023, (1 << 20) + 1])
def test_finite_data_raises_nothing_and_null_flag_and_null_partials_are_accepted(dev, n):
    g0, a0 = _randn(n, dev, 71), _randn(n, dev, 72)
    want = (a0 + g0) * torch.tensor(1.0 / 3.0, dtype=torch.float32, device=dev)
    acc = _at(a0, 0, dev)
    flag = torch.zeros(2, dtype=torch.int32, device=dev)
    parts = torch.full((_parts(),), float('nan'), device=dev)
    for fl, pt in ((flag, None), (None, parts), (None, None), (flag, parts)):
        g = _at(g0, 0, dev)
        _fused(g, acc, 1.0 / 3.0, None, fl, pt, dev)
        assert torch.equal(g, want) and flag.tolist() == [0, 0]
    assert torch.equal(parts, _sumsq(g, dev))
    # no flag: non-finite values pass through unreported
    a0[0] = float('inf')
    g = _at(g0, 0, dev)
    _fused(g, _at(a0, 0, dev), 1.0, None, None, None, dev)
    assert torch.isinf(g[0]) and flag.tolist() == [0, 0]


def test_bad_arguments_are_refused(dev):
    from fami_pose_amd._lib import FamiError, lib
    g, acc = torch.zeros(8, device=dev), torch.zeros(8, device=dev)
    for args in ((None, acc.data_ptr(), 8), (g.data_ptr(), None, 8), (g.data_ptr(), acc.data_ptr(), 0)):
        with pytest.raises(FamiError):
            lib().call(NAME, args[0], args[1], args[2], 1.0, None, None, None, _st(dev))
