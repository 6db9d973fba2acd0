"""The streaming kernels of csrc/elementwise.hip and the linear kernels of csrc/core.hip held to EXACT results through the C ABI,
with guard zones around every output and NaN around every operand, in f32, bf16 and f16: layout converts, pack_frames,
copy / concat / split of channels, axpby, cast_add, widen, fill, the HRNet fuse, the two ReLU-masked gradient passes,
scale_pairs, the i64 counters, unscale_check, the chained add_batch and fami_linear_{fwd,bwd}_f32.

Operands, references and launches are in tests/_stream_exact.py: small integers, power-of-two factors, fp32 sums below 2^24
units, 16-bit outputs within 256 -- asserted on the fp64 reference before any launch (and, without a GPU, by
tests/test_stream_exact_host.py).  Every comparison is equality with that reference, rounded once where the output is stored
in 16 bits; there is no tolerance in this module.  Every grid-stride kernel runs below one workgroup, at 256 k + 1 work items
and one work item past the grid cap of 2048 x 256 threads, where some threads take the loop's second trip; every scalar or
unaligned path is taken by one cause at a time."""
import pytest

import _stream_exact as SE

pytestmark = pytest.mark.gpu


def run(fn, cases, dt, dev):
    fails = []
    for c in cases:
        fails += fn(c, dt, SE.Run(dev))
    assert not fails, fails


@pytest.mark.parametrize('dt', SE.TYPES)
def test_layout_converts(dev, dt):
    run(SE.layout, SE.LAYOUT_CASES, dt, dev)


@pytest.mark.parametrize('dt', SE.TYPES)
def test_pack_frames(dev, dt):
    run(SE.pack_frames, SE.PACK_CASES, dt, dev)


@pytest.mark.parametrize('dt', SE.TYPES)
def test_copy_channels(dev, dt):
    run(SE.copy_channels, SE.COPY_CASES, dt, dev)


@pytest.mark.parametrize('dt', SE.TYPES)
def test_concat_and_split_channels(dev, dt):
    run(SE.cat_split, SE.CAT_CASES, dt, dev)


@pytest.mark.parametrize('dt', SE.TYPES)
def test_axpby(dev, dt):
    run(SE.axpby, SE.AXPBY_CASES, dt, dev)


@pytest.mark.parametrize('dt', SE.TYPES)
def test_cast_add_widen_fill(dev, dt):
    run(SE.cast_widen_fill, SE.FLAT_CASES, dt, dev)


@pytest.mark.parametrize('dt', SE.TYPES)
def test_fuse_sum(dev, dt):
    run(SE.fuse_sum, SE.FUSE_CASES, dt, dev)


@pytest.mark.parametrize('dt', SE.TYPES)
def test_relu_bwd(dev, dt):
    run(SE.relu_bwd, SE.RELU_CASES, dt, dev)


@pytest.mark.parametrize('dt', SE.TYPES)
def test_pool_relu_bwd(dev, dt):
    run(SE.pool_relu_bwd, SE.POOL_CASES, dt, dev)


@pytest.mark.parametrize('dt', SE.TYPES)
def test_fuse_sum_and_pool_relu_bwd_refuse_empty_shapes_and_write_nothing(dev, dt):
    fails = SE.fuse_pool_refusals(dt, SE.Run(dev))
    assert not fails, fails


def test_scale_pairs(dev):
    run(SE.scale_pairs, SE.SCALE_PAIRS_CASES, None, dev)


def test_i64_counters(dev):
    run(SE.i64_ops, SE.I64_CASES, None, dev)


def test_unscale_check(dev):
    run(SE.unscale_check, SE.UNSCALE_CASES, None, dev)


def test_add_batch_source_is_an_earlier_output(dev):
    """(a0 -> X), (X -> Y), (Y -> Z) in one 32-entry window.  The host loop used to close a launch on a repeated output only, so
    the three pairs ran as concurrent blocks of one launch and Y could read X before or after its add; a source that is an
    earlier output of the open launch now closes it too.  A race cannot be made to fail on demand: this documents the
    contract (the adds happen in call order) and the fix, it does not prove the bug."""
    fails = SE.add_batch_chain(SE.Run(dev))
    assert not fails, fails


def test_linear_fwd(dev):
    run(SE.linear_fwd, SE.LINEAR_MKN, None, dev)


def test_linear_bwd(dev):
    run(SE.linear_bwd, SE.LINEAR_BWD_CASES, None, dev)


def test_linear_bwd_refuses_db_without_dw_and_writes_nothing(dev):
    fails = SE.linear_bwd_refusal(SE.Run(dev))
    assert not fails, fails
