"""The references of tests/test_stream_exact_gpu.py and tests/test_loss_exact_gpu.py on the CPU alone: every case of every
family of tests/_stream_exact.py builds its operands and its fp64 reference and asserts the conditions that make the result
exact (representable operands, fp32 sums below 2^24 units, 16-bit outputs within 256, the edge the case is there for).  A bad
seed or bound shows here, without a GPU.  Nothing is launched and the library is not loaded."""
import pytest

import _stream_exact as SE


@pytest.mark.parametrize('dt', SE.TYPES)
@pytest.mark.parametrize('fn,cases', SE.TYPED, ids=[f.__name__ for f, _ in SE.TYPED])
def test_references_of_the_typed_families(fn, cases, dt):
    for c in cases:
        assert fn(c, dt) == []


@pytest.mark.parametrize('fn,cases', SE.UNTYPED, ids=[f.__name__ for f, _ in SE.UNTYPED])
def test_references_of_the_f32_families(fn, cases):
    for c in cases:
        assert fn(c) == []


def test_reference_of_the_add_batch_chain():
    assert SE.add_batch_chain() == []


def test_every_grid_stride_family_has_a_case_past_the_cap():
    """one work item more than 2048 x 256 threads: some threads take a second trip (a work item is four elements where the
    kernel uses ld4 / st4)"""
    cap = SE.CAP
    items = {
        'layout': max(n * c * h * w for n, c, h, w in SE.LAYOUT_CASES),
        'pack_frames': max((1 + s) * b * h * w * 3 for b, s, h, w in SE.PACK_CASES),
        'copy_channels four-wide': max(p[0] * p[5] // 4 for p in SE.COPY_CASES if SE.copy_is_vector(p)),
        'copy_channels scalar': max(p[0] * p[5] for p in SE.COPY_CASES if not SE.copy_is_vector(p)),
        'cat4': max(p * sum(cs) // 4 for cs, p in SE.CAT_CASES),
        'axpby four-wide': max(p[0] // 4 for p in SE.AXPBY_CASES if p[5] is None),
        'axpby scalar': max(p[0] for p in SE.AXPBY_CASES if p[5] is not None),
        'cast_add / widen / fill': max(n for n, _ in SE.FLAT_CASES),
        'fuse_sum': max(p[0] * p[1] * p[2] * p[3] // 4 for p in SE.FUSE_CASES),
        'relu_bwd': max(SE.RELU_CASES) // 4,
        'pool_relu_bwd': max(p[0] * p[1] * p[2] * p[3] // 4 for p in SE.POOL_CASES),
        'i64': max(SE.I64_CASES),
        'unscale_check': max(p[0] // 4 for p in SE.UNSCALE_CASES),
        'wmse_bwd': max(r * l for r, l, _ in SE.WMSE_CASES),
        'gauss_target': max(b * j * h * w for b, j, h, w, _ in SE.GAUSS_CASES),
    }
    assert all(v > cap for v in items.values()), {k: v for k, v in items.items() if v <= cap}
    assert all(v < cap + cap // 64 for k, v in items.items() if k not in ('wmse_bwd',)), items          # ... and most threads do not


def test_the_switch_points_are_cases():
    assert {4095, 4096, 4097, 8192, 8193} <= set(SE.KL_L) and 257 in SE.KL_R          # REG 16 / REG 32 / streaming; scalar_sum's second trip
    assert any(SE.copy_is_vector(p) for p in SE.COPY_CASES) and sum(not SE.copy_is_vector(p) for p in SE.COPY_CASES) >= 5
    assert {p[4] for p in SE.POOL_CASES} == {0, 1, 2, 3, 4} and {p[5] for p in SE.POOL_CASES} == {0, 1}
    assert {len(p[4]) for p in SE.FUSE_CASES} == {1, 2, 3, 4} and {s for p in SE.FUSE_CASES for s, _ in p[4]} == {0, 1, 2, 3}
    assert {p[2] for p in SE.LINEAR_BWD_CASES} == {2, 13, 64}
