"""Host side of the band kernel's weight-DMA form (csrc/conv_t4.hip): the switch changes how a launch stages its weights, never
WHETHER the split-product band kernel takes a shape -- the engine's decisions not to materialise a normalised input
(fami_conv2d_xbn_ok_f32) hang on that answer -- and it is a route field with a default like its neighbours.  No GPU."""
import ctypes
import random

OFF, ON = 102040, 102041

BRANCHES = [(20, 96, 72, 48, 48), (20, 48, 36, 96, 96), (20, 24, 18, 192, 192), (20, 12, 9, 384, 384)]
HEAD = [(4, 96, 72, 48, 48), (4, 96, 72, 96, 48), (4, 96, 72, 192, 48), (4, 96, 72, 384, 48)]
PREDICTORS = [(4, 96, 72, 48, 216), (4, 96, 72, 48, 108), (4, 96, 72, 216, 48), (4, 96, 72, 108, 48)]


def _table():
    rnd = random.Random(20251019)
    ch = [8, 16, 20, 32, 48, 64, 80, 96, 108, 144, 192, 216, 256, 384]
    return BRANCHES + HEAD + PREDICTORS + [(rnd.randint(1, 24), rnd.randint(1, 100), rnd.randint(1, 80), rnd.choice(ch), rnd.choice(ch))
                                           for _ in range(50)]


def test_the_switch_changes_no_eligibility_answer():
    from fami_pose_amd._lib import lib
    L = lib()
    L.bind(None)
    try:
        ans = {}
        for code in (OFF, ON):
            L.cdll.fami_conv_tune_lds(-1)
            L.cdll.fami_conv_tune_lds(code)
            # fami_conv_t4_eligible is fami_conv_t4_eligible_s3, the f32 half of fami_conv2d_xbn_ok_f32; the plan query agrees with it
            ans[code] = [(L.cdll.fami_conv_t4_eligible(*g), L.cdll.fami_conv2d_xbn_ok_f32(*g)) for g in _table()]
            assert [a for a, _ in ans[code]] == [int(L.cdll.fami_conv_t4_s3_plan(*g, 1, 1, 1, None) != 0) for g in _table()]
        assert ans[OFF] == ans[ON]
        assert any(a for a, _ in ans[ON]) and not all(a for a, _ in ans[ON])      # the table asks on both sides of the answer
        assert all(a == 1 for a, _ in ans[ON][:8]), ans[ON][:8]                  # the branch and head shapes are the kernel's
        # the form itself follows the switch where a pre-split image exists and two weight buffers fit
        out = (ctypes.c_long * 5)()
        assert L.cdll.fami_conv_t4_s3_plan(20, 12, 9, 384, 384, 1, 1, 0, out) == 2 and out[1] - out[0] == 9 * 3 * 1536
        L.cdll.fami_conv_tune_lds(OFF)
        assert L.cdll.fami_conv_t4_s3_plan(20, 12, 9, 384, 384, 1, 1, 0, out) == 1
    finally:
        L.cdll.fami_conv_tune_lds(-1)


def test_route_field_default_and_reset():
    from fami_pose_amd._lib import lib
    L = lib()
    r = L.new_route()
    assert r.t4_s3_wdma == 1
    L.bind(r)
    try:
        L.cdll.fami_conv_tune_lds(OFF)
        assert r.t4_s3_wdma == 0 and r.t4_s3_fill == 2 and r.t4_s3_narrow == 0      # (tested before the >= 102000 range of t4_s3_fill)
        L.cdll.fami_conv_tune_lds(ON)
        assert r.t4_s3_wdma == 1 and r.t4_s3_fill == 2
        L.cdll.fami_conv_tune_lds(OFF)
        L.cdll.fami_conv_tune_lds(-1)
        assert r.t4_s3_wdma == 1
    finally:
        L.bind(None)
