"""Every fami_bn_* / fami_channel_sum_* entry point on integer operands, against an fp64 CPU reference, bit for bit.

The operands of tests/_norm_exact.py make every sum exact in any order (sums below 2^24, 16-bit outputs within 256: asserted
on the reference before any launch), so dbeta, dgamma, dres, channel_sum -- fresh and accumulating -- and dx / y of the
entry points that take mean / invstd as inputs are compared with torch.equal: the three-launch forms, the frozen-statistics
backward with and without sums, the two-launch forms with relu 0 / 1 / 2 (fp64 slot atomics), the slot apply passes on
host-written slot rows and pivots, and the one-launch small kernels.  The statistics entry points (stats, train_fwd,
train_fwd2, finalize_slots) must give mean / invstd within one fp32 ulp of the fp64 value and the running statistics at 1e-5.
Every output sits between 4096-element guard zones and starts as NaN; every operand sits inside NaN.

Shapes [P, C]: P = 1; the small path with idle threads; just past the small-tensor threshold (idle threads, 5 workgroups,
main loop once + rolled tail); 256 rows per workgroup; one row per workgroup; 513 row groups (the BN_MAXG cap and the
511-workgroup backward grid); and the capped grid of the two-launch statistics passes."""
import pytest
import torch

from _norm_exact import CASES, Runner, assert_bounds, case_id, make_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('dt', ['f32', 'bf16', 'f16'])
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_batchnorm_entry_points_are_exact(dev, case, dt):
    from fami_pose_amd._lib import lib
    L = lib()
    P, C, tune = case
    c = make_case(P, C)
    assert_bounds(c, {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}[dt])      # ... before any launch
    if tune is not None:
        L.call('fami_bn_tune_small', tune)
    try:
        r = Runner(L, dev, dt, c)
        assert r.small == (P * C <= 32768)
        fails = r.failures(r.run_deterministic() + r.run_atomic())
    finally:
        if tune is not None:
            L.call('fami_bn_tune_small', -1)
    assert not fails, '\n'.join(fails)
