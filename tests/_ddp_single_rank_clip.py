"""Child process of tests/test_train_gpu_clip.py::test_data_parallel_plans_clip_and_scale_single_rank: gradient clipping
and the dynamic loss scale on the three data-parallel plans ('overlap' and 'serial' hipGraph plans: their g2 segment
holds the norm, the coefficient, the scale update and the optimizers; and the eager hook-driven plan) with a one-rank
RCCL process group on the MI355X.  A child for the reason tests/_ddp_single_rank.py gives."""
import os
import sys

os.environ.setdefault('HIP_FORCE_DEV_KERNARG', '1')
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import torch

from test_train_gpu_clip import _TorchTwin, _batch, _norm_bound, _relerr, _trainer


def clipped(dev, plan):
    """three steps, the last two clipped: norm against float64, parameters against clip_grad_norm_ + torch.optim.Adam"""
    tr = _trainer(dev, True, lr=1e-3, max_grad_norm=1e9, force_ddp=True, bucket_mb=8)
    assert tr.ddp and tr.use_graph == (plan != 'eager') and (plan == 'eager' or tr.ddp_plan == plan)
    twin = _TorchTwin(tr)
    opt = torch.optim.Adam(twin.params, lr=1e-3)
    bt = _batch(dev)
    max_norm = 1e9
    for k in range(3):
        tr.step(*bt)
        want = tr.grad.detach().cpu().double().norm().item()
        got = tr.grad_norm()
        assert abs(got - want) / want <= _norm_bound(tr.grad), (plan, k, got, want)
        assert (tr.clip_coef() < 1.0) == (k > 0)
        twin.clip(tr.grad, max_norm)
        opt.step()
        if k == 0:
            max_norm = 0.1 * got
            tr.set_max_grad_norm(max_norm)
    e = _relerr(tr.flat.cpu(), twin.flat)
    print('%s: clipped parameters relerr %.3g, %s' % (plan, e, tr.plan_summary()), flush=True)
    assert e < 1e-6 and tr.skipped_steps() == 0
    assert plan == 'eager' or len(tr._cache) == 1


def scaled(dev, plan):
    """fp16, init_scale 2^40 backing off by 2^-8: overflowing steps are skipped with the parameters untouched, then steps run"""
    tr = _trainer(dev, True, mode='f16', lr=1e-3, max_grad_norm=1.0, loss_scale='dynamic', force_ddp=True, bucket_mb=8,
                  scaler=dict(init_scale=2.0 ** 40, backoff_factor=2.0 ** -8, growth_interval=100))
    bt = _batch(dev)
    start = tr.flat.detach().clone()
    scales = []
    for k in range(6):
        before = tr.flat.detach().clone()
        skipped = tr.skipped_steps()
        scale = tr.loss_scale_value()
        tr.step(*bt)
        if tr.skipped_steps() > skipped:
            assert torch.equal(tr.flat, before) and tr.loss_scale_value() == scale * 2.0 ** -8
        else:
            assert not torch.equal(tr.flat, before) and tr.loss_scale_value() == scale
        scales.append(tr.loss_scale_value())
    print('%s: scales %s, %d skipped' % (plan, scales, tr.skipped_steps()), flush=True)
    assert 1 <= tr.skipped_steps() <= 5 and tr.opt.state[0].item() == 6 - tr.skipped_steps()
    assert torch.isfinite(tr.flat).all() and not torch.equal(tr.flat, start)
    assert plan == 'eager' or len(tr._cache) == 1


def main(dev):
    import torch.distributed as dist
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29519')
    dist.init_process_group('nccl', rank=0, world_size=1, device_id=dev)
    try:
        for plan in ('overlap', 'serial', 'eager'):
            env = {'FAMI_DDP_GRAPH': '0'} if plan == 'eager' else {'FAMI_DDP_PLAN': plan}
            os.environ.update(env)
            try:
                clipped(dev, plan)
                scaled(dev, plan)
            finally:
                for k in env:
                    del os.environ[k]
    finally:
        dist.destroy_process_group()


if __name__ == '__main__':
    main(torch.device('cuda:0'))
    print('DDP_CLIP_SINGLE_RANK_OK', flush=True)
