"""Child process of tests/test_train_gpu_ema.py::test_data_parallel_plans_single_rank: the moving average of the weights
on the data-parallel hipGraph plans ('serial' and 'overlap': the update sits in their second graph, behind the optimizers)
and on the serial tail an accumulating data-parallel trainer takes, with a one-rank RCCL process group on the MI355X,
against single-process trainers on the same batches.  The bound is the one tests/test_train_gpu_ema.py derives (an
all-reduce over one rank is the identity and the models are deterministic, so the averages are in fact equal bit for bit;
both are asserted).  A child for the reason tests/_ddp_single_rank.py gives."""
import os
import sys

os.environ.setdefault('HIP_FORCE_DEV_KERNARG', '1')
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import torch

from test_train_gpu_clip import _batch, _trainer


def run(dev, bts, **kw):
    tr = _trainer(dev, True, deterministic=True, lr=1e-3, ema_decay=0.5, **kw)
    for bt in bts:
        tr.step(*bt)
    return tr


def same_average(tr, single, what):
    err = (tr.ema.double() - single.ema.double()).abs().max().item()
    bound = 4 * 3 * 2.0 ** -24 * single.flat.abs().max().item()
    print('%s: |ema - single process| %.3g (bound %.3g), %d updates, %s' % (what, err, bound, tr.ema_updates(), tr.plan_summary()),
          flush=True)
    assert err <= bound and tr.ema_updates() == single.ema_updates(), what
    assert torch.equal(tr.flat, single.flat) and torch.equal(tr.ema, single.ema), what
    assert not torch.equal(tr.ema, tr.flat)


def main(dev):
    import torch.distributed as dist
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29523')
    dist.init_process_group('nccl', rank=0, world_size=1, device_id=dev)
    try:
        bts = [_batch(dev, 9 + k) for k in range(4)]
        single = run(dev, bts)
        assert not single.ddp and single.ema_updates() == 4
        windows = run(dev, bts, accum_steps=2)
        assert not windows.ddp and windows.ema_updates() == 2
        for plan in ('serial', 'overlap'):
            os.environ['FAMI_DDP_PLAN'] = plan
            try:
                tr = run(dev, bts, force_ddp=True, bucket_mb=8)
                assert tr.ddp and tr.use_graph and tr.ddp_plan == plan and len(tr._cache) == 1
                assert tr.plan_summary()['graphs'] >= 2
                same_average(tr, single, plan)
                if plan == 'serial':
                    tr = run(dev, bts, force_ddp=True, bucket_mb=8, accum_steps=2)
                    assert tr.ddp and len(tr._cache) == 1
                    same_average(tr, windows, 'serial tail of an accumulating trainer')
            finally:
                del os.environ['FAMI_DDP_PLAN']
    finally:
        dist.destroy_process_group()


if __name__ == '__main__':
    main(torch.device('cuda:0'))
    print('DDP_EMA_SINGLE_RANK_OK', flush=True)
