"""Child process of tests/test_train_gpu_accum.py::test_data_parallel_plans_accumulate_single_rank: gradient accumulation
on the three data-parallel plans ('overlap', 'serial', eager hooks -- with accum_steps > 1 all three take the serial tail:
grad = accum + grad, every bucket's all-reduce, the unscale pass with 1 / N in its factor, the optimizers) with a one-rank
RCCL process group on the MI355X, against the single-process accumulating trainer.  A child for the reason
tests/_ddp_single_rank.py gives."""
import os
import sys

os.environ.setdefault('HIP_FORCE_DEV_KERNARG', '1')
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import torch

from test_train_gpu_clip import _batch, _trainer


def windows(dev, bts, **kw):
    """two windows of N = 2 -> (trainer, all-reduce calls per step() call)"""
    tr = _trainer(dev, True, deterministic=True, lr=1e-3, accum_steps=2, **kw)
    calls, per_call = [], []
    inner = tr.reducer.allreduce
    tr.reducer.allreduce = lambda lo, hi: (calls.append((lo, hi)), inner(lo, hi))[1]
    for bt in bts:
        n = len(calls)
        tr.step(*bt)
        per_call.append(len(calls) - n)
    return tr, per_call


def main(dev):
    import torch.distributed as dist
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29521')
    dist.init_process_group('nccl', rank=0, world_size=1, device_id=dev)
    try:
        bts = [_batch(dev, 9 + k) for k in range(4)]
        single, none = windows(dev, bts)
        assert not single.ddp and none == [0, 0, 0, 0] and single.opt.state[0].item() == 2.0
        for plan in ('overlap', 'serial', 'eager'):
            env = {'FAMI_DDP_GRAPH': '0'} if plan == 'eager' else {'FAMI_DDP_PLAN': plan}
            os.environ.update(env)
            try:
                tr, per_call = windows(dev, bts, force_ddp=True, bucket_mb=8)
                assert tr.ddp and tr.use_graph == (plan != 'eager') and (plan == 'eager' or tr.ddp_plan == plan)
                buckets = len(tr.reducer.ranges())
                print('%s: all-reduces per call %s, %d buckets, %s' % (plan, per_call, buckets, tr.plan_summary()), flush=True)
                assert buckets > 1 and per_call == [0, buckets, 0, buckets]
                assert torch.equal(tr.grad, single.grad) and torch.equal(tr.flat, single.flat), plan
                assert tr.window_loss_value() == single.window_loss_value()
                assert plan == 'eager' or len(tr._cache) == 1
            finally:
                for k in env:
                    del os.environ[k]
    finally:
        dist.destroy_process_group()


if __name__ == '__main__':
    main(torch.device('cuda:0'))
    print('DDP_ACCUM_SINGLE_RANK_OK', flush=True)
