"""Child process of tests/test_engine_launches_gpu.py::test_data_parallel_plans_single_rank: the Engine's records
(tests/_engine_log.py) of the bf16 case with force_ddp=True, bucket_mb=8 and a one-rank RCCL process group on the MI355X,
under FAMI_DDP_PLAN=overlap and with FAMI_DDP_GRAPH=0 (eager launches, all-reduces fired from the backward hooks): the two
plans that run Engine.backward with bucket hooks and persist_lanes off.  The full records go to `<argv[1]>/<key>.json`; the
parent test compares them with the fixture.  A child for the reason tests/_ddp_single_rank_launches.py gives."""
import json
import os
import sys

os.environ.setdefault('HIP_FORCE_DEV_KERNARG', '1')
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import torch

from _engine_log import DDP_PLANS, environment, record_trainer


def main(dev, out):
    import torch.distributed as dist
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29526')
    dist.init_process_group('nccl', rank=0, world_size=1, device_id=dev)
    try:
        for key, env in DDP_PLANS.items():
            with environment(env):
                calls, counters = record_trainer(dev, 'bf16', graph=True, force_ddp=True, bucket_mb=8)
            with open(os.path.join(out, key + '.json'), 'w') as f:
                json.dump({'calls': calls, 'counters': counters}, f)
    finally:
        dist.destroy_process_group()


if __name__ == '__main__':
    main(torch.device('cuda:0'), sys.argv[1])
    print('DDP_ENGINE_LAUNCHES_SINGLE_RANK_OK', flush=True)
