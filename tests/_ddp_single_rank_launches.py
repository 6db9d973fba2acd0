"""Child process of tests/test_train_launches_gpu.py::test_data_parallel_plans_single_rank: the launch records
(tests/_launch_log.py) of configurations 1, 7 and 9 with force_ddp=True, bucket_mb=8 and a one-rank RCCL process group on
the MI355X, under FAMI_DDP_PLAN=serial, under overlap, and with FAMI_DDP_GRAPH=0 (eager launches, all-reduces fired from
the backward hooks).  Each Trainer's records go to stdout as one `LAUNCHES <key> <json>` line; the parent test compares
them with the fixture.  A child because creating and destroying an RCCL process group inside the long-lived pytest
process left the HIP runtime in a state where a hipGraph instantiated by a later test crashed in hipGraphLaunch
(the docstring of tests/test_model_gpu.py::test_ddp_path_single_rank_rccl has the details)."""
import json
import os
import sys

os.environ.setdefault('HIP_FORCE_DEV_KERNARG', '1')
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import torch

from _launch_log import CONFIGS, record_steps
from test_train_gpu_clip import _batch, _trainer

PLANS = {'serial': {'FAMI_DDP_PLAN': 'serial'}, 'overlap': {'FAMI_DDP_PLAN': 'overlap'}, 'eager-hooks': {'FAMI_DDP_GRAPH': '0'}}


def main(dev):
    import torch.distributed as dist
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29525')
    dist.init_process_group('nccl', rank=0, world_size=1, device_id=dev)
    try:
        bt = _batch(dev)
        for plan, env in PLANS.items():
            os.environ.update(env)
            try:
                for config in (1, 7, 9):
                    mode, kw = CONFIGS[config]
                    tr = _trainer(dev, True, deterministic=True, mode=mode, force_ddp=True, bucket_mb=8, **kw)
                    assert tr.ddp and tr.use_graph == (plan != 'eager-hooks')
                    print('LAUNCHES ddp-%s-%d %s' % (plan, config, json.dumps(record_steps(tr, bt))), flush=True)
                    del tr
            finally:
                for k in env:
                    del os.environ[k]
    finally:
        dist.destroy_process_group()


if __name__ == '__main__':
    main(torch.device('cuda:0'))
    print('DDP_LAUNCHES_SINGLE_RANK_OK', flush=True)
