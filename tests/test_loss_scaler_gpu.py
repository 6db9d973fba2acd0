"""fami_loss_scale_update_f32 against torch.amp.GradScaler('cpu') on the MI355X: the same scripted overflow sequence
drives both; scale and growth tracker must be exactly equal after every step (all values are powers of two)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _st(dev):
    return torch.cuda.current_stream(dev).cuda_stream


class _TorchScaler:
    """torch.amp.GradScaler('cpu') driven through its public protocol: a one-element parameter whose gradient is inf
    on the steps that overflow"""

    def __init__(self, **kw):
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.opt = torch.optim.SGD([self.p], lr=0.0)
        self.sc = torch.amp.GradScaler('cpu', **kw)

    def step(self, overflow):
        self.sc.scale(self.p.sum()).backward()          # (initialises the scaler lazily on the first step)
        self.p.grad = torch.full((1,), float('inf') if overflow else 1.0)
        self.sc.step(self.opt)
        self.sc.update()
        return self.sc.get_scale(), self.sc.state_dict()['_growth_tracker']


def test_scale_update_follows_grad_scaler(dev):
    """overflows at steps 1 and 5 of 10, growth_interval 3"""
    from fami_pose_amd._lib import lib
    ref = _TorchScaler(init_scale=2.0 ** 16, growth_interval=3)
    scaler = torch.tensor([2.0 ** 16, 2.0 ** -16, 0.0], device=dev)
    flag = torch.zeros(2, dtype=torch.int32, device=dev)
    used, seen = [], []
    for step in range(1, 11):
        used.append(scaler[0].item())
        overflow = step in (1, 5)
        flag[0] = int(overflow)
        lib().call('fami_loss_scale_update_f32', scaler.data_ptr(), flag.data_ptr(), 2.0, 0.5, 3, _st(dev))
        assert flag[0].item() == int(overflow)          # the update only reads the flag
        want_scale, want_tracker = ref.step(overflow)
        scale, inv, tracker = scaler.tolist()
        seen.append(scale)
        assert scale == want_scale and tracker == want_tracker, (step, scale, want_scale, tracker, want_tracker)
        assert inv == 1.0 / scale
    # the scale each of the ten steps ran with
    assert used == [65536, 32768, 32768, 32768, 65536, 32768, 32768, 32768, 65536, 65536]
    assert seen[-1] == 65536


def test_growth_that_would_reach_inf_is_refused(dev):
    from fami_pose_amd._lib import lib
    ref = _TorchScaler(init_scale=2.0 ** 127, growth_interval=1)
    scaler = torch.tensor([2.0 ** 127, 2.0 ** -127, 0.0], device=dev)
    flag = torch.zeros(2, dtype=torch.int32, device=dev)
    for _ in range(2):
        lib().call('fami_loss_scale_update_f32', scaler.data_ptr(), flag.data_ptr(), 2.0, 0.5, 1, _st(dev))
        want_scale, want_tracker = ref.step(False)
        assert scaler[0].item() == want_scale == 2.0 ** 127 and scaler[2].item() == want_tracker == 0
