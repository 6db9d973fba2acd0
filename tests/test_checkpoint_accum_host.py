"""The 'grad_accum' checkpoint entry of a Trainer with gradient accumulation, on the host: save -> load -> equal inside and
between windows; a different accum_steps on either side is refused before anything is loaded; a trainer without
accumulation keeps the file's three keys.  CPU only: the Trainer's methods run on a stand-in whose arenas are host tensors."""
import pytest
import torch

from fami_pose_amd import checkpoint as ck
from fami_pose_amd.train import FlatAdam, Trainer, flatten_parameters


class _HostTrainer:
    """What checkpoint.py needs from train.Trainer, without a GPU."""

    accum_state_dict = Trainer.accum_state_dict
    load_accum_state_dict = Trainer.load_accum_state_dict
    reset_window = Trainer.reset_window

    def __init__(self, model, accum_steps=None):
        self.flat, self.table = flatten_parameters(model)
        self.opt = FlatAdam(self.flat, lr=1e-3)
        self.dynamic_scale = False
        if accum_steps is not None:          # (a trainer of before the option has no such attribute at all)
            self.accum_steps = accum_steps
        self.window_position = 0
        if accum_steps is not None and accum_steps > 1:
            self.accum = torch.zeros_like(self.flat)
            self._window_loss = torch.zeros(2, 7)


def _net():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.BatchNorm2d(4))


def test_grad_accum_entry_round_trip_inside_a_window(tmp_path):
    src = _HostTrainer(_net(), 4)
    torch.manual_seed(1)
    src.accum.copy_(torch.randn(src.accum.numel()))
    src._window_loss[0].copy_(torch.arange(7.0) + 0.5)
    src._window_loss[1].fill_(-1.0)                      # the last closed window: reporting only, not state
    src.window_position = 2
    path = ck.save_checkpoint(3, str(tmp_path), _net(), src)
    saved = torch.load(path, map_location='cpu')
    assert sorted(saved) == ['begin_epoch', 'grad_accum', 'optimizer', 'state_dict']
    assert sorted(saved['grad_accum']) == ['arena', 'loss_sum', 'position', 'steps']
    assert saved['grad_accum']['steps'] == 4 and saved['grad_accum']['position'] == 2
    assert saved['grad_accum']['arena'].dtype == torch.float32 and torch.equal(saved['grad_accum']['arena'], src.accum)
    model = _net()
    dst = _HostTrainer(model, 4)
    _, _, begin = ck.resume(model, dst, path)
    assert begin == 4 and dst.window_position == 2
    assert torch.equal(dst.accum, src.accum) and torch.equal(dst._window_loss[0], src._window_loss[0])
    assert not dst._window_loss[1].any()


def test_grad_accum_entry_between_windows_has_no_arena(tmp_path):
    src = _HostTrainer(_net(), 3)
    src.accum.fill_(7.0)                                 # a closed window's leftovers are not state
    path = ck.save_checkpoint(0, str(tmp_path), _net(), src)
    saved = torch.load(path, map_location='cpu')
    assert saved['grad_accum'] == {'steps': 3, 'position': 0}
    model = _net()
    dst = _HostTrainer(model, 3)
    dst.window_position = 1                              # an open window of the resuming trainer is dropped
    ck.resume(model, dst, path)
    assert dst.window_position == 0 and not dst.accum.any()


def test_mismatching_accum_steps_are_refused_before_anything_is_loaded(tmp_path):
    src_model = _net()
    with torch.no_grad():
        src_model[0].weight.add_(1.0)
    src = _HostTrainer(src_model, 4)
    src.window_position = 1
    path = ck.save_checkpoint(0, str(tmp_path), src_model, src)
    for steps in (2, 1, None):                           # another window length, accum_steps=1, a trainer without the option
        model = _net()
        dst = _HostTrainer(model, steps)
        before = dst.flat.clone()
        with pytest.raises(ValueError, match='accum_steps'):
            ck.resume(model, dst, path)
        assert torch.equal(dst.flat, before) and dst.window_position == 0
    # a position outside the window is refused too
    saved = torch.load(path, map_location='cpu')
    saved['grad_accum']['position'] = 4
    torch.save(saved, path)
    model = _net()
    with pytest.raises(ValueError):
        ck.resume(model, _HostTrainer(model, 4), path)


def test_keys_are_unchanged_without_accumulation(tmp_path):
    for steps in (None, 1):
        plain = _HostTrainer(_net(), steps)
        path = ck.save_checkpoint(0, str(tmp_path / str(steps)), _net(), plain)
        assert sorted(torch.load(path, map_location='cpu')) == ['begin_epoch', 'optimizer', 'state_dict']
        # ... and such a checkpoint starts an accumulating trainer at position 0
        model = _net()
        dst = _HostTrainer(model, 2)
        dst.window_position = 1
        ck.resume(model, dst, path)
        assert dst.window_position == 0
