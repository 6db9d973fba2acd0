"""The 'ema' checkpoint entry of a Trainer with a moving average of the weights, on the host: save -> load -> equal, the
entry merged over 'state_dict' loads into a fresh module, a renamed or reshaped entry is refused before anything is loaded,
and a trainer without an average keeps the file's three keys and resumes a file that has the entry.  CPU only: the
Trainer's methods run on a stand-in whose arenas are host tensors (as tests/test_checkpoint_accum_host.py does)."""
import pytest
import torch

from fami_pose_amd import checkpoint as ck
from fami_pose_amd.train import FlatAdam, Trainer, flatten_parameters


class _HostTrainer:
    """What checkpoint.py needs from train.Trainer, without a GPU."""

    ema_state_dict = Trainer.ema_state_dict
    load_ema_state_dict = Trainer.load_ema_state_dict
    check_ema_state_dict = Trainer.check_ema_state_dict
    set_ema_decay = Trainer.set_ema_decay
    reset_ema = Trainer.reset_ema
    ema_updates = Trainer.ema_updates
    _ema_rows = Trainer._ema_rows
    _require_ema = Trainer._require_ema
    _set_ema_updates = Trainer._set_ema_updates

    def __init__(self, model, ema_decay=None, ema_warmup=False):
        self.model = model
        self.flat, self.table = flatten_parameters(model)
        self.opt = FlatAdam(self.flat, lr=1e-3)
        self.dynamic_scale = False
        if ema_decay is not None:           # (a trainer of before the option has no such attributes at all)
            self.ema_decay, self.ema_warmup = ema_decay, ema_warmup
            self._ema_version = 0
            self.ema = self.flat.detach().clone()
            self.ema_state = torch.zeros(4)
            self._set_ema_updates(0)


def _net(seed=0, frozen=False):
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.BatchNorm2d(4), torch.nn.Conv2d(4, 2, 1))
    if frozen:
        net[2].bias.requires_grad_(False)
    return net


def _averaged(seed=1, **kw):
    """a stand-in whose average differs from its weights, with 7 updates behind it"""
    model = _net(**kw)
    src = _HostTrainer(model, 0.999, True)
    torch.manual_seed(seed)
    src.ema.copy_(torch.randn(src.ema.numel()))
    src._set_ema_updates(7)
    return model, src


def test_ema_entry_round_trip(tmp_path):
    model, src = _averaged(frozen=True)
    path = ck.save_checkpoint(3, str(tmp_path), model, src)
    saved = torch.load(path, map_location='cpu')
    assert sorted(saved) == ['begin_epoch', 'ema', 'optimizer', 'state_dict']
    assert sorted(saved['ema']) == ['decay', 'params', 'updates', 'warmup']
    assert saved['ema']['decay'] == 0.999 and saved['ema']['warmup'] is True and saved['ema']['updates'] == 7
    trainable = [k for k, p in model.named_parameters() if p.requires_grad]
    assert len(trainable) == 5 and '2.bias' not in trainable
    assert list(saved['ema']['params']) == trainable and set(trainable) < set(saved['state_dict'])
    for (k, v), (p, off, n) in zip(saved['ema']['params'].items(), src.table):
        assert v.dtype == torch.float32 and v.shape == p.shape and torch.equal(v.reshape(-1), src.ema[off:off + n])
        assert not torch.equal(v, saved['state_dict'][k])
    dst_model = _net(5, frozen=True)
    dst = _HostTrainer(dst_model, 0.5)
    _, _, begin = ck.resume(dst_model, dst, path)
    assert begin == 4
    assert torch.equal(dst.ema, src.ema) and torch.equal(dst.flat, src.flat) and not torch.equal(dst.ema, dst.flat)
    assert torch.equal(dst.ema_state, src.ema_state) and dst.ema_updates() == 7
    # decay and warm-up are taken from the entry, and a captured plan would re-capture
    assert dst.ema_decay == 0.999 and dst.ema_warmup is True and dst._ema_version == 1
    assert dst.ema_state.tolist()[1] == pytest.approx(8.0 / 17.0, rel=1e-6)


def test_entry_over_state_dict_loads_into_a_fresh_module(tmp_path):
    model, src = _averaged()
    saved = torch.load(ck.save_checkpoint(0, str(tmp_path), model, src), map_location='cpu')
    fresh = _net(9)
    fresh.load_state_dict({**saved['state_dict'], **saved['ema']['params']}, strict=True)
    for k, p in fresh.named_parameters():
        assert torch.equal(p.data, saved['ema']['params'][k])
    assert torch.equal(fresh[1].running_mean, model[1].running_mean)          # buffers: the live ones


@pytest.mark.parametrize('damage', ['renamed', 'reshaped', 'missing'])
def test_mismatching_entry_is_refused_before_anything_is_loaded(tmp_path, damage):
    model, src = _averaged()
    with torch.no_grad():
        src.flat.add_(1.0)
    path = ck.save_checkpoint(0, str(tmp_path), model, src)
    saved = torch.load(path, map_location='cpu')
    params = saved['ema']['params']
    if damage == 'renamed':
        params['0.kernel'] = params.pop('0.weight')
    elif damage == 'reshaped':
        params['0.weight'] = params['0.weight'].reshape(4, 27)
    else:
        del params['2.bias']
    torch.save(saved, path)
    dst_model = _net(5)
    dst = _HostTrainer(dst_model, 0.999, True)
    dst._set_ema_updates(2)
    flat, ema, st = dst.flat.clone(), dst.ema.clone(), dst.ema_state.clone()
    opt_state, rm = dst.opt.state.clone(), dst_model[1].running_mean.clone()
    with pytest.raises(ValueError, match='ema'):
        ck.resume(dst_model, dst, path)
    assert torch.equal(dst.flat, flat) and torch.equal(dst.ema, ema) and torch.equal(dst.ema_state, st)
    assert torch.equal(dst.opt.state, opt_state) and torch.equal(dst_model[1].running_mean, rm)
    with pytest.raises(ValueError, match='ema'):
        dst.load_ema_state_dict(saved['ema'])
    assert torch.equal(dst.ema, ema) and torch.equal(dst.ema_state, st)


def test_trainer_without_an_average_keeps_the_three_keys_and_ignores_the_entry(tmp_path):
    model, src = _averaged()
    with_entry = ck.save_checkpoint(0, str(tmp_path / 'a'), model, src)
    plain_model = _net(5)
    plain = _HostTrainer(plain_model)
    assert not hasattr(plain, 'ema')
    path = ck.save_checkpoint(0, str(tmp_path / 'b'), plain_model, plain)
    assert sorted(torch.load(path, map_location='cpu')) == ['begin_epoch', 'optimizer', 'state_dict']
    _, _, begin = ck.resume(plain_model, plain, with_entry)
    assert begin == 1 and torch.equal(plain.flat, src.flat) and not hasattr(plain, 'ema')


def test_file_without_the_entry_restarts_the_average_from_the_loaded_weights(tmp_path):
    plain_model = _net(5)
    path = ck.save_checkpoint(0, str(tmp_path), plain_model, _HostTrainer(plain_model))
    model, dst = _averaged()
    assert dst.ema_updates() == 7 and not torch.equal(dst.ema, dst.flat)
    ck.resume(model, dst, path)
    want = torch.cat([p.detach().reshape(-1) for p in plain_model.parameters()])
    assert torch.equal(dst.flat, want) and torch.equal(dst.ema, dst.flat) and dst.ema_updates() == 0
    assert dst.ema_state.tolist()[3] == 0.0
