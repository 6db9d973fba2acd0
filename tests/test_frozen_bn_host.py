"""Host side of BatchNorm with frozen statistics (no GPU): scope selection of freeze_batchnorm, the flag's life cycle, the
C prototypes, and the checkpoint entry."""
import ctypes

import pytest
import torch

import fami_pose_amd as fp
from fami_pose_amd.train import freeze_batchnorm, frozen_batchnorm_names


@pytest.fixture(scope='module')
def model():
    return fp.build_model(fp.default_cfg(48, image_size=(96, 128), num_sup=2), 'train')


def _bn_names(model):
    return [n for n, m in model.named_modules() if isinstance(m, torch.nn.BatchNorm2d)]


def test_scope_selection(model):
    every = _bn_names(model)
    backbone = [n for n in every if n.startswith('hrnet.')]
    assert len(every) > len(backbone) > 100
    assert fp.freeze_batchnorm is freeze_batchnorm
    assert freeze_batchnorm(model, 'all') == every == frozen_batchnorm_names(model)
    assert freeze_batchnorm(model, 'backbone') == backbone == frozen_batchnorm_names(model)      # the call states the whole set
    pre = ('hrnet.stage2.', 'hrnet.bn1')
    want = [n for n in every if n.startswith(pre)]
    assert want and freeze_batchnorm(model, pre) == want == frozen_batchnorm_names(model)
    assert freeze_batchnorm(model, 'hrnet.layer1.') == [n for n in every if n.startswith('hrnet.layer1.')]
    assert freeze_batchnorm(model, None) == [] == frozen_batchnorm_names(model)
    assert not any(hasattr(m, 'frozen_stats') for m in model.modules())


def test_unknown_prefix_raises_and_changes_nothing(model):
    freeze_batchnorm(model, 'backbone')
    before = frozen_batchnorm_names(model)
    with pytest.raises(ValueError, match='no_such_module'):
        freeze_batchnorm(model, ('hrnet.', 'no_such_module.'))
    with pytest.raises(ValueError):
        freeze_batchnorm(model, ())
    with pytest.raises(ValueError):
        freeze_batchnorm(model, ('hrnet.conv1',))          # a convolution: the prefix matches no BatchNorm
    assert frozen_batchnorm_names(model) == before
    freeze_batchnorm(model, None)


def test_flag_survives_train_and_eval_and_stays_out_of_the_state_dict(model):
    keys = list(model.state_dict().keys())
    names = freeze_batchnorm(model, 'all')
    try:
        model.eval()
        assert frozen_batchnorm_names(model) == names
        model.train()
        assert frozen_batchnorm_names(model) == names
        assert all(m.training for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d))
        assert list(model.state_dict().keys()) == keys and len(keys) == 1929
    finally:
        freeze_batchnorm(model, None)


def test_engine_predicate():
    from fami_pose_amd.engine import Engine
    bn = torch.nn.BatchNorm2d(4)
    assert Engine.bn_batch_stats(bn)
    bn.frozen_stats = True
    assert not Engine.bn_batch_stats(bn)
    bn.frozen_stats = False
    assert Engine.bn_batch_stats(bn)
    bn.eval()
    assert not Engine.bn_batch_stats(bn)


def test_prototypes_parse_with_the_argument_list_of_bn_bwd():
    from fami_pose_amd._lib import parse_header
    protos = parse_header()
    for sfx in ('f32', 'bf16', 'f16'):
        ret, args = protos['fami_bn_eval_bwd_' + sfx]
        assert ret is ctypes.c_int
        assert args == protos['fami_bn_bwd_' + sfx][1] and len(args) == 18
        assert args[10:17] == [ctypes.c_long] + [ctypes.c_int] * 5 + [ctypes.c_void_p]


def test_checkpoint_entry(tmp_path, model):
    from fami_pose_amd import checkpoint as ck
    opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad][:2], lr=0.1)
    plain = torch.load(ck.save_checkpoint(0, str(tmp_path / 'plain'), model, opt), map_location='cpu')
    assert sorted(plain) == ['begin_epoch', 'optimizer', 'state_dict']                 # without the option: today's keys
    names = freeze_batchnorm(model, 'backbone')
    try:
        path = ck.save_checkpoint(1, str(tmp_path / 'frozen'), model, opt)
        saved = torch.load(path, map_location='cpu')
        assert sorted(saved) == ['begin_epoch', 'frozen_bn', 'optimizer', 'state_dict'] and saved['frozen_bn'] == names
        assert sorted(saved['state_dict']) == sorted(plain['state_dict'])
        assert ck.resume(model, opt, path)[2] == 2                                     # the same set: loads
        freeze_batchnorm(model, 'all')
        with pytest.raises(ValueError, match='frozen_bn') as e:
            ck.resume(model, opt, path)
        assert 'hrnet.bn1' in str(e.value) and 'frozen_bn=' in str(e.value)
        freeze_batchnorm(model, None)
        with pytest.raises(ValueError, match='frozen_bn'):
            ck.resume(model, opt, path)                                                # none is another set too
        freeze_batchnorm(model, 'all')
        assert ck.resume(model, opt, ck.get_latest_checkpoint(str(tmp_path / 'plain')))[2] == 1      # a file that does not say: loads
    finally:
        freeze_batchnorm(model, None)
