"""python -m cdnet_amd.train --model-name FullNet on synthetic data (fp32 precision mode): train_util's loop, validation, the reference's
checkpoint layout, and the inherited loss terms and optimisers."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ARGS = ['--synthetic', '2', '--epochs', '1', '--batch-size', '2', '--model-name', 'FullNet', '--direction', '0', '--validation', '1',
        '--synthetic-val', '1']


@pytest.fixture
def fp32_mode():
    import cdnet_amd
    before = cdnet_amd.get_precision()
    cdnet_amd.set_precision('fp32')
    yield
    cdnet_amd.set_precision(before)


def test_entry_point_trains_validates_and_saves(tmp_path, fp32_mode):
    import torch
    from cdnet_amd import test as cdtest
    from cdnet_amd import train
    from cdnet_amd.models.FullNet import FullNet
    from cdnet_amd.options import Options
    d = str(tmp_path / 'fullnet')
    res = train.main(ARGS + ['--save-dir', d])
    assert len(res) == 3 and np.isfinite(res).all(), res
    path = os.path.join(d, 'checkpoints', 'checkpoint_best.pth.tar')
    assert os.path.exists(path)
    ck = torch.load(path, map_location='cpu', weights_only=False)
    keys = list(ck['state_dict'])
    assert len(keys) == 301 and all(k.startswith('module.') for k in keys)
    assert [k[len('module.'):] for k in keys] == list(FullNet(3, 3).state_dict())
    assert int(ck['state_dict']['module.conv1.bn.num_batches_tracked']) == 2
    assert all(int(s['step']) == 2 for s in ck['optimizer']['state'].values())
    # the mask-only inference entry loads it
    opt = Options(isTrain=False).parse(['--model-name', 'FullNet', '--direction', '0', '--model-path', path])
    m = cdtest._load_model(opt, True)
    assert isinstance(m, FullNet) and not m.training
    sd = m.state_dict()
    assert torch.equal(sd['conv2.weight'].cpu(), ck['state_dict']['module.conv2.weight'])
    assert torch.equal(sd['blocks.trans7.bn.running_var'].cpu(), ck['state_dict']['module.blocks.trans7.bn.running_var'])
    with torch.no_grad():
        out = m(torch.randn(1, 3, 64, 64, device='cuda'))
    assert out.shape == (1, 3, 64, 64) and bool(torch.isfinite(out).all())


def test_entry_point_with_the_inherited_terms_and_ranger(tmp_path, fp32_mode):
    from cdnet_amd import train
    assert ARGS[:2] == ['--synthetic', '2']
    args = ['--synthetic', '1'] + ARGS[2:]                             # one step
    res = train.main(args + ['--save-dir', str(tmp_path / 'terms'), '--alpha', '1', '--boundary-loss', '1', '--optimizer', 'ranger'])
    assert len(res) == 3 and np.isfinite(res).all(), res


def test_entry_point_refuses_bf16_mode(tmp_path):
    import cdnet_amd
    from cdnet_amd import train
    before = cdnet_amd.get_precision()
    cdnet_amd.set_precision('bf16')
    try:
        with pytest.raises(NotImplementedError, match='fp32 precision mode'):
            train.main(ARGS + ['--save-dir', str(tmp_path / 'bf16')])
    finally:
        cdnet_amd.set_precision(before)
