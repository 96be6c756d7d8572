"""cdnet_amd.train_util (the plain UNet's train / validate) and the --dice / --weight-map / --alpha 2 switches end to end."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _unet(seed=3):
    import torch
    from cdnet_amd.models.unet import UNet
    torch.manual_seed(seed)
    return UNet(num_classes=3).cuda()


def _sample(B=2, S=64, seed=21):
    """one loader sample (input, weight_map u8 [B,1,S,S] - NOT constant -, target0 {0,127,255}) on the CPU"""
    import torch
    from cdnet_amd import synth
    lab, _, _, weight = synth.train_targets(B, S, S, seed)
    x = torch.from_numpy(synth.det_input((B, 3, S, S), 9))
    target0 = torch.from_numpy(lab.astype(np.int64) * 127 + (lab == 2)).unsqueeze(1)
    return (x, torch.from_numpy(weight), target0), torch.from_numpy(lab)


def test_default_terms_nothing_moves():
    """one UNetTrainer step == one step of an equal model driven by the earlier call sequence (four zero fills + the 9-class
    cdnet_dam_loss_classes over constant point / direction branches): losses and every parameter bit-equal"""
    import torch
    from cdnet_amd import _lib, trainer
    (x, weight, _), lab = _sample()
    xd, labd, wd = x.cuda(), lab.cuda(), weight[:, 0].contiguous().cuda()
    new = trainer.UNetTrainer(_unet())
    got = new.train_step(xd, labd, wd).clone()
    old = trainer.UNetTrainer(_unet())
    logits = old.forward(xd)
    B, _, H, W = logits.shape
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device='cuda')
    point, dirn, dirlab, pt = z((B, 1, H, W), torch.float32), z((B, 9, H, W), torch.float32), z((B, H, W), torch.uint8), z((B, H, W), torch.float16)
    ws = torch.empty((_lib.load().cdnet_dam_loss_classes_workspace_floats(B, H * W, 9),), dtype=torch.float32, device='cuda')
    losses = torch.zeros(11, device='cuda')
    dm, dp, dd = torch.empty_like(logits), torch.empty_like(point), torch.empty_like(dirn)
    _lib.call('cdnet_dam_loss_classes', _lib.ptr(logits), _lib.ptr(point), _lib.ptr(dirn), _lib.ptr(labd), _lib.ptr(dirlab), _lib.ptr(pt),
              _lib.ptr(wd), B, H, W, 9, 1, _lib.ptr(ws), ws.numel(), _lib.ptr(losses), _lib.ptr(dm), _lib.ptr(dp), _lib.ptr(dd), _lib.stream_ptr())
    old.backward(dm)
    old.allreduce_and_step()
    torch.cuda.synchronize()
    assert torch.equal(got[1:3], losses[4:6]) and torch.equal(got[0], losses[4] + losses[5])
    assert torch.equal(new.flat.P, old.flat.P)
    assert float(new.flat.P.abs().sum()) > 0 and np.isfinite(got.cpu().numpy()).all()


def _first_step(extra):
    """the trainer after train_util.train over a one-batch loader with the options `extra`"""
    import torch
    from cdnet_amd import train_util, utils
    from cdnet_amd.options import Options
    opt = Options(isTrain=True).parse(['--model-name', 'UNet'] + extra)
    m = _unet()
    tr, _ = utils.get_optimizer(opt, m)
    sample, _ = _sample()
    dice_out = []
    res = train_util.train([sample], m, tr, None, 0, opt, None, dice_out=dice_out)
    torch.cuda.synchronize()
    assert res.shape == (8,) and np.isfinite(res).all() and len(dice_out) == 1
    return tr, res, dice_out[0]


@pytest.fixture(scope='module')
def default_step():
    tr, res, dice = _first_step([])
    return tr.mask_losses.cpu().numpy().copy(), res, dice


def test_first_step_default(default_step):
    v, res, dice = default_step
    assert v[0] == np.float32(v[1] + v[2]) and res[2] == -1.0 and res[0] == v[0] and res[1] == v[1] and dice == v[2]
    assert 0.0 <= res[3] <= 1.0 and (res[3:] >= 0).all()


@pytest.mark.parametrize('flag', ['--dice=0', '--dice=2', '--weight-map=0', '--alpha=2'])
def test_switches_act(flag, default_step):
    from cdnet_amd import train
    res = train.main(['--synthetic', '2', '--epochs', '1', '--batch-size', '2', '--model-name', 'UNet'] + flag.split('='))
    assert len(res) == 3 and np.isfinite(res).all()
    tr, res8, _ = _first_step(flag.split('='))
    v = tr.mask_losses.cpu().numpy()
    lv = np.float32(tr.loss_var.item())
    d = default_step[0]
    print(flag, v.tolist(), float(lv), d.tolist())
    if flag == '--dice=0':
        assert v[0] == v[1] and v[1] == d[1] and res8[2] == -1.0
    elif flag == '--dice=2':
        assert v[0] == v[2] and v[2] == d[2]
    elif flag == '--weight-map=0':
        assert v[1] != d[1] and v[2] == d[2] and v[0] == np.float32(v[1] + v[2])
    else:
        want = np.float32(v[2] + np.float32(2) * lv)                              # total = dice, then + alpha * loss_var on the device
        assert lv > 0 and abs(v[0] - want) <= np.spacing(want) and res8[2] == float(lv)
        assert v[1] == d[1]                                                       # loss_CE is still logged


def test_dam_model_switches():
    from cdnet_amd import train
    base = ['--synthetic', '1', '--epochs', '1', '--batch-size', '2']
    for flag in (['--weight-map', '0'], ['--alpha', '2']):
        res = train.main(base + flag)
        assert len(res) == 11 and np.isfinite(res).all()
        assert (res[5] > 0) == (flag[0] == '--alpha')
    with pytest.raises(ValueError, match='loss_direction_dice'):
        train.main(base + ['--dice', '0'])


@pytest.mark.parametrize('shape', [(64, 64), (48, 80)])
@pytest.mark.parametrize('all_img_test', [1, 0])
def test_validate_against_torch_on_the_models_own_logits(shape, all_img_test):
    import torch
    import torch.nn.functional as F
    from cdnet_amd import synth, train_util, utils
    from cdnet_amd.options import Options
    from oracle import train as ot
    H, W = shape
    m = _unet()
    opt = Options(isTrain=True).parse(['--model-name', 'UNet'])
    opt.train['input_size'], opt.train['val_overlap'] = 48, 16
    lab, _, _, weight = synth.train_targets(1, H, W, 5)
    x = torch.from_numpy(synth.det_input((1, 3, H, W), 4))
    target0 = torch.from_numpy(lab.astype(np.int64) * 127 + (lab == 2)).unsqueeze(1)
    got = train_util.validate([(x, torch.from_numpy(weight), target0)], m, None, 0, opt, None, all_img_test=all_img_test)
    assert got.shape == (6,)
    m.eval()
    with torch.no_grad():
        logits = (m(x.cuda()) if all_img_test == 1 else utils.split_forward(m, x, 48, 16, opt)).float().cpu()
    assert tuple(logits.shape) == (1, 3, H, W)
    label = torch.from_numpy(lab).long()
    ce = F.nll_loss(F.log_softmax(logits, 1), label)                           # unweighted (train_util.py:387-389)
    dice = ot.multiclass_dice(F.softmax(logits, 1), F.one_hot(label, 3).permute(0, 3, 1, 2).float())
    np.testing.assert_allclose(got[0], float(ce + dice), rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(got[1:], ot.pixel_metrics(logits.argmax(1).numpy(), lab), rtol=1e-6)


def test_validation_run_writes_checkpoint_best(tmp_path):
    import os
    from cdnet_amd import train
    d = str(tmp_path / 'u')
    res = train.main(['--synthetic', '2', '--epochs', '1', '--batch-size', '2', '--model-name', 'UNet', '--validation', '1', '--synthetic-val', '1',
                      '--save-dir', d])
    assert len(res) == 3 and np.isfinite(res).all()
    assert os.path.exists(os.path.join(d, 'checkpoints', 'checkpoint_best.pth.tar'))
