"""`UNet_vgg16` through the command-line entries: python -m cdnet_amd.train on synthetic data (train_util's mask-only loop, the reference's
checkpoint layout, interchange with a plain-PyTorch copy of the network) and python -m cdnet_amd.test on an image folder."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ARGS = ['--model-name', 'UNet_vgg16', '--direction', '0', '--synthetic', '2', '--epochs', '1', '--batch-size', '2']


def test_training_entry_writes_a_checkpoint_the_mirror_loads(tmp_path):
    import torch
    import _backbone_unet_ref as br
    from cdnet_amd import checkpoint, train
    from cdnet_amd.models.model_unet import Unet
    d = str(tmp_path / 'run')
    res = train.main(ARGS + ['--save-dir', d])
    assert len(res) == 3 and np.isfinite(res).all(), res
    path = os.path.join(d, 'checkpoints', 'checkpoint.pth.tar')
    assert os.path.exists(path)
    ck = torch.load(path, map_location='cpu', weights_only=False)
    keys = list(ck['state_dict'])
    assert all(k.startswith('module.') for k in keys)
    mirror = br.BackboneUnet(3)
    assert [k[len('module.'):] for k in keys] == list(mirror.state_dict())
    mirror.load_state_dict({k[len('module.'):]: v for k, v in ck['state_dict'].items()}, strict=True)
    assert int(ck['state_dict']['module.backbone.1.num_batches_tracked']) == 2
    # the other way: a checkpoint the mirror wrote, DataParallel prefix and all, into the device class
    torch.manual_seed(5)
    src = br.BackboneUnet(3)
    theirs = str(tmp_path / 'theirs.pth.tar')
    torch.save({'epoch': 3, 'state_dict': {'module.' + k: v for k, v in src.state_dict().items()}, 'best_iou': 0.5, 'best_loss': 1.0,
                'optimizer': None}, theirs)
    m = Unet(backbone_name='vgg16_bn', pretrained=False, classes=3).cuda()
    got = checkpoint.load_checkpoint(theirs, m)
    assert got['epoch'] == 3
    sd = m.state_dict()
    for k, v in src.state_dict().items():
        assert torch.equal(sd[k].cpu(), v), k


def test_training_entry_needs_direction_0(tmp_path):
    from cdnet_amd import train
    args = [a for a in ARGS]
    args[args.index('--direction') + 1] = '1'
    with pytest.raises(ValueError, match='--direction 0'):
        train.main(args + ['--save-dir', str(tmp_path / 'no')])
    assert not os.path.exists(tmp_path / 'no' / 'checkpoints')


def test_inference_entry_matches_infer_image_mask(tmp_path, monkeypatch):
    import torch
    from PIL import Image
    from test_data_folder import make_dataset
    from cdnet_amd import checkpoint, pipeline, test
    from cdnet_amd.models.model_unet import Unet
    from cdnet_amd.options import Options
    make_dataset(tmp_path, n=1, size=(96, 80), seed=9, sub='test1')
    torch.manual_seed(2)
    m = Unet(backbone_name='vgg16_bn', pretrained=False, classes=3)
    ck = str(tmp_path / 'weights.pth.tar')
    torch.save({'epoch': 1, 'state_dict': checkpoint.model_state(m), 'best_iou': 0.0, 'best_loss': 1.0, 'optimizer': None}, ck)
    args = ['--model-name', 'UNet_vgg16', '--direction', '0', '--img-dir', str(tmp_path / 'images' / 'test1'),
            '--label-dir', str(tmp_path / 'labels' / 'test1'), '--model-path', ck, '--save-dir', str(tmp_path / 'out')]
    avg = test.main(args)
    assert avg is not None and list(avg) == test.HEADER and len(avg) == 22
    assert all(np.isfinite(v) for v in avg.values()), avg
    lines = open(tmp_path / 'out' / 'test1_result.txt').read().split('\n')
    assert lines[0].split('\t') == ['Metrics:'] + test.HEADER and lines[1].startswith('Average:\t') and lines[2] == ''
    rows = [ln for ln in lines[3:] if ln]
    assert len(rows) == 1 and rows[0].startswith('im0:') and len(rows[0].split('\t')) == 23
    seg = np.asarray(Image.open(tmp_path / 'out' / 'test1_segmentation' / 'b5_im0_seg.tiff')).astype(np.int32)
    # the same image through pipeline.infer_image_mask on the same model, directly
    opt = Options(isTrain=False).parse(args)
    model = test._load_model(opt, False)
    img = np.asarray(Image.open(tmp_path / 'images' / 'test1' / 'im0.png').convert('RGB'), dtype=np.float32) / 255.0
    x = torch.from_numpy(img).permute(2, 0, 1).contiguous()
    if 'normalize' in opt.transform['test']:
        mean, std = opt.transform['test']['normalize']
        x = (x - torch.tensor(mean, dtype=torch.float32).view(3, 1, 1)) / torch.tensor(std, dtype=torch.float32).view(3, 1, 1)
    r = pipeline.infer_image_mask(model, x.cuda(), opt)
    final = r['final'].cpu().numpy()
    assert final.shape == (96, 80)
    from cdnet_amd import test_dam
    gt = test_dam.ground_truth_instances(str(tmp_path / 'labels' / 'test1'), 'im0')
    _, relab = test.image_metrics(final, gt)                     # (the saved map is the relabelled one)
    assert np.array_equal(relab, seg)
