"""GPU: the DAM inference entry honours --postproc 1 (test_dam.py:558-563): pipeline.infer_image(..., postproc=1) and
cdnet_amd.test_dam.main(['--postproc', '1', ...])."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _model():
    import torch
    from cdnet_amd.models.dam.model_unet_rev1 import Unet
    torch.manual_seed(1)
    return Unet(backbone_name='vgg16_bn', pretrained=False, classes=3).cuda().eval()


def test_infer_image_postproc_1_and_0():
    import torch
    from cdnet_amd import pipeline, postproc, postproc_other, synth
    from oracle import postproc as orc
    m = _model()
    H, W = 120, 152
    img = torch.from_numpy(synth.det_input((3, H, W), 8)).cuda()
    kw = dict(tta=True, all_img_test=0, patch_size=64, overlap=16, min_area=20, radius=2)
    r0 = pipeline.infer_image(m, img, **kw)
    pred = r0['pred']
    # postproc 0 (given or not) is today's chain: fill holes, remove small (min_area), 8-connected label, dilate
    today = orc.cc_chain(pred.cpu().numpy() == 1, 20, 2)
    r0b = pipeline.infer_image(m, img, postproc=0, **kw)
    for r in (r0, r0b):
        assert 'postproc_err' not in r
        assert np.array_equal(r['final'].cpu().numpy(), today['final']) and r['count'] == today['count']
    inside = (pred == 1).to(torch.uint8)
    for mode in ('UNet2RevA1_vgg16', 'micronet', 'unet'):                   # the watershed variant, the per-instance loop, ws forced off
        r = pipeline.infer_image(m, img, postproc=1, model_mode=mode, **kw)
        assert torch.equal(r['pred'], pred)
        want = postproc.dilate_labels(postproc_other.process(inside, mode, min_size=10), 2)     # min_size 10, not min_area (test_dam.py:559)
        assert r['final'].dtype == torch.int32 and torch.equal(r['final'], want), mode
        ids = np.unique(want.cpu().numpy())
        assert r['count'] == len(ids[ids > 0]) and int(r['counts']) == r['count'] and int(r['postproc_err']) == 0
        assert r['counts'].is_cuda and r['counts'].dtype == torch.int32
    # the last mode against the host yardstick and the oracle's disk dilation
    host = orc.dilate_disk(postproc_other.process_host(inside.cpu().numpy().astype(np.float32) * 255, 'micronet'), 2)
    r = pipeline.infer_image(m, img, postproc=1, model_mode='micronet', defer=True, **kw)
    assert 'count' not in r and r['counts'].is_cuda
    assert np.array_equal(r['final'].cpu().numpy(), host)
    assert int(r['counts']) == len(np.unique(host[host > 0]))


def test_main_with_postproc_1(tmp_path, monkeypatch):
    import torch
    from test_data_folder import make_dataset
    from cdnet_amd import checkpoint, postproc, test_dam, trainer
    from cdnet_amd.models.dam.model_unet_rev1 import Unet
    make_dataset(tmp_path, n=2, size=(96, 112), seed=5, sub='test1')
    torch.manual_seed(0)
    m = Unet(backbone_name='vgg16_bn', pretrained=False, classes=3).cuda()
    tr = trainer.Trainer(m)
    batch = trainer.synthetic_batch(2, torch.device('cuda:0'), seed=1, H=64, W=64)
    for _ in range(3):
        tr.train_step(*batch)
    ck = checkpoint.save_checkpoint(checkpoint.make_state(m, tr, 0), 0, True, str(tmp_path), 'Main', 0)
    calls = []
    chain = postproc.other_chain

    def spy(pred, model_mode, radius=2):
        out = chain(pred, model_mode, radius)
        calls.append((model_mode, radius, out['final']))
        return out
    monkeypatch.setattr(postproc, 'other_chain', spy)
    out = str(tmp_path / 'out')
    avg = test_dam.main(['--img-dir', str(tmp_path / 'images' / 'test1'), '--label-dir', str(tmp_path / 'labels' / 'test1'),
                         '--save-dir', out, '--model-path', ck, '--postproc', '1', '--radius', '1'])
    assert [c[:2] for c in calls] == [('UNet2RevA1_vgg16', 1)] * 2
    assert os.path.exists(os.path.join(out, 'test_results.txt'))
    assert avg is not None and 'AJI' in avg
    from PIL import Image
    for i in range(2):
        seg = np.asarray(Image.open(os.path.join(out, 'im%d_seg.tiff' % i))).astype(np.int32)
        assert np.array_equal(seg, calls[i][2][0].cpu().numpy())
