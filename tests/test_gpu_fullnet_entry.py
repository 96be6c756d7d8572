"""cdnet_amd.test.main with --model-name FullNet: a saved checkpoint, two synthetic 72 x 60 images, windows of 48 with overlap 16, both
--postproc values; the result file, the saved label maps against a direct pipeline.infer_image_mask call, and get_probmaps against the
soft-max of the model's own logits."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _checkpoint(tmp_path):
    import torch
    import _fullnet_ref as fr
    from cdnet_amd import checkpoint
    from cdnet_amd.models.FullNet import FullNet
    m = fr.randomize(FullNet(3, 3), 61)
    path = str(tmp_path / 'checkpoint_best.pth.tar')
    torch.save({'epoch': 1, 'state_dict': checkpoint.model_state(m), 'best_iou': 0.0, 'best_loss': 0.0, 'optimizer': None}, path)
    return m.cuda().eval(), path


@pytest.mark.parametrize('postproc', [0, 1])
def test_main_fullnet(tmp_path, postproc):
    import torch
    from PIL import Image
    from test_data_folder import make_dataset
    from cdnet_amd import pipeline, test, utils
    make_dataset(tmp_path, n=2, size=(72, 60), seed=9, sub='test1')
    m, ck = _checkpoint(tmp_path)
    out = tmp_path / 'out'
    avg = test.main(['--model-name', 'FullNet', '--direction', '0', '--img-dir', str(tmp_path / 'images' / 'test1'),
                     '--label-dir', str(tmp_path / 'labels' / 'test1'), '--model-path', ck, '--save-dir', str(out),
                     '--all_img_test', '0', '--patch-size', '48', '--overlap', '16', '--tta', '1', '--postproc', str(postproc)])
    assert avg is not None and list(avg) == test.HEADER and len(avg) == 22
    lines = open(out / 'test1_result.txt').read().split('\n')
    assert lines[0].split('\t') == ['Metrics:'] + test.HEADER
    rows = {ln.split(':')[0]: ln.split('\t')[1:] for ln in lines[3:] if ln}
    assert sorted(rows) == ['im0', 'im1'] and all(len(r) == 22 for r in rows.values())
    for name in ('im0', 'im1'):
        img = np.asarray(Image.open(tmp_path / 'images' / 'test1' / (name + '.png')).convert('RGB'), dtype=np.float32) / 255.0
        x = torch.from_numpy(img).permute(2, 0, 1).contiguous().cuda()
        r = pipeline.infer_image_mask(m, x, tta=True, all_img_test=0, patch_size=48, overlap=16, postproc=postproc, model_mode='FullNet')
        seg = np.asarray(Image.open(out / 'test1_segmentation' / ('b5_%s_seg.tiff' % name))).astype(np.int32)
        assert seg.shape == (72, 60)
        assert np.array_equal(seg, utils.measure_label(r['final'].cpu().numpy()))        # (the saved map is the relabelled one)


def test_get_probmaps_is_the_softmax_of_the_logits(tmp_path):
    import torch
    from cdnet_amd import synth, test
    from cdnet_amd.options import Options
    m, _ = _checkpoint(tmp_path)
    opt = Options(isTrain=False)
    opt.all_img_test = 1
    x = torch.from_numpy(synth.det_input((1, 3, 72, 60), 4))
    prob = test.get_probmaps(x, m, opt)
    with torch.no_grad():
        logits = m(x.cuda())[0]
    want = torch.softmax(logits.double(), 0).cpu().numpy()
    assert prob.shape == (3, 72, 60) and np.abs(prob - want).max() <= 1e-6
