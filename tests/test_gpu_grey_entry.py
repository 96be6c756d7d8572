"""The entries on a grey-scale dataset (--dataset BBBC039V1, in_c = 1): cdnet_amd.train on synthetic one-channel tiles and on a folder of
mode-L PNGs with --device-augment, then cdnet_amd.test_dam and cdnet_amd.test on the checkpoints it wrote (whole image, --scale 96), and the
same images stored as RGB PNGs, which are converted to L and give the same label maps."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

GREY = ['--dataset', 'BBBC039V1']


def _checkpoint(d):
    import torch
    return torch.load(os.path.join(d, 'checkpoints', 'checkpoint.pth.tar'), map_location='cpu', weights_only=False)


def _initial(name, seed=2022):
    """the model train.main starts from: chooseModel under the entry's seed (train.py:75-81)"""
    import torch
    from cdnet_amd import utils
    from cdnet_amd.options import Options
    opt = Options(isTrain=True).parse(GREY + ['--model-name', name] + (['--direction', '0'] if name == 'UNet' else []))
    torch.manual_seed(seed)
    np.random.seed(seed)
    return utils.chooseModel(opt)


@pytest.mark.parametrize('name,stem,n_out', [('UNet2RevA1_vgg16', 'child0.weight', 11), ('UNet', 'down1.down_conv.0.weight', 3)])
def test_train_entry_on_synthetic_grey_tiles(tmp_path, name, stem, n_out):
    from cdnet_amd import train
    d = str(tmp_path / 'exp')
    res = train.main(GREY + ['--synthetic', '2', '--epochs', '1', '--batch-size', '2', '--save-dir', d, '--model-name', name]
                     + (['--direction', '0'] if name == 'UNet' else []))
    assert len(res) == n_out and np.isfinite(res).all()
    ck = _checkpoint(d)
    m0 = _initial(name)
    assert list(ck['state_dict'].keys()) == ['module.' + k for k in m0.state_dict().keys()]      # the reference's keys (nn.DataParallel's)
    w0, w1 = m0.state_dict()[stem], ck['state_dict']['module.' + stem]
    assert tuple(w1.shape) == tuple(w0.shape) and w1.shape[1] == 1
    assert not np.array_equal(w1.float().numpy(), w0.float().numpy())                             # the one-channel stem was stepped
    if name == 'UNet2RevA1_vgg16':
        assert np.array_equal(ck['state_dict']['module.backbone.0.weight'].numpy(), m0.state_dict()['backbone.0.weight'].numpy())


def _grey_dataset(root, rgb=False, n=3, size=64, seed=4):
    """<root>/images/{train,test1}/im<k>.png (mode L, or the same bytes as RGB), weight_maps/train/im<k>_weight.png,
    labels/train/im<k>_label.png (instance ids, mode L) and labels/test1_ins/im<k>.npy"""
    from PIL import Image
    from cdnet_amd import synth
    rs = np.random.RandomState(seed)
    for sub in ('images/train', 'images/test1', 'weight_maps/train', 'labels/train', 'labels/test1', 'labels/test1_ins'):
        (root / sub).mkdir(parents=True, exist_ok=True)
    for k in range(n):
        inst = synth.ellipse_instances(size, size, 8, rs, 5, 9, 5).astype(np.int32)
        img = np.clip(40 + 150 * (inst > 0) + rs.randint(-30, 31, (size, size)), 0, 255).astype(np.uint8)
        im = Image.fromarray(np.dstack([img] * 3)) if rgb else Image.fromarray(img)
        assert im.mode == ('RGB' if rgb else 'L')
        for sub in ('train', 'test1'):
            im.save(root / 'images' / sub / ('im%d.png' % k))
        Image.fromarray(np.full((size, size), 20, np.uint8)).save(root / 'weight_maps' / 'train' / ('im%d_weight.png' % k))
        Image.fromarray(inst.astype(np.uint8)).save(root / 'labels' / 'train' / ('im%d_label.png' % k))
        np.save(root / 'labels' / 'test1_ins' / ('im%d.npy' % k), inst)


def _rows(path, skip):
    lines = [ln for ln in open(path).read().split('\n') if ln]
    return [ln.replace(':', '\t').split('\t')[0] for ln in lines[skip:]]


def test_train_and_both_test_entries_on_l_pngs(tmp_path, monkeypatch):
    from PIL import Image
    from cdnet_amd import test, test_dam, train
    root = tmp_path / 'data' / 'BBBC039V1'
    _grey_dataset(root)
    monkeypatch.chdir(tmp_path)
    common = GREY + ['--device-augment', '--epochs', '1', '--batch-size', '2', '--input-size', '64']
    dam, unet = str(tmp_path / 'dam'), str(tmp_path / 'unet')
    res = train.main(common + ['--save-dir', dam])
    assert len(res) == 11 and np.isfinite(res).all()
    res = train.main(common + ['--save-dir', unet, '--model-name', 'UNet', '--direction', '0'])
    assert len(res) == 3 and np.isfinite(res).all()
    assert _checkpoint(dam)['state_dict']['module.child0.weight'].shape[1] == 1
    folders = ['--img-dir', str(root / 'images' / 'test1'), '--label-dir', str(root / 'labels' / 'test1')]

    def run_dam(out, imgs=folders, extra=()):
        test_dam.main(GREY + imgs + ['--model-path', os.path.join(dam, 'checkpoints', 'checkpoint.pth.tar'), '--save-dir', str(out)] + list(extra))
        assert _rows(out / 'test_results.txt', 0) == ['Average', 'im0', 'im1', 'im2']
        return [np.asarray(Image.open(out / ('im%d_seg.tiff' % k))) for k in range(3)]

    def run_unet(out, imgs=folders, extra=()):
        test.main(GREY + imgs + ['--model-name', 'UNet', '--direction', '0', '--model-path', os.path.join(unet, 'checkpoints', 'checkpoint.pth.tar'),
                                 '--save-dir', str(out)] + list(extra))
        assert _rows(out / 'test1_result.txt', 1) == ['Average', 'im0', 'im1', 'im2']
        return [np.asarray(Image.open(out / 'test1_segmentation' / ('b5_im%d_seg.tiff' % k))) for k in range(3)]
    maps_dam, maps_unet = run_dam(tmp_path / 'o_dam'), run_unet(tmp_path / 'o_unet')
    assert all(m.shape == (64, 64) for m in maps_dam + maps_unet)
    # --scale 96: the images go up as bytes, are resized in mode L on the device, and the label maps come back at 64 x 64
    assert all(m.shape == (64, 64) for m in run_dam(tmp_path / 's_dam', extra=['--scale', '96']) + run_unet(tmp_path / 's_unet', extra=['--scale', '96']))
    # the same images stored as RGB PNGs are converted to L: the same label maps
    rgb = tmp_path / 'rgb'
    _grey_dataset(rgb, rgb=True)
    rgb_folders = ['--img-dir', str(rgb / 'images' / 'test1'), '--label-dir', str(rgb / 'labels' / 'test1')]
    for a, b in zip(maps_dam + maps_unet, run_dam(tmp_path / 'r_dam', rgb_folders) + run_unet(tmp_path / 'r_unet', rgb_folders)):
        assert np.array_equal(a, b)
