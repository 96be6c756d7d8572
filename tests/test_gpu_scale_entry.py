"""GPU tests of the 'scale' test transform through the two inference entries (cdnet_amd.test, cdnet_amd.test_dam): the image is resized
on the device, the cleaned mask resized back, and `final` is at the original size - equal in every pixel to the device's own `small` stage
of the unrestored run on the Pillow-resized image, then Pillow's mode-L resize, `> 127.5`, scipy's 8-connected labelling and disk dilation."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

MEAN, STD = np.array([0.6, 0.5, 0.55]), np.array([0.2, 0.25, 0.22])
# (ori_h, ori_w, scale, image seed, tta): 70 x 53 up to 96 -> 126 x 96; 150 x 120 down to 64 -> 80 x 64
IMAGES = [(70, 53, 96, 11, 0), (150, 120, 64, 12, 1)]


def _image(H, W, seed):
    """a smooth seeded RGB image (noise would give the network nothing to segment)"""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.zeros((H, W, 3))
    for _ in range(10):
        cy, cx, r = rs.uniform(0, H), rs.uniform(0, W), rs.uniform(4, 12)
        img += np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * r * r))[..., None] * rs.uniform(0.3, 1.0, 3)
    img = img / img.max() * 200 + rs.uniform(0, 55, (H, W, 3))
    return img.astype(np.uint8)


def _balance(m, conv):
    """seeded weights alone leave class 1 (inside) below the other two almost everywhere: its bias moves by the median margin over the two
    test images at the network's sizes, so that about half of the pixels are inside and the chain has objects to clean, resize and label"""
    import torch
    from cdnet_amd import utils
    margins = []
    with torch.no_grad():
        for ori_h, ori_w, scale, seed, _ in IMAGES:
            x = _host_transform(_image(ori_h, ori_w, seed), scale).cuda()
            mask = utils.split_forward_views(m, x, max(x.shape[1:]), 0, (0,), 9)[0][0]
            margins.append((mask[1] - torch.maximum(mask[0], mask[2])).flatten())
        conv.bias[1] -= torch.cat(margins).median()


def _unet(seed=1):
    import torch
    from cdnet_amd.models.unet import UNet
    torch.manual_seed(seed)
    m = UNet(num_classes=3).cuda().eval()
    _balance(m, m.final_conv)
    return m


def _dam(seed=0):
    import torch
    from cdnet_amd.models.dam.model_unet_rev1 import Unet
    torch.manual_seed(seed)
    m = Unet(backbone_name='vgg16_bn', pretrained=False, classes=3).cuda().eval()
    _balance(m, m.mask_conv)
    return m


def _opt(kind, extra=()):
    from cdnet_amd.options import Options
    base = ['--model-name', 'UNet', '--direction', '0'] if kind == 'unet' else []
    opt = Options(isTrain=False).parse(base + list(extra))
    opt.transform['test']['normalize'] = [MEAN, STD]
    return opt


def _host_transform(img_u8, size=None):
    """Scale on Pillow itself, then the host conversion of the entries: / 255.0 and (x - mean) / std in float32"""
    import torch
    from PIL import Image
    from cdnet_amd.my_transforms_direction import Scale
    pil, = (Scale(size) if size else (lambda t: t))((Image.fromarray(img_u8),))
    x = torch.from_numpy(np.asarray(pil, dtype=np.float32) / 255.0).permute(2, 0, 1).contiguous()
    return (x - torch.tensor(MEAN, dtype=torch.float32).view(3, 1, 1)) / torch.tensor(STD, dtype=torch.float32).view(3, 1, 1)


def _disk(r):
    y, x = np.mgrid[-r:r + 1, -r:r + 1]
    return (y * y + x * x) <= r * r


def _expected(small, ori_h, ori_w, radius):
    from PIL import Image
    from scipy import ndimage as ndi
    back = np.asarray(Image.fromarray(small * np.uint8(255), 'L').resize((ori_w, ori_h), Image.BILINEAR)) > 127.5
    lab, n = ndi.label(back, structure=np.ones((3, 3), int))
    return ndi.grey_dilation(lab, footprint=_disk(radius)).astype(np.int32), n


def _small_stage(kind, model, x, opt):
    """the `small` stage (holes filled, small objects removed) of the unrestored run at the network's size"""
    from cdnet_amd import pipeline, postproc
    if kind == 'dam':
        r = pipeline.infer_image(model, x.cuda(), opt, want_stages=True)
        return r['small'].cpu().numpy(), r
    r = pipeline.infer_image_mask(model, x.cuda(), opt)
    cc = postproc.cc_chain(r['pred'][None], 1, opt.post['min_area'], opt.post['radius'], want_stages=True)
    return cc['small'][0].cpu().numpy(), r


@pytest.fixture(scope='module')
def models():
    return {'unet': _unet(), 'dam': _dam()}


def test_scaled_input_has_the_bits_of_the_host_transform():
    """resize, / 255.0 and (x - mean) / std on the device against Pillow and the host's float32 operations, every byte value included"""
    import torch
    from cdnet_amd import pipeline
    ramp = np.arange(70 * 53 * 3, dtype=np.int64).reshape(70, 53, 3)
    img = ((ramp * 7 + ramp // 53) % 256).astype(np.uint8)
    assert len(np.unique(img)) == 256
    for transform, size in (({'scale': 96, 'to_tensor': 1, 'normalize': [MEAN, STD]}, 96), ({'to_tensor': 1, 'normalize': [MEAN, STD]}, None),
                            ({'scale': 53, 'to_tensor': 1}, None)):
        x, restore = pipeline.scaled_input(torch.from_numpy(img), transform)
        want = _host_transform(img, size)
        if 'normalize' not in transform:
            want = torch.from_numpy(np.asarray(img, dtype=np.float32) / 255.0).permute(2, 0, 1).contiguous()
        assert restore == ((70, 53) if size else None)
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
        assert np.array_equal(x.cpu().numpy().view(np.uint32), want.numpy().view(np.uint32))
    # the Scale step for an image already converted and normalised at its original size (what test_dam.main hands over): same bits
    for transform in ({'scale': 96, 'to_tensor': 1, 'normalize': [MEAN, STD]}, {'scale': 96, 'to_tensor': 1}):
        plain = _host_transform(img) if 'normalize' in transform else torch.from_numpy(np.asarray(img, dtype=np.float32) / 255.0).permute(2, 0, 1).contiguous()
        x, restore = pipeline.scale_transformed(plain.cuda(), transform)
        want, _ = pipeline.scaled_input(torch.from_numpy(img), transform)
        assert restore == (70, 53) and tuple(x.shape) == (3, 126, 96)
        assert np.array_equal(x.cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32))
    same, restore = pipeline.scale_transformed(_host_transform(img).cuda(), {'scale': 53, 'to_tensor': 1, 'normalize': [MEAN, STD]})
    assert restore is None and tuple(same.shape) == (3, 70, 53)


@pytest.mark.parametrize('kind', ['unet', 'dam'])
@pytest.mark.parametrize('spec', IMAGES, ids=lambda s: '{}x{}_to_{}'.format(*s[:3]))
def test_process_image_restores_the_original_size(models, kind, spec):
    import torch
    from cdnet_amd import test, test_dam
    ori_h, ori_w, scale, seed, tta = spec
    model, entry = models[kind], (test if kind == 'unet' else test_dam)
    img = _image(ori_h, ori_w, seed)
    opt = _opt(kind, ['--scale', str(scale), '--tta', str(tta)])
    x = _host_transform(img, scale)
    assert tuple(x.shape[1:]) == ((126, 96) if scale == 96 else (80, 64))
    small, unrestored = _small_stage(kind, model, x, opt)
    want, n = _expected(small, ori_h, ori_w, opt.post['radius'])
    assert n >= 1, 'the seeded network found nothing: the comparison would be empty'
    from cdnet_amd import pipeline
    plain = _host_transform(img)                         # converted and normalised at the original size: the Scale step runs on the device
    if kind == 'unet':
        runs = [lambda: entry.process_image(model, img, opt), lambda: entry.process_image(model, torch.from_numpy(img), opt),
                lambda: entry.process_image(model, plain, opt), lambda: entry.process_image(model, x, opt, ori_size=(ori_h, ori_w))]
    else:
        def scaled_by_the_caller():
            r = pipeline.infer_image(model, x.cuda(), opt, restore=(ori_h, ori_w))
            return dict(final=r['final'].cpu().numpy(), count=r['count'], pred=r['pred'].cpu().numpy())
        runs = [lambda: entry.process_image(model, plain, opt), scaled_by_the_caller]
    for run in runs:
        got = run()
        assert got['final'].shape == (ori_h, ori_w) and got['final'].dtype == np.int32
        assert np.array_equal(got['final'], want)
        assert got['count'] == n
        assert np.array_equal(got['pred'], unrestored['pred'].cpu().numpy())        # (at the scaled size, where the reference saves it)


@pytest.mark.parametrize('kind', ['unet', 'dam'])
def test_scale_equal_to_the_smaller_edge_changes_nothing(models, kind):
    from cdnet_amd import test, test_dam
    model, entry = models[kind], (test if kind == 'unet' else test_dam)
    img = _image(70, 53, 11)
    plain = entry.process_image(model, _host_transform(img), _opt(kind, ['--tta', '0']))
    same = entry.process_image(model, img if kind == 'unet' else _host_transform(img), _opt(kind, ['--tta', '0', '--scale', '53']))
    assert np.array_equal(same['final'], plain['final']) and same['count'] == plain['count']
    assert np.array_equal(same['pred'], plain['pred'])


@pytest.mark.parametrize('kind', ['unet', 'dam'])
def test_scale_with_postproc_1_is_refused(models, kind, tmp_path):
    from cdnet_amd import pipeline, test, test_dam
    model, entry = models[kind], (test if kind == 'unet' else test_dam)
    opt = _opt(kind, ['--tta', '0', '--scale', '96', '--postproc', '1'])
    with pytest.raises(ValueError, match='postproc 1'):
        entry.process_image(model, _host_transform(_image(70, 53, 11)), opt)
    _, args = _folder(tmp_path, model)
    with pytest.raises(ValueError, match='postproc 1'):
        entry.main((['--model-name', 'UNet', '--direction', '0'] if kind == 'unet' else []) + args + ['--postproc', '1'])
    infer = pipeline.infer_image_mask if kind == 'unet' else pipeline.infer_image
    with pytest.raises(ValueError, match='postproc 1'):
        infer(model, _host_transform(_image(70, 53, 11), 96).cuda(), postproc=1, restore=(70, 53))


def _folder(tmp_path, model):
    """two synthetic images with labels, the model's weights as a reference-format checkpoint"""
    import torch
    from PIL import Image
    from test_data_folder import make_dataset
    from cdnet_amd import checkpoint
    make_dataset(tmp_path, n=2, size=(70, 53), seed=5, sub='test1')
    imgs = []
    for k in range(2):                                   # (make_dataset's images are white noise: overwrite them with smooth ones)
        imgs.append(_image(70, 53, 20 + k))
        Image.fromarray(imgs[k]).save(tmp_path / 'images' / 'test1' / ('im%d.png' % k))
    ck = str(tmp_path / 'weights.pth.tar')
    torch.save({'state_dict': checkpoint.model_state(model)}, ck)
    args = ['--img-dir', str(tmp_path / 'images' / 'test1'), '--label-dir', str(tmp_path / 'labels' / 'test1'), '--model-path', ck,
            '--save-dir', str(tmp_path / 'out'), '--scale', '96', '--tta', '0']
    return imgs, args


def test_test_main_with_scale(models, tmp_path):
    from PIL import Image
    from cdnet_amd import test, utils
    imgs, args = _folder(tmp_path, models['unet'])
    avg = test.main(['--model-name', 'UNet', '--direction', '0'] + args)
    assert avg is not None and list(avg) == test.HEADER and all(np.isfinite(v) for v in avg.values()), avg
    lines = open(tmp_path / 'out' / 'test1_result.txt').read().split('\n')
    assert sorted(ln.split(':')[0] for ln in lines[3:] if ln) == ['im0', 'im1']
    opt = _opt('unet', ['--scale', '96', '--tta', '0'])
    del opt.transform['test']['normalize']               # (main found no mean_std.npy: it does not normalise)
    for k in range(2):
        seg = np.asarray(Image.open(tmp_path / 'out' / 'test1_segmentation' / ('b5_im%d_seg.tiff' % k))).astype(np.int32)
        prob = np.asarray(Image.open(tmp_path / 'out' / 'test1_prob_maps' / ('b5_im%d_prob_inside.png' % k)))
        want = test.process_image(models['unet'], imgs[k], opt)
        assert seg.shape == (70, 53) and prob.shape == (126, 96)
        assert np.array_equal(seg, utils.measure_label(want['final']))          # (the saved map is the relabelled one, test.py:339, 379)
        assert np.array_equal(seg > 0, want['final'] > 0)


def test_test_dam_main_with_scale(models, tmp_path):
    import torch
    from PIL import Image
    from cdnet_amd import test_dam
    imgs, args = _folder(tmp_path, models['dam'])
    avg = test_dam.main(args)
    assert avg is not None and all(np.isfinite(v) for v in avg.values()), avg
    rows = [ln.split('\t')[0] for ln in open(tmp_path / 'out' / 'test_results.txt').read().split('\n') if ln]
    assert rows == ['Average:', 'im0', 'im1']
    opt = _opt('dam', ['--scale', '96', '--tta', '0'])
    del opt.transform['test']['normalize']
    for k in range(2):
        seg = np.asarray(Image.open(tmp_path / 'out' / ('im%d_seg.tiff' % k))).astype(np.int32)
        plain = torch.from_numpy(np.asarray(imgs[k], dtype=np.float32) / 255.0).permute(2, 0, 1).contiguous()    # (main's conversion)
        want = test_dam.process_image(models['dam'], plain, opt)
        assert seg.shape == (70, 53)
        assert np.array_equal(seg, want['final'])
