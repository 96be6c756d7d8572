"""Grey-scale datasets (in_c = 1) without a GPU: the options, chooseModel's one-channel Unet family (set_input_channels: per-instance
UNUSED_PREFIXES, unchanged state-dict keys), the flat optimiser layout (child0.* stepped, backbone.0.* behind n_used, with and without
encoder_freeze), img_loader's conversion to mode L, augment_host on L against Pillow's own results (tests/golden/augment_grey.npz) and the
argument checks of cdnet_augment_batch_c / cdnet_augment_batch_geo_c."""
import ctypes as C

import numpy as np
import pytest

from cdnet_amd import augment
from cdnet_amd.augment import Params
from cdnet_amd.options import Options

UNET_FAMILY = ('UNet2RevA1_vgg16', 'UNet_vgg16', 'model_unet_MandD', 'model_unet_MandD4', 'model_unet_MandD16', 'model_unet_MandDandP')


def _params(**kw):
    p = dict(color=(1.0, 1.0, 1.0, 1.0), hflip=0, vflip=0, minv=augment.IDENTITY, alpha=0.0, sigma=50.0, seed=0, filter=0, y0=0, x0=0)
    p.update(kw)
    return Params(**p)


def test_options_give_one_channel_for_the_grey_dataset_only():
    assert Options(isTrain=True).parse(['--dataset', 'BBBC039V1']).model['in_c'] == 1
    assert Options(isTrain=False).parse(['--dataset', 'BBBC039V1']).model['in_c'] == 1
    assert Options(isTrain=True).parse([]).model['in_c'] == 3
    assert Options(isTrain=False).parse([]).model['in_c'] == 3
    assert Options(isTrain=True).parse(['--dataset', 'CPM2017']).model['in_c'] == 3


def _opt(name, grey=True, extra=()):
    direction = [] if name not in ('UNet_vgg16', 'UNet') else ['--direction', '0']
    return Options(isTrain=True).parse((['--dataset', 'BBBC039V1'] if grey else []) + ['--model-name', name, '--pretrained', '0'] + direction + list(extra))


@pytest.mark.parametrize('name', UNET_FAMILY)
def test_choose_model_sets_the_one_channel_stem(name):
    from cdnet_amd import utils
    m1, m3 = utils.chooseModel(_opt(name)), utils.chooseModel(_opt(name, grey=False))
    assert m1.input_channels == 1 and m3.input_channels == 3
    cls = type(m1).UNUSED_PREFIXES
    assert 'child0.' in cls and m3.UNUSED_PREFIXES == cls and 'UNUSED_PREFIXES' not in vars(m3)      # the class attribute stays
    assert m1.UNUSED_PREFIXES == tuple(p for p in cls if p != 'child0.') + ('backbone.0.',)
    assert list(m1.state_dict().keys()) == list(m3.state_dict().keys())
    assert [tuple(v.shape) for v in m1.state_dict().values()] == [tuple(v.shape) for v in m3.state_dict().values()]
    # the runtime's first encoder layer is child0 with backbone child '1' as its BatchNorm; everything behind is unchanged
    l1, l3 = m1.conv_layers(), m3.conv_layers()
    assert l1[0].name == 'child0' and l1[0].weight is m1.child0.weight and l1[0].bias is m1.child0.bias and l1[0].bn is m1.backbone[1]
    assert l3[0].name == 'backbone.0' and [l.name for l in l1[1:]] == [l.name for l in l3[1:]]
    with pytest.raises(ValueError):
        m1.set_input_channels(2)
    m1.set_input_channels(3)                                         # back: the class tuple again
    assert m1.UNUSED_PREFIXES == cls and m1.conv_layers()[0].name == 'backbone.0'


def test_hrnet_refuses_one_channel():
    from cdnet_amd import utils
    with pytest.raises(ValueError, match='three-channel'):
        utils.chooseModel(_opt('HRNet18_rev1'))


@pytest.mark.parametrize('freeze', [0, 1])
@pytest.mark.parametrize('name', ['UNet2RevA1_vgg16', 'UNet_vgg16'])
def test_flat_state_steps_child0_and_not_backbone0(name, freeze):
    from cdnet_amd import utils
    from cdnet_amd.optim import FlatState
    m = utils.chooseModel(_opt(name, extra=['--encoder-freeze', str(freeze)]))
    assert m.child0.weight.requires_grad and m.child0.bias.requires_grad              # encoder_freeze freezes backbone.* only
    assert m.backbone[0].weight.requires_grad == (not freeze)
    fs = FlatState(m)
    for n in ('child0.weight', 'child0.bias'):
        off, sz = fs.offsets[n]
        assert off + sz <= fs.n_used, n
    for n in ('backbone.0.weight', 'backbone.0.bias', 'child_conv1.weight'):
        assert fs.offsets[n][0] >= fs.n_used, n
    stepped = {n for n in fs.order if fs.offsets[n][0] < fs.n_used}
    if freeze:
        assert not any(n.startswith('backbone.') for n in stepped) and 'backbone.0.weight' not in fs.frozen
        assert 'backbone.1.weight' in fs.frozen
    else:
        assert 'backbone.1.weight' in stepped and 'backbone.3.weight' in stepped
    # the three-channel model of the same name: the other way round
    f3 = FlatState(utils.chooseModel(_opt(name, grey=False)))
    assert f3.offsets['child0.weight'][0] >= f3.n_used and f3.offsets['backbone.0.weight'][0] + f3.offsets['backbone.0.weight'][1] <= f3.n_used
    m.set_input_channels(1)                                          # the count it has: allowed ...
    m._trainer_bound = True
    with pytest.raises(RuntimeError, match='trainer'):               # ... another one after a trainer was bound: the rule of freeze_encoder
        m.set_input_channels(3)


def test_img_loader_converts_to_l_and_refuses_sixteen_bits(tmp_path):
    from PIL import Image
    from cdnet_amd.data_folder import DataFolder, img_loader
    rs = np.random.RandomState(0)
    rgb = rs.randint(0, 256, (20, 24, 3)).astype(np.uint8)
    Image.fromarray(rgb).save(tmp_path / 'rgb.png')
    Image.fromarray(rgb[..., 0]).save(tmp_path / 'l.png')
    Image.fromarray(np.dstack([rgb, np.full((20, 24), 200, np.uint8)])).save(tmp_path / 'rgba.png')
    Image.fromarray(rgb[..., 0]).convert('P').save(tmp_path / 'p.png')
    Image.fromarray((rgb[..., 0].astype(np.uint16) * 200)).save(tmp_path / 'deep.png')
    assert Image.open(tmp_path / 'deep.png').mode in ('I;16', 'I')
    want = np.asarray(Image.fromarray(rgb).convert('L'))
    got = img_loader(str(tmp_path / 'rgb.png'), 1, grey=True)
    assert got.mode == 'L' and np.array_equal(np.asarray(got), want)
    assert np.array_equal(np.asarray(img_loader(str(tmp_path / 'rgba.png'), 1, grey=True)), want)
    for f in ('l.png', 'p.png'):
        got = img_loader(str(tmp_path / f), 1, grey=True)
        assert got.mode == 'L' and np.array_equal(np.asarray(got), rgb[..., 0]), f
    with pytest.raises(ValueError, match='deep.png'):
        img_loader(str(tmp_path / 'deep.png'), 1, grey=True)
    assert img_loader(str(tmp_path / 'l.png'), 3).mode == 'RGB'      # three channels: as before
    # the weight-map slot of every dataset (one channel, no `grey`) reads the file as it always did
    assert img_loader(str(tmp_path / 'rgb.png'), 1).mode == 'RGB' and img_loader(str(tmp_path / 'p.png'), 1).mode == 'P'
    assert img_loader(str(tmp_path / 'deep.png'), 1).mode in ('I;16', 'I')
    # a one-channel DataFolder hands [H, W] images to TileBatches, whose batches are [B, 1, s, s]
    from cdnet_amd.data_folder import TileBatches
    dirs = [tmp_path / d / 'train' for d in ('images', 'weight_maps', 'labels')]
    for d in dirs:
        d.mkdir(parents=True)
    lab = np.zeros((20, 24, 3), np.uint8)
    lab[..., 2] = 255
    lab[4:12, 4:12, 0], lab[4:12, 4:12, 2] = 255, 0
    Image.fromarray(rgb).save(dirs[0] / 'a.png')
    Image.fromarray(np.full((20, 24, 3), 20, np.uint8)).save(dirs[1] / 'a_weight.png')       # an RGB weight map stays RGB (channel 0 is taken)
    Image.fromarray(lab).save(dirs[2] / 'a_label.png')
    ds = DataFolder([str(d) for d in dirs], ['weight.png', 'label.png'], [1, 1, 3])
    assert [im.mode for im in ds.load(0)] == ['L', 'RGB', 'RGB']
    tb = TileBatches(ds, {'random_crop': 16, 'to_tensor': 1, 'normalize': [[0.5, 0.1, 0.2], [0.25, 0.3, 0.4]]}, 1, 'cpu', seed=0)
    assert tb.items[0][0].shape == (20, 24) and np.array_equal(tb.items[0][0], want)
    img, weight, lab0 = tb._host_batch([0])
    assert tuple(img.shape) == (1, 1, 16, 16) and img.dtype.is_floating_point
    lo, hi = (0 - 0.5) / 0.25, (1 - 0.5) / 0.25                      # the first entries of mean and std
    assert lo <= float(img.min()) and float(img.max()) <= hi and float(img.max()) > 1.0


def test_augment_host_on_l_equals_pillow(golden):
    g = golden('augment_grey')
    factors = g['factors']
    for k in range(3):
        src = g['src%d' % k]
        assert src.ndim == 2 and src.shape[0] <= 48 and src.shape[1] <= 56
        H, W = src.shape
        w, lab = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
        for j, f in enumerate(factors):
            f = tuple(float(v) for v in f)
            assert np.array_equal(augment.colour_chain(src, f), g['chain%d' % k][j]), (k, j)
            out = augment.augment_host(src, w, lab, _params(color=f), max(H, W))
            assert out[0].shape == (max(H, W),) * 2 and np.array_equal(out[0][:H, :W], g['chain%d' % k][j]), (k, j)
            assert not out[0][H:].any() and not out[0][:, W:].any()
            # the Color factor is drawn and ignored: any value gives the same image
            for c in (0.5, 1.5):
                assert np.array_equal(augment.colour_chain(src, (c,) + f[1:]), g['chain%d' % k][j]), (k, j, c)
        for i, c in enumerate(g['color_only']):
            assert np.array_equal(g['colour%d' % k][i], src)                        # Pillow itself: the identity
            assert np.array_equal(augment.colour_chain(src, (float(c), 1.0, 1.0, 1.0)), src), (k, c)
        for code in (1, 2, 3):
            assert np.array_equal(augment.apply_filter(src, code), g['filt%d' % k][code - 1]), (k, code)
            out = augment.augment_host(src, w, lab, _params(filter=code), max(H, W))
            assert np.array_equal(out[0][:H, :W], g['filt%d' % k][code - 1]), (k, code)


def test_recipe_draws_the_same_numbers_for_both_channel_counts():
    rec = augment.Recipe(size=32, resize=(1, 2), affine=0.3, rotation=True)
    a = augment.draw_params(np.random.RandomState(4), 60, 70, rec)
    b = augment.draw_params(np.random.RandomState(4), 60, 70, rec)
    assert a == b and len(a.color) == 4                                              # (the draw never sees the image: one stream)
    rs = np.random.RandomState(1)
    grey = rs.randint(0, 256, (60, 70)).astype(np.uint8)
    w, lab = np.full((60, 70), 7, np.uint8), rs.randint(0, 3, (60, 70)).astype(np.uint8)
    p = augment.draw_params(np.random.RandomState(9), 60, 70, augment.Recipe(size=32, elastic_alpha=20.0, elastic_sigma=3.0, affine=0.2))
    out = augment.augment_host(grey, w, lab, p, 32)
    assert out[0].shape == (32, 32) and out[1].shape == (32, 32) and out[2].shape == (32, 32)
    # geometry does not depend on the plane count: the weight and label crops are those of the RGB call on the stacked image
    out3 = augment.augment_host(np.dstack([grey] * 3), w, lab, p, 32)
    assert np.array_equal(out[1], out3[1]) and np.array_equal(out[2], out3[2])


def test_new_entries_check_channels_and_null_tables_before_any_hip_call():
    from cdnet_amd import _lib
    lib = _lib.load()
    assert lib.cdnet_abi_version() == 5
    fake = C.c_void_p(4096)                                                          # never dereferenced: every call below fails validation
    t = (augment.AugSample * 1)()
    t[0].img = t[0].weight = t[0].label = 4096
    t[0].H, t[0].W, t[0].img_stride, t[0].weight_stride, t[0].label_stride = 100, 100, 100, 100, 100
    t[0].sigma = 50.0
    geo = (augment.AugGeo * 1)()
    geo[0].Hr, geo[0].Wr = 100, 100

    def plain(ch, dev_table=fake, host_table=t):
        return lib.cdnet_augment_batch_c(dev_table, host_table, 1, 64, None, fake, 1 << 30, fake, fake, fake, 0, fake, None, None, ch)

    def geo_call(ch, g=fake, gh=geo, dev_table=fake):
        return lib.cdnet_augment_batch_geo_c(dev_table, t, g, gh, 76, 1, 64, None, fake, 1 << 30, fake, fake, fake, 0, fake, None, None, ch)
    for ch in (0, 2, 4):
        assert plain(ch) == 1 and b'channels' in lib.cdnet_last_error(), ch
        assert geo_call(ch) == 1 and b'channels' in lib.cdnet_last_error(), ch
        assert geo_call(ch, g=None, gh=None) == 1 and b'channels' in lib.cdnet_last_error(), ch
    for ch in (1, 3):
        assert plain(ch, dev_table=None) == 1 and b'null pointer' in lib.cdnet_last_error(), ch
        assert plain(ch, host_table=None) == 1 and b'null pointer' in lib.cdnet_last_error(), ch
        assert geo_call(ch, g=None, gh=None) == 1 and b'null pointer' in lib.cdnet_last_error(), ch
        assert geo_call(ch, dev_table=None) == 1 and b'null pointer' in lib.cdnet_last_error(), ch
    # a one-channel row stride of W bytes passes where RGB needs 3 W: the stride check follows the channel count
    t[0].y0 = 37                                                                     # (a later check fails instead: nothing is launched)
    assert plain(1) == 1 and b'crop origin' in lib.cdnet_last_error()
    assert plain(3) == 1 and b'stride' in lib.cdnet_last_error()


def test_grey_transformed_is_pillows_convert_l():
    """pipeline.infer_image's conversion of an image the test_dam entry read as RGB: the bits of loading it with convert('L')"""
    import torch
    from PIL import Image
    from cdnet_amd import pipeline
    rs = np.random.RandomState(0)
    rgb = rs.randint(0, 256, (37, 41, 3)).astype(np.uint8)
    grey = np.dstack([rgb[..., 0]] * 3)
    opt = Options(isTrain=False).parse(['--dataset', 'BBBC039V1'])
    for norm in (None, [[0.7, 0.5, 0.6], [0.2, 0.25, 0.3]]):
        if norm:
            opt.transform['test']['normalize'] = norm
        for img in (rgb, grey):
            x3 = pipeline.host_input(Image.fromarray(img), opt.transform['test'], 3)
            want = pipeline.host_input(Image.fromarray(img), opt.transform['test'], 1)
            got = pipeline.grey_transformed(x3, opt)
            assert tuple(got.shape) == (1, 37, 41) and torch.equal(got, want)
        assert pipeline.grey_transformed(want, opt) is want                                   # one plane already: untouched
    rgb_opt = Options(isTrain=False).parse([])
    assert pipeline.grey_transformed(x3, rgb_opt) is x3 and pipeline.grey_transformed(x3, None) is x3   # in_c = 3: untouched
