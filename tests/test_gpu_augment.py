"""cdnet_augment_batch on the MI355X: the colour chain and the filters against the Pillow fixtures, the whole device chain against the
host implementation (cdnet_amd.augment.augment_host) bit for bit, the device field against scipy, the re-draw rule, and the loader /
training entry with --device-augment."""
import numpy as np
import pytest
import torch

from cdnet_amd import augment
from cdnet_amd.augment import Params, Source

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def _params(**kw):
    p = dict(color=(1.0, 1.0, 1.0, 1.0), hflip=0, vflip=0, minv=augment.IDENTITY, alpha=0.0, sigma=50.0, seed=0, filter=0, y0=0, x0=0)
    p.update(kw)
    return Params(**p)


def _to_u8(img):
    """device image f32 [3, s, s] (/ 255) -> u8 [s, s, 3]: v / 255 in fp32 is exact to invert by rounding"""
    return np.rint(img.permute(1, 2, 0).cpu().numpy() * 255.0).astype(np.uint8)


def test_colour_chain_and_filters_equal_the_pillow_fixtures(golden):
    g = golden('augment')
    for k in range(3):
        src = g['src%d' % k]
        H, W = src.shape[:2]
        s = max(H, W)
        z = np.zeros((H, W), np.uint8)
        z[0, 0] = 1
        source = Source(src, z, z, DEV)
        ps = [_params(color=tuple(float(v) for v in f)) for f in g['factors']] + [_params(filter=c) for c in (1, 2, 3)]
        img, weight, label, varied = augment.augment_batch([source] * len(ps), ps, s)
        torch.cuda.synchronize()
        want = list(g['chain%d' % k]) + list(g['filt%d' % k])
        for j, w in enumerate(want):
            got = _to_u8(img[j])
            assert np.array_equal(got[:H, :W], w), (k, j, int((got[:H, :W] != w).sum()))
            assert not got[H:].any() and not got[:, W:].any()
        assert varied.tolist() == [1] * len(ps)


def _sources(rs):
    """mixed sizes: one smaller than the crop (zero pad), odd shapes; 3-class u8 labels"""
    out = []
    for H, W in ((150, 170), (40, 52), (97, 131), (128, 128)):
        img = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
        img = np.clip(img.astype(int) // 3 + 80 + (np.arange(W) % 50)[None, :, None], 0, 255).astype(np.uint8)
        w = rs.randint(1, 30, (H, W)).astype(np.uint8)
        lab = np.where(rs.rand(H, W) < 0.3, 255, 0).astype(np.uint8)
        out.append((img, w, lab))
    return out


def _check_against_host(items, ps, size, label_dtype):
    srcs = [Source(*it, DEV) for it in items]
    img, weight, label, varied, field = augment.augment_batch(srcs, ps, size, want_field=True)
    torch.cuda.synchronize()
    for b, (it, p) in enumerate(zip(items, ps)):
        f = field[b].cpu().numpy() if p.alpha != 0 else None
        want = augment.augment_host(it[0], it[1], it[2], p, size, field=f)
        got_img = img[b].cpu().numpy()
        want_img = (want[0].astype(np.float32) / np.float32(255)).transpose(2, 0, 1)
        assert np.array_equal(got_img, want_img), (b, p, int((got_img != want_img).sum()))
        assert np.array_equal(weight[b].cpu().numpy(), want[1]), b
        assert label.dtype == label_dtype and np.array_equal(label[b].cpu().numpy(), want[2].astype(label.cpu().numpy().dtype)), b
        assert varied[b].item() == int(len(np.unique(want[2])) > 1), b
    return field


def test_device_equals_host_on_random_parameters():
    rs = np.random.RandomState(11)
    items = _sources(rs)
    size = 96
    from cdnet_amd.augment import Recipe
    rec = Recipe(size=size)
    ps = []
    for k in range(16):                                     # every filter, both flips, random colour / affine, alpha 0 and 30 (sigma 4)
        it = items[k % len(items)]
        p = augment.draw_params(rs, it[1].shape[0], it[1].shape[1], rec)
        p.filter = k % 4
        p.alpha, p.sigma = (0.0, 50.0) if k % 2 == 0 else (30.0, 4.0)
        ps.append(p)
    items = [items[k % len(items)] for k in range(16)]
    field = _check_against_host(items, ps, size, torch.uint8)
    assert float(field.abs().max()) > 0.5                  # alpha 30 moves pixels
    # the default recipe (alpha 1, sigma 50) too
    ps = [augment.draw_params(rs, it[1].shape[0], it[1].shape[1], rec) for it in items[:4]]
    _check_against_host(items[:4], ps, size, torch.uint8)


def test_device_equals_host_with_instance_labels():
    rs = np.random.RandomState(5)
    items = []
    for H, W in ((120, 90), (70, 70)):
        from cdnet_amd import synth
        inst = synth.ellipse_instances(H, W, 10, rs, 5, 10, 6).astype(np.int32)
        items.append((rs.randint(0, 256, (H, W, 3)).astype(np.uint8), np.full((H, W), 20, np.uint8), inst))
    rec = augment.Recipe(size=64, elastic_alpha=30.0, elastic_sigma=4.0)
    ps = [augment.draw_params(rs, it[1].shape[0], it[1].shape[1], rec) for it in items]
    _check_against_host(items, ps, 64, torch.int32)


def test_device_field_is_scipy_of_the_device_noise():
    from scipy.ndimage import gaussian_filter
    rs = np.random.RandomState(3)
    H, W, size = 180, 140, 64
    img = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    z = np.ones((H, W), np.uint8)
    ps = [_params(alpha=1.0, sigma=50.0, seed=123, y0=100, x0=60), _params(alpha=30.0, sigma=4.0, seed=9, y0=3, x0=0)]
    srcs = [Source(img, z, z, DEV)] * 2
    out = augment.augment_batch(srcs, ps, size, want_field=True)
    field = out[4].cpu().numpy()
    for b, p in enumerate(ps):
        for k in range(2):
            full = gaussian_filter(augment.field_noise(p.seed, k, H, W).astype(np.float64), p.sigma, mode='reflect', truncate=4.0) * p.alpha
            FS = size + 2 * augment.HALO
            ys, xs = np.arange(p.y0 - 6, p.y0 - 6 + FS), np.arange(p.x0 - 6, p.x0 - 6 + FS)
            iy, ix = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
            got = field[b, k][np.ix_(iy, ix)]
            want = full[np.ix_(ys[iy], xs[ix])]
            assert np.abs(got - want).max() <= 1e-5 * max(1.0, p.alpha), (b, k, np.abs(got - want).max())
            assert not field[b, k][~iy].any() and not field[b, k][:, ~ix].any()


def test_redraw_rule_on_a_mostly_constant_label(tmp_path):
    """a source whose label is foreground in one corner only: most draws give a constant crop, flagged and re-drawn by the loader"""
    from PIL import Image
    from cdnet_amd.data_folder import DataFolder, TileBatches
    H, W = 200, 200
    dirs = [tmp_path / d / 'train' for d in ('images', 'weight_maps', 'labels')]
    for d in dirs:
        d.mkdir(parents=True)
    lab = np.zeros((H, W, 3), np.uint8)
    lab[..., 2] = 255
    lab[5:65, 5:65, 0] = 255
    lab[5:65, 5:65, 2] = 0
    Image.fromarray(np.random.RandomState(0).randint(0, 256, (H, W, 3)).astype(np.uint8)).save(dirs[0] / 'a.png')
    Image.fromarray(np.full((H, W), 20, np.uint8)).save(dirs[1] / 'a_weight.png')
    Image.fromarray(lab).save(dirs[2] / 'a_label.png')
    ds = DataFolder([str(d) for d in dirs], ['weight.png', 'label.png'], [3, 1, 3])
    tf = {'random_color': 1, 'horizontal_flip': True, 'vertical_flip': True, 'random_elastic': [6, 15], 'random_chooseAug': 1,
          'random_crop': 64, 'label_encoding': [3, 2, 1], 'to_tensor': 1}
    tb = TileBatches(ds, tf, 1, DEV, seed=2, augment=True, elastic={'elastic_alpha_affine': 0.0})
    flags = []
    for _ in range(40):
        p = augment.draw_params(tb.rs, H, W, tb.recipe)
        flags.append(augment.augment_batch([tb.sources[0]], [p], 64)[3].item())
    assert flags.count(0) > 20                             # most single draws are constant ...
    for _ in range(3):
        img, weight, label, point, direction = next(iter(tb))
        assert len(torch.unique(label)) > 1                # ... the loader re-draws them


def test_tile_batches_augment_end_to_end_and_train_entry(tmp_path, monkeypatch):
    from test_data_folder import make_dataset
    from cdnet_amd import train
    from cdnet_amd.data_folder import DataFolder, TileBatches
    from cdnet_amd.options import Options
    root = tmp_path / 'data' / Options(isTrain=True).dataset
    dirs = make_dataset(root, n=5, size=(150, 170), seed=3)
    monkeypatch.chdir(tmp_path)
    ds = DataFolder(dirs, ['weight.png', 'label.png'], [3, 1, 3])
    tf = dict(Options(isTrain=True).parse(['--input-size', '64']).transform['train'])
    tb = TileBatches(ds, tf, 2, DEV, seed=1, augment=True)
    seen = 0
    for img, weight, label, point, direction in tb:
        B = img.shape[0]
        seen += B
        assert img.shape == (B, 3, 64, 64) and img.dtype == torch.float32 and 0 <= float(img.min()) and float(img.max()) <= 1
        assert weight.shape == (B, 1, 64, 64) and weight.dtype == torch.uint8 and int(weight.max()) <= 20
        assert label.shape == (B, 1, 64, 64) and set(np.unique(label.cpu().numpy())) <= {0, 127, 255}
        assert all(len(torch.unique(label[b])) > 1 for b in range(B))
        assert point.shape == (B, 64, 64) and direction.dtype == torch.uint8 and int(direction.max()) <= 8
    assert seen == 5
    res = train.main(['--device-augment', '--epochs', '2', '--batch-size', '2', '--input-size', '64', '--save-dir', str(tmp_path / 'exp')])
    assert len(res) == 11 and np.isfinite(res).all()
