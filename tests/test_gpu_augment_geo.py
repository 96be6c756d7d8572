"""cdnet_augment_batch_geo on the MI355X: random_resize, random_affine and random_rotation against the host implementation
(cdnet_amd.augment.augment_host: PIL for the affine, numpy for the restated OpenCV rules) bit for bit, the entry with every step off
against cdnet_augment_batch, the displacement field under a rotation against scipy, and the loader / training entry with every key."""
import numpy as np
import pytest
import torch

from cdnet_amd import augment
from cdnet_amd.augment import Params, Recipe, Source

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SIZE = 64
ALL = ('random_resize,random_color,random_affine,horizontal_flip,vertical_flip,random_elastic,random_rotation,random_chooseAug,'
       'random_crop,label_encoding,to_tensor')


def _sources(rs):
    """the shapes of test_gpu_augment.py: one smaller than the crop (zero pad), odd shapes; 3-class u8 labels"""
    out = []
    for H, W in ((150, 170), (40, 52), (97, 131), (128, 128)):
        img = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
        img = np.clip(img.astype(int) // 3 + 80 + (np.arange(W) % 50)[None, :, None], 0, 255).astype(np.uint8)
        w = rs.randint(1, 30, (H, W)).astype(np.uint8)
        lab = np.where(rs.rand(H, W) < 0.3, 255, 0).astype(np.uint8)
        out.append((img, w, lab))
    return out


def _check_against_host(items, ps, label_dtype=torch.uint8):
    srcs = [Source(*it, DEV) for it in items]
    img, weight, label, varied, field, origin = augment.augment_batch(srcs, ps, SIZE, want_field=True, want_origin=True)
    torch.cuda.synchronize()
    assert label.dtype == label_dtype
    for b, (it, p) in enumerate(zip(items, ps)):
        f = field[b].cpu().numpy() if p.alpha != 0 else None
        want = augment.augment_host(it[0], it[1], it[2], p, SIZE, field=f, origin=tuple(origin[b]))
        got_img = img[b].cpu().numpy()
        want_img = (want[0].astype(np.float32) / np.float32(255)).transpose(2, 0, 1)
        assert np.array_equal(got_img, want_img), (b, p, int((got_img != want_img).sum()))
        assert np.array_equal(weight[b].cpu().numpy(), want[1]), (b, p)
        assert np.array_equal(label[b].cpu().numpy(), want[2].astype(label.cpu().numpy().dtype)), (b, p)
        assert varied[b].item() == int(len(np.unique(want[2])) > 1), (b, p)
    return field


def _with_angle(p, H, W, angle):
    Hr, Wr = p.dims(H, W)
    p.angle, p.rinv = angle, tuple(augment.rotation_inverse(angle, Hr, Wr))
    p.fy0, p.fx0, p.fedge = augment.field_box(p, Hr, Wr, SIZE)
    return p


def _draws(rs, items, rec, n, alpha_alternates=True):
    ps = []
    for k in range(n):
        it = items[k % len(items)]
        p = augment.draw_params(rs, it[1].shape[0], it[1].shape[1], rec)
        p.filter = k % 4
        if alpha_alternates:
            p.alpha, p.sigma = (0.0, 50.0) if (k // 4) % 2 == 0 else (30.0, 4.0)
        ps.append(p)
    return [items[k % len(items)] for k in range(n)], ps


@pytest.fixture(scope='module')
def items():
    return _sources(np.random.RandomState(11))


def test_resize_alone(items):
    rs = np.random.RandomState(1)
    for scale in ((1.0, 1.0), (2.0, 2.0), (1.0, 2.0)):               # scale 1, scale 2, random in [1, 2]
        rec = Recipe(size=SIZE, color=False, hflip=False, vflip=False, elastic=False, choose_aug=False, resize=scale)
        its, ps = _draws(rs, items, rec, 8, alpha_alternates=False)
        _check_against_host(its, ps)
        if scale == (1.0, 1.0):
            assert all((p.Hr, p.Wr) == it[1].shape for it, p in zip(its, ps))
    # with the colour chain: the Contrast mean and Sharpness's neighbours are the resized image's
    rec = Recipe(size=SIZE, hflip=False, vflip=False, elastic=False, choose_aug=False, resize=(1.0, 2.0))
    _check_against_host(*_draws(rs, items, rec, 8, alpha_alternates=False))
    # (40, 52) at scale 1.2 is 48 x 62: still smaller than the crop, zero-padded
    rec = Recipe(size=SIZE, resize=(1.2, 1.2))
    its, ps = _draws(rs, [items[1]], rec, 4)
    assert all((p.Hr, p.Wr) == (48, 62) for p in ps)
    _check_against_host(its, ps)


def test_affine_alone(items):
    rs = np.random.RandomState(2)
    rec = Recipe(size=SIZE, color=False, hflip=False, vflip=False, elastic=False, choose_aug=False, affine=0.3)
    _check_against_host(*_draws(rs, items, rec, 8, alpha_alternates=False))
    rec = Recipe(size=SIZE, affine=0.5)                                  # with colour, flips, elastic (alpha 0 / 30) and every filter
    _check_against_host(*_draws(rs, items, rec, 16))


def test_rotation_alone(items):
    rs = np.random.RandomState(3)
    rec = Recipe(size=SIZE, color=False, hflip=False, vflip=False, elastic=False, choose_aug=False, rotation=True)
    its, ps = _draws(rs, items, rec, 8, alpha_alternates=False)
    for p, it, angle in zip(ps, its, (0.0, 90.0, -90.0, 0.0, 90.0, -90.0)):    # angles 0 and +-90; the last two stay random
        _with_angle(p, it[1].shape[0], it[1].shape[1], angle)
    _check_against_host(its, ps)
    # the field matters under a rotation: alpha 30 / sigma 4, elastic affine on, every filter
    rec = Recipe(size=SIZE, color=False, rotation=True)
    its, ps = _draws(rs, items, rec, 16)
    for k, angle in ((4, 0.0), (5, 90.0), (6, -90.0)):
        _with_angle(ps[k], its[k][1].shape[0], its[k][1].shape[1], angle)
    field = _check_against_host(its, ps)
    assert float(field.abs().max()) > 0.5                               # alpha 30 moves pixels


def test_all_nine_steps(items):
    rs = np.random.RandomState(4)
    rec = Recipe(size=SIZE, resize=(1.0, 2.0), affine=0.3, rotation=True)
    its, ps = _draws(rs, items, rec, 16)
    assert {p.hflip for p in ps} == {0, 1} and {p.vflip for p in ps} == {0, 1} and {p.filter for p in ps} == {0, 1, 2, 3}
    _check_against_host(its, ps)
    its, ps = _draws(rs, items, rec, 8, alpha_alternates=False)         # the reference's field (alpha 1, sigma 50)
    _check_against_host(its, ps)
    # a batch that mixes samples with and without each step
    mixed = [Recipe(size=SIZE), Recipe(size=SIZE, rotation=True), Recipe(size=SIZE, resize=(1.0, 2.0)), Recipe(size=SIZE, affine=0.3)]
    ps = [augment.draw_params(rs, it[1].shape[0], it[1].shape[1], rec) for it, rec in zip(items, mixed)]
    for p in ps:
        p.alpha, p.sigma = 30.0, 4.0
    _check_against_host(items, ps)


def test_all_nine_steps_with_instance_labels():
    from cdnet_amd import synth
    rs = np.random.RandomState(5)
    its = []
    for H, W in ((120, 90), (70, 70)):
        inst = synth.ellipse_instances(H, W, 10, rs, 5, 10, 6).astype(np.int32)
        its.append((rs.randint(0, 256, (H, W, 3)).astype(np.uint8), np.full((H, W), 20, np.uint8), inst))
    rec = Recipe(size=SIZE, elastic_alpha=30.0, elastic_sigma=4.0, resize=(1.0, 2.0), affine=0.3, rotation=True)
    ps = [augment.draw_params(rs, it[1].shape[0], it[1].shape[1], rec) for it in its]
    _check_against_host(its, ps, torch.int32)


def test_geo_table_with_every_step_off_is_the_legacy_entry(items):
    from cdnet_amd import _lib
    rs = np.random.RandomState(6)
    its, ps = _draws(rs, items, Recipe(size=SIZE), 8)
    srcs = [Source(*it, DEV) for it in its]
    old = augment.augment_batch(srcs, ps, SIZE, want_field=True)
    B = len(ps)
    table = (augment.AugSample * B)()
    geo = (augment.AugGeo * B)()
    for t, g, src, p in zip(table, geo, srcs, ps):
        t.minv[:] = p.minv
        t.img, t.weight, t.label = src.img.data_ptr(), src.weight.data_ptr(), src.label.data_ptr()
        t.H, t.W, t.img_stride, t.weight_stride, t.label_stride, t.label_i32 = src.H, src.W, 3 * src.W, src.W, src.W, 0
        t.color[:] = p.color
        t.hflip, t.vflip, t.filter, t.y0, t.x0 = p.hflip, p.vflip, p.filter, p.y0, p.x0
        t.alpha, t.sigma, t.seed = p.alpha, p.sigma, p.seed
        g.Hr, g.Wr, g.fy0, g.fx0, g.flags = src.H, src.W, p.y0 - 6, p.x0 - 6, 0
        g.paff[:] = augment.IDENTITY
        g.rinv[:] = augment.IDENTITY
    FS = SIZE + 12
    lib = _lib.load()
    ws = torch.empty((lib.cdnet_augment_geo_workspace_bytes(B, SIZE, 16, FS),), dtype=torch.uint8, device=DEV)
    up = lambda a: torch.frombuffer(bytearray(bytes(a)), dtype=torch.uint8).to(DEV)
    table_dev, geo_dev = up(table), up(geo)
    image = torch.empty((B, 3, SIZE, SIZE), dtype=torch.float32, device=DEV)
    weight = torch.empty((B, SIZE, SIZE), dtype=torch.uint8, device=DEV)
    label = torch.empty((B, SIZE, SIZE), dtype=torch.uint8, device=DEV)
    varied = torch.empty((B,), dtype=torch.int32, device=DEV)
    field = torch.zeros((B, 2, FS, FS), dtype=torch.float32, device=DEV)
    _lib.call('cdnet_augment_batch_geo', _lib.ptr(table_dev), table, _lib.ptr(geo_dev), geo, FS, B, SIZE, None, _lib.ptr(ws), ws.numel(),
              _lib.ptr(image), _lib.ptr(weight), _lib.ptr(label), 0, _lib.ptr(varied), _lib.ptr(field), _lib.stream_ptr())
    torch.cuda.synchronize()
    for got, want in zip((image, weight, label, varied, field), old):
        assert torch.equal(got, want)
    assert float(field.abs().max()) > 0.5


def test_field_under_rotation_is_scipy_of_the_device_noise():
    from scipy.ndimage import gaussian_filter
    rs = np.random.RandomState(3)
    H, W = 150, 170
    img = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    z = np.ones((H, W), np.uint8)
    base = dict(color=(1.0,) * 4, hflip=0, vflip=0, minv=augment.IDENTITY, filter=0, angle=37.0, rinv=tuple(augment.rotation_inverse(37.0, H, W)))
    ps = [Params(alpha=1.0, sigma=50.0, seed=123, y0=80, x0=60, **base), Params(alpha=30.0, sigma=4.0, seed=9, y0=3, x0=0, **base)]
    out = augment.augment_batch([Source(img, z, z, DEV)] * 2, ps, SIZE, want_field=True, want_origin=True)
    field, origin = out[4].cpu().numpy(), out[5]
    FS = field.shape[-1]
    assert SIZE + 12 < FS <= int(np.ceil(np.sqrt(2) * (SIZE + 12))) + 4
    for b, p in enumerate(ps):
        assert tuple(origin[b]) == augment.field_box(p, H, W, SIZE)[:2]
        for k in range(2):
            full = gaussian_filter(augment.field_noise(p.seed, k, H, W).astype(np.float64), p.sigma, mode='reflect', truncate=4.0) * p.alpha
            ys, xs = np.arange(origin[b][0], origin[b][0] + FS), np.arange(origin[b][1], origin[b][1] + FS)
            iy, ix = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
            assert iy.sum() > SIZE and ix.sum() > SIZE
            got = field[b, k][np.ix_(iy, ix)]
            want = full[np.ix_(ys[iy], xs[ix])]
            assert np.abs(got - want).max() <= 1e-5 * max(1.0, p.alpha), (b, k, np.abs(got - want).max())
            assert not field[b, k][~iy].any() and not field[b, k][:, ~ix].any()


def _check_zero_fill(img, weight):
    """img [B, 3, s, s] (0 = black), weight [B, 1, s, s] of sources whose stored weight is non-zero everywhere and whose stored pixels
    the colour chain never turns black: Z = (weight == 0) is exactly what a pad or a border zero-filled.  The filters act on the image
    alone and reach 6 px (GaussianBlur), so the image is black wherever Z holds the whole 13 x 13 neighbourhood (pixels beyond the crop
    count as unknown); and a black pixel lies in Z or within 2 px of it (MedianFilter 3 x 3, BLUR's 5 x 5 ring without its centre)."""
    import torch.nn.functional as F
    Z = (weight == 0).float()
    black = (img == 0).all(1, keepdim=True)
    deep = F.max_pool2d(F.pad(1 - Z, (6, 6, 6, 6), value=1.0), 13, 1) == 0
    assert bool(black[deep].all())
    near = F.max_pool2d(Z, 5, 1, 2) > 0
    assert bool(near[black].all())
    return int(Z.sum()), int(deep.sum())


def _mid_grey_images(img_dir, n, size):
    """overwrite the dataset's images with noise in [120, 140].  With factors in [0.5, 1.5) Color keeps a pixel in [105, 155], Brightness b
    scales that, Contrast about a mean near 130 b leaves at least 92 b, Sharpness at least 55 b > 27: no stored pixel turns black, so a
    black output pixel was zero-filled"""
    import os
    from PIL import Image
    rs = np.random.RandomState(8)
    for k in range(n):
        Image.fromarray(rs.randint(120, 141, size + (3,)).astype(np.uint8)).save(os.path.join(img_dir, 'im%d.png' % k))


def test_tile_batches_and_train_entry_with_every_key(tmp_path, monkeypatch):
    from test_data_folder import make_dataset
    from cdnet_amd import train
    from cdnet_amd.data_folder import DataFolder, TileBatches
    from cdnet_amd.options import Options
    root = tmp_path / 'data' / Options(isTrain=True).dataset
    dirs = make_dataset(root, n=5, size=(50, 70), seed=3)                # the source weight is 20 everywhere
    _mid_grey_images(dirs[0], 5, (50, 70))
    monkeypatch.chdir(tmp_path)
    ds = DataFolder(dirs, ['weight.png', 'label.png'], [3, 1, 3])
    tf = dict(Options(isTrain=True).parse(['--input-size', '64', '--trans-train', ALL]).transform['train'])
    assert 'random_rotation' in tf and 'random_resize' in tf and 'random_affine' in tf
    tb = TileBatches(ds, tf, 2, DEV, seed=1, augment=True)
    assert tb.recipe.resize == (1.0, 2.0) and tb.recipe.affine == 0.3 and tb.recipe.rotation
    seen, padded = 0, 0
    for img, weight, label, point, direction in tb:
        B = img.shape[0]
        seen += B
        assert img.shape == (B, 3, 64, 64) and img.dtype == torch.float32 and 0 <= float(img.min()) and float(img.max()) <= 1
        assert weight.shape == (B, 1, 64, 64) and weight.dtype == torch.uint8 and int(weight.max()) <= 20
        assert label.shape == (B, 1, 64, 64) and label.dtype == torch.int64 and set(np.unique(label.cpu().numpy())) <= {0, 127, 255}
        assert all(len(torch.unique(label[b])) > 1 for b in range(B))   # the constant-label re-draw rule
        assert point.shape == (B, 64, 64) and direction.dtype == torch.uint8 and int(direction.max()) <= 8
        padded += _check_zero_fill(img, weight)[0]
    assert seen == 5 and padded > 0
    res = train.main(['--device-augment', '--trans-train', ALL, '--epochs', '2', '--batch-size', '2', '--input-size', '64',
                      '--save-dir', str(tmp_path / 'exp')])
    assert len(res) == 11 and np.isfinite(res).all()
