"""cdnet_amd.augment on the host: the PIL-backed path against the Pillow fixtures, the restated geometry's identities, the draws'
ranges and frequencies, and the ABI entries' argument checks (no GPU needed)."""
import ctypes as C

import numpy as np
import pytest

from cdnet_amd import augment
from cdnet_amd.augment import Params, Recipe


def _params(**kw):
    p = dict(color=(1.0, 1.0, 1.0, 1.0), hflip=0, vflip=0, minv=augment.IDENTITY, alpha=0.0, sigma=50.0, seed=0, filter=0, y0=0, x0=0)
    p.update(kw)
    return Params(**p)


def _sample(H, W, seed=0):
    rs = np.random.RandomState(seed)
    return (rs.randint(0, 256, (H, W, 3)).astype(np.uint8), rs.randint(0, 256, (H, W)).astype(np.uint8),
            rs.randint(0, 256, (H, W)).astype(np.uint8))


def test_host_path_equals_the_pillow_fixtures(golden):
    g = golden('augment')
    factors = g['factors']
    for k in range(3):
        src = g['src%d' % k]
        for j, f in enumerate(factors):
            assert np.array_equal(augment.colour_chain(src, tuple(float(v) for v in f)), g['chain%d' % k][j]), (k, j)
        for code in (1, 2, 3):
            assert np.array_equal(augment.apply_filter(src, code), g['filt%d' % k][code - 1]), (k, code)
        # the whole host chain with only colour or only a filter is the fixture too
        H, W = src.shape[:2]
        w, lab = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
        out = augment.augment_host(src, w, lab, _params(color=tuple(float(v) for v in factors[2])), max(H, W))
        assert np.array_equal(out[0][:H, :W], g['chain%d' % k][2])
        out = augment.augment_host(src, w, lab, _params(filter=2), max(H, W))
        assert np.array_equal(out[0][:H, :W], g['filt%d' % k][1])


def test_identity_affine_and_zero_alpha_is_the_identity():
    img, w, lab = _sample(40, 53)
    pts = augment.affine_points(40, 53)
    minv = augment.affine_inverse(pts, pts.copy())
    assert np.allclose(minv, augment.IDENTITY, atol=1e-12)
    out = augment.augment_host(img, w, lab, _params(minv=minv), 32)
    assert np.array_equal(out[0], img[:32, :32]) and np.array_equal(out[1], w[:32, :32]) and np.array_equal(out[2], lab[:32, :32])


def test_flips_and_integer_shift():
    img, w, lab = _sample(30, 37, 1)
    out = augment.augment_host(img, w, lab, _params(hflip=1, vflip=1), 40)
    assert np.array_equal(out[0][:30, :37], img[::-1, ::-1]) and np.array_equal(out[2][:30, :37], lab[::-1, ::-1])
    assert not out[1][30:].any() and not out[1][:, 37:].any()                     # zero pad, weight 0
    # M maps source (x, y) to destination (x + 3, y - 2): its inverse reads source (x - 3, y + 2); the rest is a zero border
    out = augment.augment_host(img, w, lab, _params(minv=(1.0, 0.0, -3.0, 0.0, 1.0, 2.0)), 30)
    want = np.zeros_like(w[:30, :30])
    want[:28, 3:] = w[2:30, :27]
    assert np.array_equal(out[1], want)
    assert not out[0][28:].any() and not out[0][:, :3].any()


def test_given_field_moves_pixels_by_its_rounded_value():
    img, w, lab = _sample(24, 24, 2)
    p = _params(alpha=1.0, sigma=1.0)
    FS = 16 + 2 * augment.HALO
    field = np.zeros((2, FS, FS), np.float32)
    field[0] = 1.49                     # dx: rounds to 1
    field[1] = -0.5                     # dy: half-to-even -> q.y - 0 at even, -1 at odd rows
    out = augment.augment_host(img, w, lab, p, 16, field=field)
    ys = np.arange(16)
    ry = np.rint(ys.astype(np.float32) - np.float32(0.5)).astype(int)
    want = np.where((ry >= 0)[:, None], w[np.clip(ry, 0, None)][:, 1:17], 0)
    assert np.array_equal(out[1], want)


def test_field_window_is_scipy_of_the_noise():
    from scipy.ndimage import gaussian_filter
    p = _params(alpha=30.0, sigma=4.0, seed=77, y0=5, x0=3)
    f = augment.field_window(p, 40, 50, 20)
    full = gaussian_filter(augment.field_noise(77, 1, 40, 50), 4.0, mode='reflect', truncate=4.0) * np.float32(30.0)
    assert np.array_equal(f[1][augment.HALO - 5 + 5:, augment.HALO - 3 + 3:][:26, :26], full[5:31, 3:29])
    assert not f[0][:1].any()                                                   # row y0 - 6 < 0 is outside
    n = augment.field_noise(77, 0, 64, 64)
    assert n.dtype == np.float32 and n.min() >= -1 and n.max() < 1 and abs(float(n.mean())) < 0.05


def test_draws_have_the_stated_ranges_and_frequencies():
    rs = np.random.RandomState(0)
    rec = Recipe(size=256)
    ps = [augment.draw_params(rs, 1000, 900, rec) for _ in range(4000)]
    col = np.array([p.color for p in ps])
    assert col.min() >= 0.5 and col.max() < 1.5
    for attr in ('hflip', 'vflip'):
        assert abs(np.mean([getattr(p, attr) for p in ps]) - 0.5) < 0.03
    freq = np.bincount([p.filter for p in ps], minlength=4) / len(ps)
    assert np.all(np.abs(freq - 0.25) < 0.03), freq
    assert all(0 <= p.y0 <= 744 and 0 <= p.x0 <= 644 for p in ps)
    assert all(p.alpha == 1.0 and p.sigma == 50.0 for p in ps)
    small = augment.draw_params(rs, 100, 120, rec)
    assert small.y0 == 0 and small.x0 == 0
    off = augment.draw_params(rs, 300, 300, Recipe(size=64, color=False, hflip=False, vflip=False, elastic=False, choose_aug=False))
    assert off.color == (1.0, 1.0, 1.0, 1.0) and off.minv == augment.IDENTITY and off.alpha == 0.0 and off.filter == 0


def test_recipe_from_the_default_transform():
    from cdnet_amd.options import Options
    opt = Options(isTrain=True).parse([])
    r = Recipe.from_transform(opt.transform['train'])
    assert r.color and r.hflip and r.vflip and r.elastic and r.choose_aug and r.size == opt.train['input_size']
    assert (r.elastic_alpha, r.elastic_sigma, r.elastic_alpha_affine) == (1.0, 50.0, 50.0)


def test_abi_struct_mirror_and_argument_checks():
    from cdnet_amd import _lib
    lib = _lib.load()
    assert lib.cdnet_abi_sizeof(b'cdnet_aug_sample') == C.sizeof(augment.AugSample)
    assert lib.cdnet_abi_version() == 5
    assert lib.cdnet_augment_workspace_bytes(0, 256, 0) == 0
    assert lib.cdnet_augment_workspace_bytes(16, 256, 5000) == 0
    assert lib.cdnet_augment_workspace_bytes(2, 64, 8) > lib.cdnet_augment_workspace_bytes(2, 64, 0) > 0
    fake = C.c_void_p(4096)                                                     # never dereferenced: every call below fails validation
    t = (augment.AugSample * 1)()
    t[0].img = t[0].weight = t[0].label = 4096
    t[0].H, t[0].W, t[0].img_stride, t[0].weight_stride, t[0].label_stride = 100, 100, 300, 100, 100
    t[0].sigma = 50.0

    def call(B=1, size=64, label_i32=0, table=t, ws_bytes=1 << 30):
        return lib.cdnet_augment_batch(fake, table, B, size, None, fake, ws_bytes, fake, fake, fake, label_i32, fake, None, None)
    assert lib.cdnet_augment_batch(None, t, 1, 64, None, fake, 1 << 30, fake, fake, fake, 0, fake, None, None) == 1
    assert b'null pointer' in lib.cdnet_last_error()
    assert call(B=0) == 1 and call(size=0) == 1 and call(label_i32=1) == 1
    t[0].filter = 4
    assert call() == 1 and b'filter code' in lib.cdnet_last_error()
    t[0].filter = 0
    t[0].y0 = 37
    assert call() == 1 and b'crop origin' in lib.cdnet_last_error()
    t[0].y0 = 0
    t[0].alpha, t[0].sigma = 1.0, 0.0
    assert call() == 1 and b'sigma' in lib.cdnet_last_error()
    t[0].sigma = 50.0
    assert call(ws_bytes=16) == 2 and b'workspace' in lib.cdnet_last_error()
    t[0].img_stride = 10
    assert call() == 1 and b'stride' in lib.cdnet_last_error()


def test_tile_batches_host_augmentation(tmp_path):
    """TileBatches(augment=True) on the host: crops of the recipe's size, padded sources keep weight 0 in the pad, and a constant label
    crop is re-drawn"""
    from test_data_folder import make_dataset
    from cdnet_amd.data_folder import DataFolder, TileBatches
    dirs = make_dataset(tmp_path, n=2, size=(50, 70))
    ds = DataFolder(dirs, ['weight.png', 'label.png'], [3, 1, 3])
    tf = {'random_color': 1, 'horizontal_flip': True, 'vertical_flip': True, 'random_elastic': [6, 15], 'random_chooseAug': 1,
          'random_crop': 64, 'label_encoding': [3, 2, 1], 'to_tensor': 1}
    tb = TileBatches(ds, tf, 2, 'cpu', seed=1, augment=True)
    for i in range(len(tb.items)):
        img, w, lab = tb._draw(*tb.items[i])
        assert img.shape == (64, 64, 3) and w.shape == (64, 64) and lab.shape[:2] == (64, 64)
        assert len(np.unique(lab if lab.ndim == 2 else lab[:, :, 0])) > 1
        assert not w[50:].any() and not w[:, 70:].any()
