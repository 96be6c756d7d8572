"""random_resize, random_affine and random_rotation on the host: the restated Pillow affine against Pillow itself, the rotation and
resize identities, the three planes moving together through augment_host, the draws, the field window's containment, --trans-train and
the argument checks of cdnet_augment_batch_geo (no GPU needed)."""
import ctypes as C

import numpy as np
import pytest

from cdnet_amd import augment
from cdnet_amd.augment import Params, Recipe

ALL = ('random_resize,random_color,random_affine,horizontal_flip,vertical_flip,random_elastic,random_rotation,random_chooseAug,'
       'random_crop,label_encoding,to_tensor')


def _params(**kw):
    p = dict(color=(1.0, 1.0, 1.0, 1.0), hflip=0, vflip=0, minv=augment.IDENTITY, alpha=0.0, sigma=50.0, seed=0, filter=0, y0=0, x0=0)
    p.update(kw)
    return Params(**p)


def _paff(rs, v, W, H):
    a, b, d, e = 1 + 2 * v * (rs.rand() - 0.5), 2 * v * (rs.rand() - 0.5), 2 * v * (rs.rand() - 0.5), 1 + 2 * v * (rs.rand() - 0.5)
    return (a, b, -a * W / 2 - b * H / 2 + W / 2, d, e, -d * W / 2 - e * H / 2 + H / 2)


def test_pil_affine_restatement_equals_pillow():
    from PIL import Image
    rs = np.random.RandomState(1)
    sizes = list(range(5, 141, 2))                                       # odd sizes 5 .. 139
    cases = [(int(rs.choice(sizes)), int(rs.choice(sizes)), None) for _ in range(240)]
    cases += [(33, 51, (1.25, 0.0, 0.0, 0.0, 0.75, 0.0)), (140, 7, (0.7, 0.0, 0.0, 0.0, 1.3, 0.0))]      # pure scale
    cases += [(33, 51, (1.0, 0.0, 0.0, 0.0, 1.0, 0.0))]                  # bound 0: the only b = d = 0 draw (Pillow's scaling path)
    for n, (H, W, m) in enumerate(cases):
        m = m or _paff(rs, 0.3, W, H)
        kind = n % 3
        if kind == 0:
            src = rs.randint(0, 256, (H, W)).astype(np.uint8)            # L
        elif kind == 1:
            src = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)         # RGB
        else:
            src = rs.randint(0, 2 ** 20, (H, W)).astype(np.int32)        # I (instance labels)
        im = Image.fromarray(src)
        assert im.mode == ('L', 'RGB', 'I')[kind]
        want = np.asarray(im.transform((W, H), Image.AFFINE, m))
        y, x = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
        yin, xin, ok = augment.pil_affine_source(m, H, W, y, x)
        got = np.where(ok if src.ndim == 2 else ok[..., None], src[np.where(ok, yin, 0), np.where(ok, xin, 0)], 0)
        assert np.array_equal(got, want), (n, H, W, m, int((got != want).sum()))


@pytest.mark.parametrize('n', [8, 20, 33])
def test_rotation_identities(n):
    src = np.random.RandomState(n).randint(1, 256, (n, n)).astype(np.uint8)
    y, x = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')

    def rot(angle):
        Y, X, ok = augment.warp_source(augment.rotation_inverse(angle, n, n), n, n, y, x)
        return np.where(ok, src[np.where(ok, Y, 0), np.where(ok, X, 0)], 0)
    assert np.array_equal(rot(0.0), src)
    want = np.zeros_like(src)
    want[1:] = np.rot90(src, 1)[:-1]                                     # +90: rot90 shifted one row down, row 0 zero
    assert np.array_equal(rot(90.0), want)
    want = np.zeros_like(src)
    want[:, 1:] = np.rot90(src, -1)[:, :-1]                              # -90: rot90(-1) shifted one column right, column 0 zero
    assert np.array_equal(rot(-90.0), want)


def test_resize_identities():
    rs = np.random.RandomState(2)
    for H, W in ((7, 10), (33, 20)):
        src = rs.randint(0, 256, (H, W)).astype(np.uint8)
        up = src[augment.resize_index(2 * H, H)][:, augment.resize_index(2 * W, W)]
        assert np.array_equal(up, np.repeat(np.repeat(src, 2, 0), 2, 1))
        assert np.array_equal(augment.resize_index(H, H), np.arange(H)) and np.array_equal(augment.resize_index(W, W), np.arange(W))
        for s in (1.0, 1.37, 1.999, 2.0, 0.6):
            assert augment.resize_dims(H, W, s) == (int(H * s), int(W * s))
            idx = augment.resize_index(int(H * s), H)
            assert len(idx) == int(H * s) and idx.min() == 0 and idx.max() <= H - 1 and np.all(np.diff(idx) >= 0)


def _coded(H, W):
    """planes that name their source pixel: label = y * W + x + 1 (i32), weight = label % 251, image channels from the same code"""
    lab = (np.arange(H * W, dtype=np.int32) + 1).reshape(H, W)
    w = (lab % 251).astype(np.uint8)
    img = np.stack([(lab % 256), (lab // 256) % 256, (lab * 7) % 256], -1).astype(np.uint8)
    return img, w, lab


def _moves_together(out, src):
    img, w, lab = src
    o_img, o_w, o_lab = out
    on = o_lab > 0
    code = o_lab[on] - 1
    sy, sx = code // lab.shape[1], code % lab.shape[1]
    assert np.array_equal(o_w[on], w[sy, sx]) and np.array_equal(o_img[on], img[sy, sx])
    assert not o_w[~on].any() and not o_img[~on].any()
    return on


def test_augment_host_each_step_alone_moves_the_three_planes_together():
    H, W, size = 50, 66, 40
    src = _coded(H, W)
    rs = np.random.RandomState(3)
    # resize by 1.5: dims, and pixel (y, x) reads source (floor(y / 1.5), floor(x / 1.5))
    Hr, Wr = augment.resize_dims(H, W, 1.5)
    out = augment.augment_host(*src, _params(scale=1.5, Hr=Hr, Wr=Wr, y0=20, x0=31), size)
    assert _moves_together(out, src).all()
    yy = np.minimum(np.floor(np.arange(20, 60) * (1.0 / (Hr / H))).astype(int), H - 1)
    xx = np.minimum(np.floor(np.arange(31, 71) * (1.0 / (Wr / W))).astype(int), W - 1)
    assert np.array_equal(out[2], src[2][yy][:, xx])
    # affine alone: equals the restated rule, planes together, some zero border
    m = _paff(rs, 0.3, W, H)
    out = augment.augment_host(*src, _params(paff=m, y0=5, x0=10), size)
    on = _moves_together(out, src)
    y, x = np.meshgrid(np.arange(5, 45), np.arange(10, 50), indexing='ij')
    yin, xin, ok = augment.pil_affine_source(m, H, W, y, x)
    assert np.array_equal(on, ok) and np.array_equal(out[2][ok], src[2][yin[ok], xin[ok]])
    # rotation alone
    out = augment.augment_host(*src, _params(angle=37.0, rinv=augment.rotation_inverse(37.0, H, W), y0=0, x0=0), size)
    on = _moves_together(out, src)
    assert 0 < on.sum() < on.size
    Y, X, ok = augment.warp_source(augment.rotation_inverse(37.0, H, W), H, W, *np.meshgrid(np.arange(40), np.arange(40), indexing='ij'))
    assert np.array_equal(on, ok) and np.array_equal(out[2][ok], src[2][Y[ok], X[ok]])
    # all three with flips and a displacement field: still one source pixel behind the three planes
    rec = Recipe(size=size, color=False, choose_aug=False, resize=(1, 2), affine=0.3, rotation=True, elastic_alpha=30.0, elastic_sigma=4.0)
    for _ in range(3):
        p = augment.draw_params(rs, H, W, rec)
        _moves_together(augment.augment_host(*src, p, size), src)


def test_draws_with_the_new_steps_off_are_the_old_draws():
    old = Recipe(size=64)
    new = Recipe.from_transform({'random_color': 1, 'horizontal_flip': True, 'vertical_flip': True, 'random_elastic': [6, 15],
                                 'random_chooseAug': 1, 'random_crop': 64})
    assert new.resize is None and new.affine is None and not new.rotation and new.rotation_limit == 90.0
    a, b = np.random.RandomState(7), np.random.RandomState(7)
    for H, W in ((150, 170), (40, 52), (97, 131)):
        p, q = augment.draw_params(a, H, W, old), augment.draw_params(b, H, W, new)
        for f in ('color', 'hflip', 'vflip', 'minv', 'alpha', 'sigma', 'seed', 'filter', 'y0', 'x0'):
            assert getattr(p, f) == getattr(q, f), f
        assert (q.scale, q.Hr, q.Wr, q.paff, q.rinv, q.fy0, q.fx0, q.fedge) == (1.0, 0, 0, None, None, None, None, None)
    assert a.rand() == b.rand()                                          # the same stream position
    # the stream is the one of the recipe before these steps existed: colour x 4, flips x 2, elastic offsets, seed, filter, crop
    rs, ref = np.random.RandomState(9), np.random.RandomState(9)
    p = augment.draw_params(rs, 100, 120, old)
    color = tuple(1 + (ref.rand() - 0.5) for _ in range(4))
    hf, vf = int(ref.rand() < 0.5), int(ref.rand() < 0.5)
    ref.uniform(-50.0, 50.0, size=(3, 2))
    seed = int(ref.randint(0, 2 ** 31))
    ref.rand()
    assert (p.color, p.hflip, p.vflip, p.seed) == (color, hf, vf, seed)
    assert (p.y0, p.x0) == (int(ref.randint(0, 37)), int(ref.randint(0, 57)))


def test_draws_with_the_new_steps_on_have_the_stated_ranges():
    rs = np.random.RandomState(0)
    rec = Recipe.from_transform({'random_resize': [1, 2], 'random_color': 1, 'random_affine': 0.3, 'horizontal_flip': True,
                                 'vertical_flip': True, 'random_elastic': [6, 15], 'random_rotation': 90, 'random_chooseAug': 1,
                                 'random_crop': 64})
    assert rec.resize == (1.0, 2.0) and rec.affine == 0.3 and rec.rotation
    H, W = 100, 130
    ps = [augment.draw_params(rs, H, W, rec) for _ in range(4000)]
    for p in ps:
        assert 1.0 <= p.scale < 2.0 and (p.Hr, p.Wr) == (int(H * p.scale), int(W * p.scale))
        assert -90.0 <= p.angle < 90.0
        a, b, c, d, e, f = p.paff
        assert abs(a - 1) <= 0.3 and abs(b) <= 0.3 and abs(d) <= 0.3 and abs(e - 1) <= 0.3
        assert c == -a * p.Wr / 2 - b * p.Hr / 2 + p.Wr / 2 and f == -d * p.Wr / 2 - e * p.Hr / 2 + p.Hr / 2
        assert 0 <= p.y0 <= max(p.Hr - 64, 0) and 0 <= p.x0 <= max(p.Wr - 64, 0)
    sc, an = np.array([p.scale for p in ps]), np.array([p.angle for p in ps])
    assert abs(sc.mean() - 1.5) < 0.03 and sc.max() > 1.95 and abs(an.mean()) < 3 and an.min() < -85 and an.max() > 85
    with pytest.raises(ValueError):
        Recipe(size=64, affine=0.6)
    with pytest.raises(ValueError):
        Recipe(size=64, affine=-0.1)


def test_field_window_holds_every_corner_pre_image():
    rs = np.random.RandomState(4)
    size = 64
    rec = Recipe(size=size, resize=(1, 2), rotation=True)
    plain = Recipe(size=size, rotation=True)
    worst = 0
    for k in range(1000):
        H, W = int(rs.randint(40, 151)), int(rs.randint(52, 171))
        p = augment.draw_params(rs, H, W, rec if k % 2 else plain)
        Hr, Wr = p.dims(H, W)
        ys = np.array([p.y0 - 6, p.y0 - 6, p.y0 + size + 5, p.y0 + size + 5])
        xs = np.array([p.x0 - 6, p.x0 + size + 5, p.x0 - 6, p.x0 + size + 5])
        Y, X, inside = augment.warp_source(p.rinv, Hr, Wr, ys, xs)
        in_win = (Y >= p.fy0) & (Y < p.fy0 + p.fedge) & (X >= p.fx0) & (X < p.fx0 + p.fedge)
        assert np.all(in_win | ~inside), (k, p)
        assert 0 <= p.fy0 < Hr and 0 <= p.fx0 < Wr
        worst = max(worst, p.fedge)
    assert worst <= int(np.ceil(np.sqrt(2) * (size + 12))) + 4


def test_options_trans_train():
    from cdnet_amd.options import Options
    opt = Options(isTrain=True).parse(['--trans-train', ALL, '--input-size', '64'])
    tf = opt.transform['train']
    assert list(tf) == ['random_resize', 'random_color', 'random_affine', 'horizontal_flip', 'vertical_flip', 'random_elastic',
                        'random_rotation', 'random_chooseAug', 'random_crop', 'label_encoding', 'to_tensor']
    assert tf['random_resize'] == [1, 2] and tf['random_affine'] == 0.3 and tf['random_rotation'] == 90 and tf['random_elastic'] == [6, 15]
    assert tf['random_crop'] == 64 and tf['random_color'] == 1 and tf['random_chooseAug'] == 1
    # the default is the dict the options held before the switch existed
    d = Options(isTrain=True).parse([]).transform['train']
    assert d == {'random_color': 1, 'horizontal_flip': True, 'vertical_flip': True, 'random_elastic': [6, 15], 'random_chooseAug': 1,
                 'random_crop': 256, 'label_encoding': [3, 2, 1], 'to_tensor': 1}
    assert list(d) == ['random_color', 'horizontal_flip', 'vertical_flip', 'random_elastic', 'random_chooseAug', 'random_crop',
                       'label_encoding', 'to_tensor']
    # vertical_flip is always there; order of the list does not matter
    t = Options(isTrain=True).parse(['--trans-train', 'random_crop,random_rotation']).transform['train']
    assert list(t) == ['vertical_flip', 'random_rotation', 'random_crop', 'label_encoding', 'to_tensor']
    with pytest.raises(ValueError):
        Options(isTrain=True).parse(['--trans-train', 'random_color,random_shear'])


def test_tile_batches_host_path_honours_the_new_keys(tmp_path):
    from test_data_folder import make_dataset
    from cdnet_amd.data_folder import DataFolder, TileBatches
    from cdnet_amd.options import Options
    from PIL import Image
    dirs = make_dataset(tmp_path, n=2, size=(50, 70))
    for k in range(2):                          # noise in [120, 140]: the colour chain turns no stored pixel black, so black = zero-filled
        Image.fromarray(np.random.RandomState(k).randint(120, 141, (50, 70, 3)).astype(np.uint8)).save(dirs[0] + '/im%d.png' % k)
    ds = DataFolder(dirs, ['weight.png', 'label.png'], [3, 1, 3])
    tf = Options(isTrain=True).parse(['--trans-train', ALL, '--input-size', '64']).transform['train']
    assert set(TileBatches.AUGMENTED) >= {'random_resize', 'random_affine', 'random_rotation'}
    tb = TileBatches(ds, tf, 2, 'cpu', seed=1, augment=True)
    assert tb.recipe.resize == (1.0, 2.0) and tb.recipe.affine == 0.3 and tb.recipe.rotation
    for i in range(len(tb.items)):
        img, w, lab = tb._draw(*tb.items[i])
        assert img.shape == (64, 64, 3) and w.shape == (64, 64) and lab.shape[:2] == (64, 64)
        assert len(np.unique(lab)) > 1
        # the source weight is 20 everywhere, so weight 0 marks what a pad or a border zero-filled: there the label is background, and
        # the image is black wherever the filters (reach 6 px; pixels beyond the crop count as unknown) saw nothing else
        Z = np.pad(w == 0, 6)
        deep = np.lib.stride_tricks.sliding_window_view(Z, (13, 13)).all((-1, -2))
        assert not img[deep].any() and not lab[w == 0].any()


def test_abi_geo_struct_and_argument_checks():
    from cdnet_amd import _lib
    lib = _lib.load()
    assert lib.cdnet_abi_sizeof(b'cdnet_aug_geo') == C.sizeof(augment.AugGeo)
    ws = lib.cdnet_augment_geo_workspace_bytes
    assert ws(0, 64, 0, 76) == 0 and ws(2, 0, 0, 76) == 0 and ws(2, 64, 5000, 76) == 0 and ws(2, 64, 0, 0) == 0 and ws(2, 64, -1, 76) == 0
    assert ws(2, 64, 8, 112) > ws(2, 64, 8, 76) > 0 and ws(2, 64, 0, 112) > ws(2, 64, 0, 76) > 0
    assert ws(2, 64, 8, 76) == lib.cdnet_augment_workspace_bytes(2, 64, 8)
    fake = C.c_void_p(4096)                                              # never dereferenced: every call below fails validation
    t = (augment.AugSample * 1)()
    t[0].img = t[0].weight = t[0].label = 4096
    t[0].H, t[0].W, t[0].img_stride, t[0].weight_stride, t[0].label_stride = 100, 100, 300, 100, 100
    t[0].sigma = 50.0
    t[0].minv[:] = augment.IDENTITY
    g = (augment.AugGeo * 1)()

    def reset():
        g[0].Hr, g[0].Wr, g[0].fy0, g[0].fx0, g[0].flags = 100, 100, -6, -6, 0
        g[0].paff[:] = augment.IDENTITY
        g[0].rinv[:] = augment.IDENTITY
        t[0].y0 = t[0].x0 = 0
        t[0].alpha = 0.0

    def call(edge=76, geo=g, ws_bytes=16):
        return lib.cdnet_augment_batch_geo(fake, t, fake if geo is not None else None, geo, edge, 1, 64, None, fake, ws_bytes, fake, fake,
                                           fake, 0, fake, None, None)
    reset()
    assert call() == 2 and b'workspace' in lib.cdnet_last_error()        # a valid table gets as far as the workspace check
    assert call(geo=None) == 1 and b'null pointer' in lib.cdnet_last_error()
    assert call(edge=0) == 1 and b'field_edge' in lib.cdnet_last_error()
    for Hr, Wr in ((0, 100), (100, 0), (32768, 100), (100, 40000)):
        reset()
        g[0].Hr, g[0].Wr, g[0].flags = Hr, Wr, augment.GEO_RESIZE
        assert call() == 1 and b'1..32767' in lib.cdnet_last_error()
    reset()
    g[0].Hr = 120                                                       # a resized size without the resize flag
    assert call() == 1 and b'resize flag' in lib.cdnet_last_error()
    for name in ('paff', 'rinv'):
        for bad in (float('nan'), float('inf')):
            reset()
            getattr(g[0], name)[2] = bad
            assert call() == 1 and b'not finite' in lib.cdnet_last_error()
    reset()
    g[0].flags = 8
    assert call() == 1 and b'flags' in lib.cdnet_last_error()
    reset()                                                             # the crop origin is checked against Hr x Wr, not H x W
    g[0].Hr, g[0].Wr, g[0].flags = 80, 80, augment.GEO_RESIZE
    t[0].y0 = 30
    assert call() == 1 and b'crop origin' in lib.cdnet_last_error()
    g[0].Hr = g[0].Wr = 200
    t[0].y0 = 130
    assert call() == 2
    reset()                                                             # an affine outside Pillow's 16.16 range
    g[0].flags = augment.GEO_AFFINE
    g[0].paff[2] = 40000.0
    assert call() == 1 and b'16.16' in lib.cdnet_last_error()
    reset()                                                             # a field window that misses the rotated crop
    t[0].alpha = 1.0
    g[0].flags = augment.GEO_ROTATION
    g[0].rinv[:] = augment.rotation_inverse(45.0, 100, 100)
    assert call(edge=76) == 1 and b'field window' in lib.cdnet_last_error()
    p = Params(color=(1.0,) * 4, hflip=0, vflip=0, minv=augment.IDENTITY, alpha=1.0, sigma=50.0, seed=0, filter=0, y0=0, x0=0,
               rinv=augment.rotation_inverse(45.0, 100, 100))
    g[0].fy0, g[0].fx0, edge = augment.field_box(p, 100, 100, 64)
    assert call(edge=edge) == 2                                         # the host's own window passes
    assert call(edge=edge - 40) == 1 and b'field window' in lib.cdnet_last_error()
    # a 40 x 40 source under the 64 crop at 45 degrees: all four corner pre-images fall outside the image, the crop's interior does not,
    # so the window must still hold the image part of the corners' bounding box
    reset()
    t[0].H, t[0].W, t[0].img_stride, t[0].weight_stride, t[0].label_stride = 40, 40, 120, 40, 40
    t[0].alpha = 1.0
    g[0].Hr, g[0].Wr, g[0].flags = 40, 40, augment.GEO_ROTATION
    g[0].rinv[:] = augment.rotation_inverse(45.0, 40, 40)
    ys, xs = np.array([-6, -6, 69, 69]), np.array([-6, 69, -6, 69])
    Y, X, inside = augment.warp_source(augment.rotation_inverse(45.0, 40, 40), 40, 40, ys, xs)
    assert not inside.any()
    for fy0, fx0, edge in ((0, 0, 1), (0, 0, 39), (1, 0, 40), (10000, 0, 76), (-100, -100, 76), (0, 10000, 76)):
        g[0].fy0, g[0].fx0 = fy0, fx0
        assert call(edge=edge) == 1 and b'field window' in lib.cdnet_last_error(), (fy0, fx0, edge)
    g[0].fy0, g[0].fx0 = 0, 0
    assert call(edge=40) == 2                                           # the whole image: passes
    p = Params(color=(1.0,) * 4, hflip=0, vflip=0, minv=augment.IDENTITY, alpha=1.0, sigma=50.0, seed=0, filter=0, y0=0, x0=0,
               rinv=augment.rotation_inverse(45.0, 40, 40))
    g[0].fy0, g[0].fx0, edge = augment.field_box(p, 40, 40, 64)
    assert call(edge=edge) == 2
    # some corners inside: a window around the in-image corners alone misses the strip next to the image edge
    reset()
    t[0].H, t[0].W, t[0].img_stride, t[0].weight_stride, t[0].label_stride = 100, 100, 300, 100, 100
    t[0].alpha = 1.0
    g[0].flags = augment.GEO_ROTATION
    g[0].rinv[:] = augment.rotation_inverse(30.0, 100, 100)
    Y, X, inside = augment.warp_source(augment.rotation_inverse(30.0, 100, 100), 100, 100, ys, xs)
    assert inside.any() and not inside.all()
    lo_y, lo_x = int(Y[inside].min()), int(X[inside].min())
    edge = int(max(Y[inside].max() - lo_y, X[inside].max() - lo_x)) + 1
    g[0].fy0, g[0].fx0 = lo_y, lo_x
    assert call(edge=edge) == 1 and b'field window' in lib.cdnet_last_error()
