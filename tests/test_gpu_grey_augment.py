"""Mode-L device augmentation (cdnet_augment_batch_c / cdnet_augment_batch_geo_c, channels = 1) on the MI355X: the whole chain against
the host implementation (cdnet_amd.augment.augment_host: Pillow itself for the colour chain, the filters and random_affine) bit for bit,
the colour chain and the filters against Pillow's own results (tests/golden/augment_grey.npz), channels = 3 through the new entries
against the RGB entries byte for byte, and the zero pad of a source smaller than the crop."""
import ctypes as C

import numpy as np
import pytest
import torch

from cdnet_amd import _lib, augment
from cdnet_amd.augment import Params, Recipe, Source

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SIZE = 32
SHAPES = ((40, 52), (70, 64), (33, 90))


def _params(**kw):
    p = dict(color=(1.0, 1.0, 1.0, 1.0), hflip=0, vflip=0, minv=augment.IDENTITY, alpha=0.0, sigma=50.0, seed=0, filter=0, y0=0, x0=0)
    p.update(kw)
    return Params(**p)


def _sources(rs, instance):
    out = []
    for H, W in SHAPES:
        img = np.clip(rs.randint(0, 256, (H, W)) // 3 + 60 + (np.arange(W) % 50)[None, :] * 2, 0, 255).astype(np.uint8)
        w = rs.randint(1, 30, (H, W)).astype(np.uint8)
        if instance:
            from cdnet_amd import synth
            lab = synth.ellipse_instances(H, W, 8, rs, 4, 8, 5).astype(np.int32)
        else:
            lab = np.where(rs.rand(H, W) < 0.3, 255, 0).astype(np.uint8)
        out.append((img, w, lab))
    return out


def _check_against_host(items, ps, size, label_dtype):
    srcs = [Source(*it, DEV) for it in items]
    assert all(s.channels == 1 for s in srcs)
    img, weight, label, varied, field, origin = augment.augment_batch(srcs, ps, size, want_field=True, want_origin=True)
    torch.cuda.synchronize()
    assert tuple(img.shape) == (len(ps), 1, size, size) and label.dtype == label_dtype
    for b, (it, p) in enumerate(zip(items, ps)):
        f = field[b].cpu().numpy() if p.alpha != 0 else None
        want = augment.augment_host(it[0], it[1], it[2], p, size, field=f, origin=tuple(origin[b]))
        got_img = img[b, 0].cpu().numpy()
        want_img = want[0].astype(np.float32) / np.float32(255)
        assert want_img.shape == (size, size)
        assert np.array_equal(got_img, want_img), (b, p, int((got_img != want_img).sum()))
        assert np.array_equal(weight[b].cpu().numpy(), want[1]), (b, p)
        assert np.array_equal(label[b].cpu().numpy(), want[2].astype(label.cpu().numpy().dtype)), (b, p)
        assert varied[b].item() == int(len(np.unique(want[2])) > 1), (b, p)
    return field


def _draws(rs, items, rec, n):
    """n samples over the sources in turn: every filter code, alpha 0 and alpha 30 / sigma 4 in turn, the flips as drawn"""
    its, ps = [], []
    for k in range(n):
        it = items[k % len(items)]
        p = augment.draw_params(rs, it[1].shape[0], it[1].shape[1], rec)
        p.filter = k % 4
        p.alpha, p.sigma = (0.0, 50.0) if (k // 4) % 2 == 0 else (30.0, 4.0)
        if p.rinv is not None:
            Hr, Wr = p.dims(it[1].shape[0], it[1].shape[1])
            p.fy0, p.fx0, p.fedge = augment.field_box(p, Hr, Wr, rec.size)
        its.append(it)
        ps.append(p)
    return its, ps


@pytest.mark.parametrize('geo', [False, True])
@pytest.mark.parametrize('instance', [False, True])
def test_device_equals_host_on_l(instance, geo):
    rs = np.random.RandomState(17 + 2 * int(instance) + int(geo))
    items = _sources(rs, instance)
    rec = Recipe(size=SIZE, resize=(1.0, 2.0), affine=0.3, rotation=True) if geo else Recipe(size=SIZE)
    its, ps = _draws(rs, items, rec, 24)
    assert {p.hflip for p in ps} == {0, 1} and {p.vflip for p in ps} == {0, 1} and {p.filter for p in ps} == {0, 1, 2, 3}
    assert {p.alpha for p in ps} == {0.0, 30.0}
    field = _check_against_host(its, ps, SIZE, torch.int32 if instance else torch.uint8)
    assert float(field.abs().max()) > 0.5                               # alpha 30 moves pixels


def test_colour_chain_and_filters_equal_pillow_on_the_device(golden):
    g = golden('augment_grey')
    for k in range(3):
        src = g['src%d' % k]
        H, W = src.shape
        s = max(H, W)
        z = np.zeros((H, W), np.uint8)
        z[0, 0] = 1
        source = Source(src, z, z, DEV)
        ps = [_params(color=tuple(float(v) for v in f)) for f in g['factors']] + [_params(filter=c) for c in (1, 2, 3)]
        ps += [_params(color=(float(c), 1.0, 1.0, 1.0)) for c in g['color_only']]
        img, weight, label, varied = augment.augment_batch([source] * len(ps), ps, s)
        torch.cuda.synchronize()
        want = list(g['chain%d' % k]) + list(g['filt%d' % k]) + [src, src]          # (Color alone: the identity)
        for j, w in enumerate(want):
            got = np.rint(img[j, 0].cpu().numpy() * 255.0).astype(np.uint8)         # v / 255 in fp32 is exact to invert by rounding
            assert np.array_equal(got[:H, :W], w), (k, j, int((got[:H, :W] != w).sum()))     # edge rows and columns included
            assert not got[H:].any() and not got[:, W:].any()
        assert varied.tolist() == [1] * len(ps)


def _raw_call(name, srcs, ps, size, geo, FS, norm, channels=None):
    """one raw ABI call on RGB sources -> (image, weight, label, varied, field)"""
    B = len(srcs)
    table = (augment.AugSample * B)()
    rmax = 0
    for t, src, p in zip(table, srcs, ps):
        t.minv[:] = p.minv
        t.img, t.weight, t.label = src.img.data_ptr(), src.weight.data_ptr(), src.label.data_ptr()
        t.H, t.W, t.img_stride, t.weight_stride, t.label_stride, t.label_i32 = src.H, src.W, 3 * src.W, src.W, src.W, int(src.label_i32)
        t.color[:] = p.color
        t.hflip, t.vflip, t.filter, t.y0, t.x0 = p.hflip, p.vflip, p.filter, p.y0, p.x0
        t.alpha, t.sigma, t.seed = p.alpha, p.sigma, p.seed
        if p.alpha != 0.0:
            rmax = max(rmax, augment.gauss_radius(p.sigma))
    lib = _lib.load()
    ws = torch.empty((lib.cdnet_augment_geo_workspace_bytes(B, size, rmax, FS),), dtype=torch.uint8, device=DEV)
    up = lambda tab: torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(DEV)
    table_dev = up(table)
    image = torch.full((B, 3, size, size), -7.0, dtype=torch.float32, device=DEV)
    weight = torch.full((B, size, size), 99, dtype=torch.uint8, device=DEV)
    label = torch.full((B, size, size), 99, dtype=torch.uint8, device=DEV)
    varied = torch.full((B,), 99, dtype=torch.int32, device=DEV)
    field = torch.zeros((B, 2, FS, FS), dtype=torch.float32, device=DEV)
    nrm = (C.c_float * 6)(*norm)
    tail = () if channels is None else (channels,)
    if geo is None:
        _lib.call(name, _lib.ptr(table_dev), table, B, size, nrm, _lib.ptr(ws), ws.numel(), _lib.ptr(image), _lib.ptr(weight), _lib.ptr(label),
                  0, _lib.ptr(varied), _lib.ptr(field), _lib.stream_ptr(), *tail)
    else:
        geo_dev = up(geo)
        _lib.call(name, _lib.ptr(table_dev), table, _lib.ptr(geo_dev), geo, FS, B, size, nrm, _lib.ptr(ws), ws.numel(), _lib.ptr(image),
                  _lib.ptr(weight), _lib.ptr(label), 0, _lib.ptr(varied), _lib.ptr(field), _lib.stream_ptr(), *tail)
    torch.cuda.synchronize()
    return image, weight, label, varied, field


@pytest.mark.parametrize('geo', [False, True])
def test_three_channels_through_the_new_entries_equal_the_rgb_entries(geo):
    rs = np.random.RandomState(23 + int(geo))
    items = []
    for H, W in SHAPES:
        items.append((rs.randint(0, 256, (H, W, 3)).astype(np.uint8), rs.randint(1, 30, (H, W)).astype(np.uint8),
                      np.where(rs.rand(H, W) < 0.3, 255, 0).astype(np.uint8)))
    rec = Recipe(size=SIZE, resize=(1.0, 2.0), affine=0.3, rotation=True) if geo else Recipe(size=SIZE)
    its, ps = _draws(rs, items, rec, 12)
    srcs = [Source(*it, DEV) for it in its]
    table, FS = augment._geo_table(srcs, ps, SIZE)
    assert (table is not None) == geo
    norm = (0.5, 0.4, 0.3, 0.2, 0.25, 0.3)
    old = _raw_call('cdnet_augment_batch_geo' if geo else 'cdnet_augment_batch', srcs, ps, SIZE, table, FS, norm)
    new = _raw_call('cdnet_augment_batch_geo_c' if geo else 'cdnet_augment_batch_c', srcs, ps, SIZE, table, FS, norm, channels=3)
    for name, a, b in zip(('image', 'weight', 'label', 'varied', 'field'), old, new):
        a, b = a.cpu().numpy(), b.cpu().numpy()
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), name
    assert float(old[0].min()) > -7.0 and int(old[3].max()) <= 1 and float(old[4].abs().max()) > 0.5        # every output was written


def test_one_channel_source_smaller_than_the_crop_is_zero_padded():
    rs = np.random.RandomState(5)
    H, W, size = 20, 29, 40                                             # 2 x 2 output tiles; rows 20.. and columns 29.. lie outside
    img = rs.randint(1, 256, (H, W)).astype(np.uint8)
    w = rs.randint(1, 30, (H, W)).astype(np.uint8)
    lab = rs.randint(1, 3, (H, W)).astype(np.uint8)
    ps = [_params(), _params(filter=2), _params(hflip=1, vflip=1, filter=3), _params(color=(0.7, 1.2, 0.8, 1.4), filter=1)]
    _check_against_host([(img, w, lab)] * len(ps), ps, size, torch.uint8)
    image, weight, label, varied = augment.augment_batch([Source(img, w, lab, DEV)], ps[:1], size, normalize=([0.5], [0.25]))
    torch.cuda.synchronize()
    assert np.array_equal(weight[0].cpu().numpy()[:H, :W], w) and not weight[0, H:].any() and not weight[0, :, W:].any()
    assert not label[0, H:].any() and np.array_equal(label[0].cpu().numpy()[:H, :W], lab) and varied.tolist() == [1]
    want = (img.astype(np.float32) / np.float32(255) - np.float32(0.5)) / np.float32(0.25)
    assert np.array_equal(image[0, 0].cpu().numpy()[:H, :W], want)
    pad = (np.float32(0) - np.float32(0.5)) / np.float32(0.25)                  # the pad is a zero byte, normalised like any other
    assert np.all(image[0, 0, H:].cpu().numpy() == pad) and np.all(image[0, 0, :, W:].cpu().numpy() == pad)
