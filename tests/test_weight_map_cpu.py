"""cdnet_amd.data_prepare.weight_maps on the host: weight_map_host against the per-instance-EDT formula, the argument checks of the ABI
entry (no GPU needed), the command line and the pairing of get_imgs_list after it.  The oracle and the drawn cases below are shared with
tests/test_gpu_weight_map.py.

Comparison rule (`assert_same_bytes`): the bytes are equal; a pixel whose pre-floor oracle value lies within 1e-9 of an integer may differ
by 1, and such pixels are at most 0.01 % of a case."""
import ctypes
import functools
import os

import numpy as np
import pytest


def oracle_values(L, w0=10.0, sigma=5.0):
    """pre-floor 20 * w of every pixel, float64: one whole-image EDT per instance, sorted, d[0] + d[1]"""
    from scipy.ndimage import distance_transform_edt
    L = np.asarray(L)
    v = np.full(L.shape, 20.0)
    ids = np.unique(L[L > 0])
    if len(ids) < 2:
        return v
    d = np.sort(np.stack([distance_transform_edt(L != k) for k in ids]), axis=0)
    s = d[0] + d[1]
    v = 20.0 * (1.0 + w0 * np.exp(-(s ** 2) / (2.0 * sigma ** 2)))
    v[L > 0] = 20.0
    return v


def assert_same_bytes(got, values, what=''):
    want = np.floor(values).astype(np.uint8)
    got = np.asarray(got)
    assert got.dtype == np.uint8 and got.shape == want.shape, what
    near = np.abs(values - np.round(values)) < 1e-9
    # values in [20, 20 + 1e-9) - instance pixels, and background whose border term has died out - are no rounding cases: they get no
    # allowance (the byte must be 20) and do not count against the cap
    near &= values - 20.0 >= 1e-9
    assert near.sum() <= 1e-4 * near.size, '%s: %d pixels within 1e-9 of an integer' % (what, near.sum())
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    bad = (diff > 0) & ~near
    assert not bad.any(), '%s: %d bytes differ, first at %s: got %d, want %d (pre-floor %.12f)' % (
        what, bad.sum(), np.argwhere(bad)[0], got[bad][0], want[bad][0], values[bad][0])
    assert diff.max() <= 1, what


def draw_ellipses(H, W, n, seed, rmin=3, rmax=8, touching=False, ids=None):
    """n ellipses at random places; a later one takes only free pixels, so with `touching` instances may abut, without it an ellipse
    that meets an earlier one (or its 8-neighbourhood) is left out"""
    from scipy.ndimage import binary_dilation
    rs = np.random.RandomState(seed)
    L = np.zeros((H, W), np.int64)
    yy, xx = np.mgrid[:H, :W]
    k = 0
    for _ in range(20 * n):
        if k == n:
            break
        cy, cx, a, b, th = rs.randint(0, H), rs.randint(0, W), rs.randint(rmin, rmax + 1), rs.randint(rmin, rmax + 1), rs.rand() * np.pi
        u = (yy - cy) * np.cos(th) + (xx - cx) * np.sin(th)
        v = -(yy - cy) * np.sin(th) + (xx - cx) * np.cos(th)
        m = ((u / a) ** 2 + (v / b) ** 2 <= 1) & (L == 0)
        if not m.any() or (not touching and (L[binary_dilation(m, np.ones((3, 3), bool))] != 0).any()):
            continue
        L[m] = ids[k] if ids is not None else k + 1
        k += 1
    assert k == n, 'only %d of %d ellipses fitted' % (k, n)
    return L


def _single():
    L = np.zeros((40, 40), np.int64)
    L[12:20, 9:30] = 7
    return L


CASES = {
    'ellipses_70x53': lambda: draw_ellipses(70, 53, 13, seed=1, rmin=3, rmax=6),
    'sparse_ids_33x95': lambda: draw_ellipses(33, 95, 10, seed=2, rmin=2, rmax=6, ids=[1000 + 37 * k for k in range(9)] + [70001]),
    'touching_64x64': lambda: draw_ellipses(64, 64, 30, seed=3, rmin=2, rmax=6, touching=True),
    'empty_40x40': lambda: np.zeros((40, 40), np.int64),
    'single_40x40': _single,
}


@functools.lru_cache(maxsize=None)
def case(name, w0=10.0, sigma=5.0):
    """(instance map, pre-floor oracle values) of a drawn case, computed once per session and never written to"""
    L = CASES[name]()
    v = oracle_values(L, w0, sigma)
    L.setflags(write=False)
    v.setflags(write=False)
    return L, v


def png_instances(lab3):
    """the rule of test_dam.ground_truth_instances for a 3-class label image: 8-connected components of channel 0 > 127, grown by disk(1)"""
    from scipy import ndimage as ndi
    cc, _ = ndi.label(lab3[:, :, 0] > 127, structure=np.ones((3, 3), int))
    return ndi.grey_dilation(cc, footprint=np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool))


def three_class(L):
    """3-class colour label of an instance map as the datasets store it: red = inside, green = boundary, blue = background"""
    from cdnet_amd import synth
    inside = L > 0
    ero = synth.erode8(inside)
    lab = np.zeros(L.shape + (3,), np.uint8)
    lab[..., 0][ero] = 255
    lab[..., 1][inside & ~ero] = 255
    lab[..., 2][~inside] = 255
    return lab


@pytest.mark.parametrize('name', sorted(CASES))
def test_host_matches_oracle(name):
    from cdnet_amd.data_prepare.weight_maps import weight_map, weight_map_host
    L, v = case(name)
    got = weight_map_host(L)
    assert_same_bytes(got, v, name)
    if name in ('empty_40x40', 'single_40x40'):
        assert (got == 20).all()
    else:
        assert got.max() > 40 and len(np.unique(L)) - 1 == {'ellipses_70x53': 13, 'sparse_ids_33x95': 10, 'touching_64x64': 30}[name]
    assert np.array_equal(weight_map(L, device='cpu'), got)
    import torch
    assert np.array_equal(weight_map(torch.from_numpy(np.array(L)), device='cpu'), got)


def test_host_other_constants_and_negative_ids():
    from cdnet_amd.data_prepare.weight_maps import weight_map_host
    for w0, sigma in ((5.0, 3.0), (11.75, 12.0), (10.0, 19.6)):
        L, v = case('ellipses_70x53', w0, sigma)
        assert_same_bytes(weight_map_host(L, w0, sigma), v, 'w0 %g sigma %g' % (w0, sigma))
    L, v = case('touching_64x64')
    neg = np.where(L == 0, -3, L)                                   # ids <= 0 are background
    assert_same_bytes(weight_map_host(neg), v, 'negative background')
    full = np.ones((9, 11), np.int32)                               # no background pixel at all
    full[:, 6:] = 2
    assert (weight_map_host(full) == 20).all()
    with pytest.raises(ValueError):
        weight_map_host(L, w0=12.0)
    with pytest.raises(ValueError):
        weight_map_host(L, sigma=20.0)
    with pytest.raises(ValueError):
        weight_map_host(L.astype(np.float32))


def test_radius():
    from cdnet_amd import _lib
    from cdnet_amd.data_prepare import weight_maps
    lib = _lib.load()
    for w0, sigma, R in ((10.0, 5.0, 17), (5.0, 3.0, 10), (11.75, 12.0, 40), (10.0, 19.6, 64)):
        assert lib.cdnet_weight_map_radius(w0, sigma) == R and weight_maps.radius(w0, sigma) == R
    assert lib.cdnet_weight_map_radius(10.0, 20.0) == 66            # the radius itself; cdnet_weight_map refuses it
    for w0, sigma in ((0.0, 5.0), (-1.0, 5.0), (10.0, 0.0), (10.0, -2.0), (12.0, 5.0), (float('nan'), 5.0), (10.0, float('nan'))):
        assert lib.cdnet_weight_map_radius(w0, sigma) == 0


def test_entry_refuses_bad_arguments_without_gpu():
    """every refusal comes before any HIP call: the pointers below are host addresses that are never read"""
    from cdnet_amd import _lib
    lib = _lib.load()
    lab, out = np.zeros((8, 8), np.int32), np.zeros((8, 8), np.uint8)
    pl, po = ctypes.c_void_p(lab.ctypes.data), ctypes.c_void_p(out.ctypes.data)

    def refused(*args):
        rc = lib.cdnet_weight_map(*args)
        msg = lib.cdnet_last_error()
        assert rc == 1 and msg.startswith(b'cdnet_weight_map:'), (rc, msg)
        return msg
    assert b'null pointer' in refused(None, 8, 8, 10.0, 5.0, po, None)
    assert b'null pointer' in refused(pl, 8, 8, 10.0, 5.0, None, None)
    assert b'wrap' in refused(pl, 8, 8, 12.0, 5.0, po, None)
    assert b'R = 66 > 64' in refused(pl, 8, 8, 10.0, 20.0, po, None)
    assert b'positive' in refused(pl, 8, 8, 10.0, 0.0, po, None)
    assert b'positive' in refused(pl, 8, 8, -1.0, 5.0, po, None)
    assert b'size' in refused(pl, 0, 8, 10.0, 5.0, po, None)
    assert (out == 0).all()


def _label_dir(tmp_path):
    """images/ and labels/ of three samples: two instance-level .npy (one with ids above 255), one 3-class .png; {stem: oracle values}"""
    from PIL import Image
    img, lab = tmp_path / 'images', tmp_path / 'labels'
    img.mkdir()
    lab.mkdir()
    a = np.array(case('ellipses_70x53')[0])
    b = np.array(case('touching_64x64')[0]) * 300                  # ids 300 .. 9000: a cast to uint8 would merge 256 with background
    c = np.array(case('sparse_ids_33x95')[0])
    np.save(lab / 'a_label.npy', a.astype(np.int32))
    np.save(lab / 'b_label.npy', np.stack([b, np.zeros_like(b)], axis=2))          # 3-D: channel 0 holds the ids
    c3 = three_class(c)
    Image.fromarray(c3).save(lab / 'c_label.png')
    (lab / 'notes.txt').write_text('x')
    for stem, L in (('a', a), ('b', b), ('c', c)):
        Image.fromarray(np.zeros(L.shape + (3,), np.uint8)).save(img / (stem + '.png'))
    return img, lab, {'a': case('ellipses_70x53')[1], 'b': case('touching_64x64')[1], 'c': oracle_values(png_instances(c3))}


def test_training_entry_prepares_a_split(tmp_path, caplog):
    """train._prepare_weight_maps, the step `--make-weight-maps` adds in front of DataFolder: without the flag only a warning about the
    dropped images, with it the missing files (here through device 'cpu')"""
    import logging
    from cdnet_amd import train
    from cdnet_amd.data_folder import get_imgs_list
    img, lab, want = _label_dir(tmp_path)
    out = tmp_path / 'weight_maps'
    out.mkdir()
    dirs, fix = [str(img), str(out), str(lab)], ['weight.png', 'label.npy']
    logger = logging.getLogger('test_weight_map_cpu')
    with caplog.at_level(logging.INFO, logger=logger.name):
        train._prepare_weight_maps(dirs, fix, False, 0, 1, 'cpu', logger)
    assert os.listdir(out) == []
    assert [r.levelno for r in caplog.records] == [logging.WARNING] and '3 of 3 images' in caplog.records[0].getMessage()
    caplog.clear()
    with caplog.at_level(logging.INFO, logger=logger.name):
        train._prepare_weight_maps(dirs, fix, False, 1, 2, 'cpu', logger)          # not rank 0: silent
    assert caplog.records == []
    with caplog.at_level(logging.INFO, logger=logger.name):
        train._prepare_weight_maps(dirs, fix, True, 0, 1, 'cpu', logger)
    assert sorted(os.listdir(out)) == ['a_weight.png', 'b_weight.png', 'c_weight.png']
    msgs = [r.getMessage() for r in caplog.records]
    assert '3 weight maps written' in msgs[0] and '1 of 3 images' in msgs[1]        # c has a .png label, no label.npy: still left out
    assert len(get_imgs_list(dirs, fix)) == 2


def test_command_line_and_pairing(tmp_path, capsys):
    from PIL import Image
    from cdnet_amd.data_folder import get_imgs_list
    from cdnet_amd.data_prepare import weight_maps
    img, lab, want = _label_dir(tmp_path)
    out = tmp_path / 'weight_maps'
    assert np.array_equal(weight_maps.instances_of(str(lab / 'b_label.npy')), np.array(case('touching_64x64')[0]) * 300)
    assert weight_maps.instances_of(str(lab / 'b_label.npy')).max() == 9000
    out.mkdir()
    dirs, fix = [str(img), str(out), str(lab)], ['weight.png', 'label.npy']
    assert get_imgs_list(dirs, fix) == []
    argv = ['--label-dir', str(lab), '--out-dir', str(out), '--device', 'cpu']
    assert weight_maps.main(argv) == (3, 0)
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 4 and lines[-1] == '3 weight maps written, 0 skipped'
    for stem, v in want.items():
        im = Image.open(out / (stem + '_weight.png'))
        assert im.mode == 'L'
        assert_same_bytes(np.asarray(im), v, stem)
    assert np.asarray(Image.open(out / 'b_weight.png')).max() > 100     # touching instances: the ids above 255 stayed apart
    assert sorted(os.path.basename(i[0]) for i in get_imgs_list(dirs, fix)) == ['a.png', 'b.png']
    assert [os.path.basename(i[0]) for i in get_imgs_list(dirs, ['weight.png', 'label.png'])] == ['c.png']
    # a second run writes nothing; --overwrite rewrites
    stamp = {p: os.stat(out / p).st_mtime_ns for p in os.listdir(out)}
    Image.fromarray(np.full((70, 53), 20, np.uint8)).save(out / 'a_weight.png')
    assert weight_maps.main(argv) == (0, 3)
    assert (np.asarray(Image.open(out / 'a_weight.png')) == 20).all()
    assert all(os.stat(out / p).st_mtime_ns == stamp[p] for p in ('b_weight.png', 'c_weight.png'))
    assert weight_maps.main(argv + ['--overwrite']) == (3, 0)
    assert_same_bytes(np.asarray(Image.open(out / 'a_weight.png')), want['a'], 'a rewritten')
    with pytest.raises(ValueError):
        weight_maps.main(argv + ['--w0', '12'])
