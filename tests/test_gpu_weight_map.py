"""cdnet_weight_map (csrc/weight_map.hip) against the per-instance-EDT formula, and `train --make-weight-maps`.  The oracle, the drawn
cases and the comparison rule are those of tests/test_weight_map_cpu.py: equal bytes, except that a pixel whose pre-floor oracle value
lies within 1e-9 of an integer may differ by 1 (at most 0.01 % of a case).

The tile is 32 x 32 and the default radius 17, so a window is 66 wide: every drawn case is ragged against the tile in both dimensions and
has one dimension below 66."""
import numpy as np
import pytest

from test_weight_map_cpu import CASES, assert_same_bytes, case, draw_ellipses, oracle_values, png_instances

pytestmark = pytest.mark.gpu


def device_map(L, w0=10.0, sigma=5.0):
    from cdnet_amd.data_prepare.weight_maps import weight_map
    return weight_map(np.asarray(L), w0, sigma, device='cuda')


def check(L, what, w0=10.0, sigma=5.0):
    got = device_map(L, w0, sigma)
    assert_same_bytes(got, oracle_values(L, w0, sigma), what)
    return got


@pytest.mark.parametrize('name', sorted(CASES))
def test_drawn_cases(name):
    import torch
    from cdnet_amd.data_prepare.weight_maps import weight_map
    L, v = case(name)
    got = device_map(L)
    assert_same_bytes(got, v, name)
    if name in ('empty_40x40', 'single_40x40'):
        assert (got == 20).all()
    dev = torch.from_numpy(np.array(L)).to('cuda', torch.int32)                   # a device tensor is taken as it is
    assert np.array_equal(weight_map(dev), got)
    neg = np.where(np.asarray(L) == 0, -5, L)                                      # ids <= 0 are background
    assert np.array_equal(device_map(neg), got)


@pytest.mark.parametrize('w0,sigma,R', [(5.0, 3.0, 10), (11.75, 12.0, 40), (10.0, 19.6, 64)])
def test_other_constants(w0, sigma, R):
    """R = 64 is the cap: its window, (32 + 128)^2 * 4 B = 100 KB, is the one launch beyond the default 64 KB of dynamic LDS"""
    from cdnet_amd import _lib
    assert _lib.load().cdnet_weight_map_radius(w0, sigma) == R
    L, v = case('ellipses_70x53', w0, sigma)
    got = device_map(L, w0, sigma)
    assert_same_bytes(got, v, 'w0 %g sigma %g' % (w0, sigma))
    assert got.max() > 20 * (1 + w0) * 0.5


@pytest.mark.parametrize('shape', [(1, 40), (17, 17), (40, 1)])
def test_thin_shapes(shape):
    rs = np.random.RandomState(shape[0])
    L = np.zeros(shape, np.int64)
    at = rs.choice(L.size, 5, replace=False)
    L.flat[at] = [3, 900000, 17, 2 ** 31 - 1, 256]                                  # arbitrary positive int32 ids
    got = check(L, str(shape))
    assert got.max() > 20


def test_cut_off_across_a_tile_boundary():
    """two single-pixel instances on one row, 16 apart and then 17 apart, either side of the tile boundary at column 32: d1 + d2 is the
    gap for every pixel between them, 20 * (1 + 10 exp(-256 / 50)) = 21.19.. and 20 * (1 + 10 exp(-289 / 50)) = 20.61.."""
    for other, byte in ((39, 21), (40, 20)):
        L = np.zeros((9, 70), np.int32)
        L[4, 23], L[4, other] = 1, 2
        got = check(L, 'columns 23 and %d' % other)
        assert (got[4, 24:other] == byte).all() and got[4, 23] == 20 and got[4, other] == 20
    L = np.zeros((70, 9), np.int32)                                                  # the same down a column, across the tile boundary at row 32
    L[23, 4], L[39, 4] = 5, 4
    assert (check(L, 'rows 23 and 39')[24:39, 4] == 21).all()


def test_one_pixel_gap_reads_204():
    L = np.zeros((40, 45), np.int32)
    L[5:30, 10:31] = 1
    L[5:30, 32:40] = 2                                                               # column 31 is the gap, on the last column of tile 0
    got = check(L, 'one-pixel gap')
    assert (got[5:30, 31] == 204).all() and got.max() == 204


def test_border_and_corner_instances():
    L = np.zeros((50, 75), np.int32)
    L[0:4, 0:5] = 1                                                                  # corner
    L[0:3, 20:40] = 2                                                                # top border, across a tile boundary
    L[20:33, 0:2] = 3                                                                # left border
    L[47:50, 70:75] = 4                                                              # far corner
    L[30:36, 72:75] = 5                                                              # right border
    L[49, 10:30] = 6                                                                 # bottom border
    got = check(L, 'border')
    assert got[0, 5:20].max() > 20


def test_window_with_one_instance_next_to_one_with_two():
    """tile (0, 0)'s window [-17, 49) holds instance 1 alone: the workgroup leaves early; the windows of the tiles right of it hold two"""
    L = np.zeros((32, 128), np.int32)
    L[5:9, 5:9] = 1
    L[10:20, 70:80] = 2
    L[12:18, 84:90] = 3
    got = check(L, 'early exit')
    assert (got[:, :32] == 20).all() and got[:, 64:96].max() > 100


def test_device_equals_host_300x260():
    from cdnet_amd.data_prepare.weight_maps import weight_map_host
    L = draw_ellipses(300, 260, 80, seed=5, rmin=4, rmax=11, touching=True)
    v = oracle_values(L)
    host, got = weight_map_host(L), device_map(L)
    assert_same_bytes(host, v, 'host')
    assert_same_bytes(got, v, 'device')
    near = (np.abs(v - np.round(v)) < 1e-9) & (v - 20.0 >= 1e-9)
    assert np.array_equal(got[~near], host[~near]) and np.abs(got.astype(int) - host.astype(int)).max() <= 1


def test_train_makes_missing_weight_maps(tmp_path, monkeypatch):
    """--make-weight-maps writes the three missing PNGs (equal to the oracle of their labels) and trains; without it the same call still
    stops at 'Found 0 image pairs'"""
    import os
    import torch
    from PIL import Image
    from test_data_folder import make_dataset
    from cdnet_amd import train
    from cdnet_amd.data_folder import DataFolder, TileBatches
    from cdnet_amd.options import Options
    root = tmp_path / 'data' / Options(isTrain=True).dataset
    dirs = make_dataset(root, n=3, size=(150, 170), seed=4)
    for k in range(3):
        os.remove(os.path.join(dirs[1], 'im%d_weight.png' % k))
    monkeypatch.chdir(tmp_path)
    args = ['--epochs', '1', '--batch-size', '2', '--input-size', '64', '--save-dir', str(tmp_path / 'exp')]
    with pytest.raises(RuntimeError, match='Found 0 image pairs'):
        train.main(args)
    assert os.listdir(dirs[1]) == []
    res = train.main(['--make-weight-maps'] + args)
    assert len(res) == 11 and np.isfinite(res).all()
    for k in range(3):
        im = Image.open(os.path.join(dirs[1], 'im%d_weight.png' % k))
        assert im.mode == 'L'
        lab = np.asarray(Image.open(os.path.join(dirs[2], 'im%d_label.png' % k)))
        assert_same_bytes(np.asarray(im), oracle_values(png_instances(lab)), 'im%d' % k)
    ds = DataFolder(dirs, ['weight.png', 'label.png'], [3, 1, 3])
    assert len(ds) == 3
    tb = TileBatches(ds, {'to_tensor': 1, 'label_encoding': [3, 2, 1]}, 1, torch.device('cuda:0'), seed=1, shuffle=False)
    weight = next(iter(tb))[1]
    assert weight.dtype == torch.uint8 and tuple(weight.shape) == (1, 1, 150, 170) and int(weight.max()) > 20
