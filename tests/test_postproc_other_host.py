"""postproc_other.process_host - the reference's 'micronet' and 'dcan' branches restated with numpy + scipy, the yardstick of the device
chain - against arrays written out by hand, and the argument checks of the new library entries (they fail before any HIP call)."""
import ctypes as C

import numpy as np
import pytest


def ring_and_blob(ring_id, blob_id):
    """24 x 24: a two-pixel-wide square ring (rows / columns 4..19) around a 4 x 4 blob (10..13)"""
    lab = np.zeros((24, 24), np.int32)
    lab[4:20, 4:20] = ring_id
    lab[6:18, 6:18] = 0
    lab[10:14, 10:14] = blob_id
    return lab


def ring_and_blob_want(ring_id, blob_id):
    """r = 1: the ring grows to 3..20 without its four corner pixels and encloses everything inside it; the blob grows to 9..14 without
    corners and survives only under the larger id"""
    want = np.zeros((24, 24), np.int32)
    want[3:21, 4:20] = ring_id
    want[4:20, 3:21] = ring_id
    if blob_id > ring_id:
        want[9:15, 10:14] = blob_id
        want[10:14, 9:15] = blob_id
    return want


def open_cavity():
    """a U against the top border (bars at columns 5..6 and 13..14 from row 0, bottom rows 8..9): its cavity is open to the image's outside"""
    lab = np.zeros((16, 20), np.int32)
    lab[0:10, 5:7] = 1
    lab[0:10, 13:15] = 1
    lab[8:10, 5:15] = 1
    want = np.zeros((16, 20), np.int32)
    want[0:10, 4:8] = 1
    want[0:10, 12:16] = 1
    want[7:11, 5:15] = 1
    want[8:10, 4:16] = 1                 # rows 0..6 of columns 8..11 stay 0: not a hole
    return lab, want


def neighbours():
    """two 5 x 5 instances one pixel apart: column 8 lies in both dilations and takes the larger id"""
    lab = np.zeros((16, 18), np.int32)
    lab[5:10, 3:8] = 1
    lab[5:10, 9:14] = 2
    want = np.zeros((16, 18), np.int32)
    want[5:10, 2:9] = 1
    want[4:11, 3:8] = 1
    want[5:10, 8:15] = 2
    want[4:11, 9:14] = 2
    return lab, want


def test_redilate_host_hand_cases():
    from cdnet_amd.postproc_other import redilate_host
    for ring_id, blob_id in ((2, 1), (1, 2)):
        got = redilate_host(ring_and_blob(ring_id, blob_id), 1)
        assert got.dtype == np.int32
        np.testing.assert_array_equal(got, ring_and_blob_want(ring_id, blob_id))
        assert got[12, 12] == 2 and got[8, 8] == ring_id
    for lab, want in (open_cavity(), neighbours()):
        np.testing.assert_array_equal(redilate_host(lab, 1), want)


def test_process_host_micronet_by_hand():
    """fill holes -> label -> remove small (the speck keeps id 1 to itself, the block stays 2) -> the cross"""
    from cdnet_amd.postproc_other import process_host
    pred = np.zeros((20, 20), np.float32)
    pred[1, 1] = 0.9                    # a speck below min_size: raster-first, so it takes id 1 and leaves a gap
    pred[5:13, 5:13] = 0.7
    pred[8, 8] = 0.5                    # `> 0.5` is strict: a hole, filled before labelling
    want = np.zeros((20, 20), np.int32)
    want[5:13, 4:14] = 2
    want[4:14, 5:13] = 2
    keep = pred.copy()
    got = process_host(pred, 'micronet')
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(pred, keep)
    want1 = want.copy()
    want1[0:3, 1] = 1
    want1[1, 0:3] = 1
    np.testing.assert_array_equal(process_host(pred, 'micronet', min_size=1), want1)


def test_process_host_dcan_by_hand():
    """a 6 x 6 block of blb - cnt = 0.5 grows by the diamond of radius 3: every pixel within city-block distance 3 of the block"""
    from cdnet_amd.postproc_other import process_host
    pred = np.zeros((26, 26, 2), np.float32)
    pred[10:16, 10:16, 0] = 0.9
    pred[10:16, 10:16, 1] = 0.4
    pred[2:4, 2:4, 0] = 1.0             # 4 pixels: removed by min_size 10
    pred[20:24, 4:8, 0] = 0.9
    pred[20:24, 4:8, 1] = 0.7           # 0.2: below the threshold
    y, x = np.indices((26, 26))
    dist = np.maximum(0, np.maximum(10 - y, y - 15)) + np.maximum(0, np.maximum(10 - x, x - 15))
    want = np.where(dist <= 3, 2, 0).astype(np.int32)
    assert want[7, 12] == 2 and want[8, 8] == 0 and want[9, 8] == 2 and want[8, 9] == 2
    np.testing.assert_array_equal(process_host(pred, 'dcan'), want)
    np.testing.assert_array_equal(process_host(pred.astype(np.float64), 'dcan'), want)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_process_host_dcan_threshold_is_numpys_own(dtype):
    from cdnet_amd.postproc_other import process_host
    t32 = np.float32(0.3)
    values = [dtype(t32), np.nextafter(dtype(t32), dtype(1)), np.nextafter(dtype(t32), dtype(0)),
              dtype(0.3), np.nextafter(dtype(0.3), dtype(1)), np.nextafter(dtype(0.3), dtype(0))]
    seen = set()
    for v in values:
        pred = np.zeros((12, 12, 2), dtype)
        pred[4:8, 4:8, 0] = v
        above = bool((np.full(1, v, dtype) > 0.3)[0])           # numpy's comparison in the array's own type
        seen.add(above)
        got = process_host(pred, 'dcan')
        assert bool(got.any()) == above, (dtype, float(v))
        assert got[6, 6] == (1 if above else 0)
    assert seen == {True, False}
    if dtype is np.float32:
        assert not (np.full(1, t32, np.float32) > 0.3)[0]       # float32(0.3) is NOT above the float32 threshold (it is above the double 0.3)
    else:
        assert (np.full(1, float(t32), np.float64) > 0.3)[0]


def test_process_host_assertions_and_types():
    from cdnet_amd.postproc_other import process_host
    with pytest.raises(AssertionError, match='Prediction shape is not HW'):
        process_host(np.zeros((4, 4, 3), np.float32), 'micronet')
    with pytest.raises(AssertionError, match='Prediction should have contour and blb'):
        process_host(np.zeros((4, 4, 3), np.float32), 'dcan')
    with pytest.raises(AssertionError, match='Prediction should have contour and blb'):
        process_host(np.zeros((4, 4), np.float32), 'dcan')
    with pytest.raises(TypeError):
        process_host(np.zeros((4, 4, 2), np.uint8), 'dcan')
    with pytest.raises(ValueError):
        process_host(np.zeros((4, 4), np.float32), 'unet')


FAKE = C.c_void_p(4096)          # (never dereferenced: every call below fails its argument checks first)


def test_new_entries_reject_bad_arguments_without_a_gpu():
    from cdnet_amd import _lib
    lib = _lib.load()
    err = lambda: lib.cdnet_last_error().decode()
    big = 1 << 30
    args = lambda **kw: [kw.get('label', FAKE), kw.get('N', 1), 64, 64, kw.get('r', 1), kw.get('cap', 100), kw.get('ws', FAKE), kw.get('wsb', big),
                         kw.get('out', C.c_void_p(1 << 20)), kw.get('err', FAKE), None]
    for kw in (dict(label=None), dict(ws=None), dict(out=None), dict(err=None)):
        assert lib.cdnet_instance_redilate(*args(**kw)) == 1 and 'null pointer' in err(), kw
    for kw, what in ((dict(r=0), 'r 0'), (dict(r=4), 'r 4'), (dict(N=0), 'bad size'), (dict(cap=0), 'bad size'), (dict(cap=1 << 29), 'bad size'),
                     (dict(ws=C.c_void_p(4100)), 'aligned'), (dict(out=C.c_void_p(4096 + 64)), 'overlaps')):
        assert lib.cdnet_instance_redilate(*args(**kw)) == 1 and what in err(), (kw, err())
    assert lib.cdnet_instance_redilate(*args(wsb=16)) == 2 and 'workspace' in err()
    need = lib.cdnet_instance_redilate_workspace_bytes(2, 100, 130, 50)
    assert need >= 2 * 50 * 20 + 2 * 2 * 100 * 3 * 8
    assert lib.cdnet_instance_redilate_workspace_bytes(0, 100, 130, 50) == 0 and lib.cdnet_instance_redilate_workspace_bytes(1, 8, 8, 1 << 29) == 0
    assert lib.cdnet_instance_redilate_lds_rows() >= 64 and lib.cdnet_instance_redilate_lds_cols() >= 64

    assert lib.cdnet_label_process(None, 1, 8, 8, 10, FAKE, big, FAKE, None) == 1 and 'null pointer' in err()
    assert lib.cdnet_label_process(FAKE, 1, 8, 8, 10, None, big, FAKE, None) == 1 and 'null pointer' in err()
    assert lib.cdnet_label_process(FAKE, 1, 0, 8, 10, FAKE, big, FAKE, None) == 1 and 'bad size' in err()
    assert lib.cdnet_label_process(FAKE, 1, 8, 8, 10, FAKE, 16, FAKE, None) == 2 and 'workspace' in err()

    assert lib.cdnet_label_count(None, 1, 64, 8, FAKE, FAKE, FAKE, None) == 1 and 'null pointer' in err()
    assert lib.cdnet_label_count(FAKE, 1, 64, 8, FAKE, None, FAKE, None) == 1 and 'null pointer' in err()
    assert lib.cdnet_label_count(FAKE, 1, 64, 0, FAKE, FAKE, FAKE, None) == 1 and 'bad size' in err()
