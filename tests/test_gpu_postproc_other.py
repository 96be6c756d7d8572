"""GPU: cdnet_instance_redilate (csrc/instance_fill.hip) and postproc_other.process for 'micronet' / 'dcan' against
postproc_other.process_host / redilate_host - the reference's per-instance whole-image loop restated with scipy - bit for bit."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _dev(lab, r, cap=None):
    import torch
    from cdnet_amd import postproc_other
    out = postproc_other.redilate_instances(torch.from_numpy(np.ascontiguousarray(lab, np.int32)).cuda(), r, cap)
    assert out.dtype == torch.int32 and out.is_cuda and tuple(out.shape) == lab.shape
    return out.cpu().numpy()


def _same(lab, r, cap=None):
    from cdnet_amd.postproc_other import redilate_host
    got = _dev(lab, r, cap)
    np.testing.assert_array_equal(got, redilate_host(lab, r))
    return got


def _blobs(H, W, n, seed, rmin=4, rmax=11):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[:H, :W]
    m = np.zeros((H, W), bool)
    for _ in range(n):
        cy, cx, r = rs.randint(0, H), rs.randint(0, W), rs.randint(rmin, rmax)
        m |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    return m.astype(np.uint8)


def _holes(H, W, n, seed):
    """blobs with punched holes (some touching the border) and specks below the size threshold (as tests/test_gpu_watershed.py builds them)"""
    rs = np.random.RandomState(seed)
    m = _blobs(H, W, n, seed, 5, 14)
    yy, xx = np.mgrid[:H, :W]
    for _ in range(n):
        cy, cx, r = rs.randint(0, H), rs.randint(0, W), rs.randint(1, 4)
        m[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 0
    for _ in range(n):
        m[rs.randint(0, H), rs.randint(0, W)] = 1
    return m


def _instances(H, W, n, seed):
    """a label map of holed blobs with shuffled ids, so that overlapping dilations meet in both id orders"""
    from scipy import ndimage as ndi
    lab, k = ndi.label(_holes(H, W, n, seed))
    perm = np.concatenate([[0], np.random.RandomState(seed + 7).permutation(k) + 1])
    return perm[lab].astype(np.int32)


def _spiral(m, corridor, wall):
    """a square block with a spiral corridor: coarse cells of width `wall` (even indices) and `corridor` (odd indices), the corridor's mouth
    on the block's top edge"""
    a = np.ones((m, m), np.int32)
    a[0, 1] = 0
    t, b, l, r = 1, m - 2, 1, m - 2
    start = l
    while t <= b and l <= r:
        a[t, start:r + 1] = 0
        a[t:b + 1, r] = 0
        a[b, l:r + 1] = 0
        if t + 2 > b - 2:
            break
        a[t + 2:b + 1, l] = 0
        start = l
        t, b, l, r = t + 2, b - 2, l + 2, r - 2
    reps = [wall if i % 2 == 0 else corridor for i in range(m)]
    return np.repeat(np.repeat(a, reps, 0), reps, 1)


def test_hand_cases():
    from test_postproc_other_host import neighbours, open_cavity, ring_and_blob, ring_and_blob_want
    for ring_id, blob_id in ((2, 1), (1, 2)):
        np.testing.assert_array_equal(_dev(ring_and_blob(ring_id, blob_id), 1), ring_and_blob_want(ring_id, blob_id))
        _same(ring_and_blob(ring_id, blob_id), 3)
    for lab, want in (open_cavity(), neighbours()):
        np.testing.assert_array_equal(_dev(lab, 1), want)
        _same(lab, 2)
        _same(lab, 3)


def test_borders_zero_image_and_one_pixel():
    frame = np.zeros((20, 30), np.int32)
    frame[0, :] = frame[-1, :] = frame[:, 0] = frame[:, -1] = 4             # touches all four borders: the whole image is its hole
    for r in (1, 3):
        assert (_same(frame, r) == 4).all()
        assert not _same(np.zeros((17, 70), np.int32), r).any()
        _same(np.full((9, 67), 2, np.int32), r)
        one = np.zeros((12, 12), np.int32)
        one[0, 0], one[11, 5], one[6, 6] = 1, 2, 3
        _same(one, r)
    _same(np.array([[5]], np.int32), 1)
    _same(np.array([[0, 1, 0, 0, 2, 2]], np.int32), 3)


@pytest.mark.parametrize('case', [(33, 65, 6, 5), (50, 120, 20, 3), (64, 64, 10, 1), (96, 80, 24, 2), (128, 128, 40, 4)])
def test_random_instance_maps(case):
    H, W, n, seed = case
    lab = _instances(H, W, n, seed)
    assert lab.max() >= 2
    for r in (1, 2, 3):
        _same(lab, r)


def test_ring_across_a_word_boundary():
    """the ring's window starts at column 45 (r = 1) / 43 (r = 3), not a multiple of 64, and ends beyond column 64 of the window"""
    lab = np.zeros((48, 150), np.int32)
    lab[6:40, 46:126] = 3
    lab[9:37, 49:123] = 0
    lab[12:20, 60:70] = 1                # inside the ring: swallowed
    lab[24:30, 100:118] = 7              # inside the ring, larger id: survives
    lab[20:23, 108:112] = 0
    lab[2:5, 2:140] = 2                  # a long thin instance over three words
    for r in (1, 3):
        got = _same(lab, r)
        assert got[15, 65] == 3 and got[26, 105] == 7


def test_spiral_corridors_converge():
    """the worst case of the pass loop: a one-pixel spiral corridor.  In the label map itself it is closed by the dilation; three pixels wide
    with one-pixel walls it is one pixel wide in D_k for r = 1 - 15 turns the flood has to follow.  No error flag: redilate_instances raises
    on one."""
    lab = np.zeros((72, 135), np.int32)
    lab[4:68, 40:104] = 5 * _spiral(64, 1, 1)
    for r in (1, 3):
        _same(lab, r)
    block = _spiral(31, 3, 1)
    assert block.shape == (61, 61)
    lab = np.zeros((70, 135), np.int32)
    lab[5:66, 38:99] = 6 * block
    got = _same(lab, 1)
    assert (got[5:66, 38:99] == 0).sum() > 300          # the corridor stays open: not a hole
    lab[5, 38:99] = 6                                   # the mouth closed: now it is one
    got = _same(lab, 1)
    assert (got[5:66, 38:99] == 6).all()
    _same(lab, 3)


def test_sparse_ids_cap_and_error_flag():
    import torch
    from cdnet_amd import postproc_other
    lab = np.zeros((40, 90), np.int32)
    lab[5:12, 5:14] = 3
    lab[5:12, 16:30] = 2500
    lab[20:30, 60:85] = 1000
    lab[22:28, 62:83] = 0
    lab[24:26, 70:74] = 12
    _same(lab, 1)
    _same(lab, 3, cap=100000)
    _same(lab, 3, cap=2500)
    with pytest.raises(ValueError, match='outside'):
        postproc_other.redilate_instances(torch.from_numpy(lab).cuda(), 1, cap=2499)
    neg = lab.copy()
    neg[0, 0] = -1
    with pytest.raises(ValueError, match='outside'):
        postproc_other.redilate_instances(torch.from_numpy(neg).cuda(), 1)
    with pytest.raises(Exception, match='r 4'):
        postproc_other.redilate_instances(torch.from_numpy(lab).cuda(), 4)


def test_batch_of_three():
    from cdnet_amd.postproc_other import redilate_host
    batch = np.stack([_instances(50, 120, 12, 21), _instances(50, 120, 5, 22), np.zeros((50, 120), np.int32)])
    batch[1][batch[1] > 0] += 40
    for r in (1, 3):
        got = _dev(batch, r)
        for i in range(3):
            np.testing.assert_array_equal(got[i], redilate_host(batch[i], r))


def test_window_just_past_the_lds_capacity():
    """a thin ring on the border of an image one pixel larger than the LDS form's window in each dimension: the workspace form runs, next to
    small instances in the LDS form"""
    from cdnet_amd import postproc_other
    rows, cols = postproc_other.redilate_limits()
    H, W = rows + 1, cols + 1
    lab = np.zeros((H, W), np.int32)
    lab[0, :] = lab[-1, :] = lab[:, 0] = lab[:, -1] = 2
    lab[10:20, 10:24] = 1
    lab[40:52, 60:70] = 3
    lab[44:47, 63:66] = 0
    lab[H - 1, W // 2] = 0                              # a gap in the ring: closed by the dilation
    for r in (1, 3):
        got = _same(lab, r)
        assert got[15, 15] == 2 and got[45, 64] == 3 and got[H // 2, W // 2] == 2
    lab[H - 6:, W // 2 - 3:W // 2 + 4] = 0              # a gap wider than 2 r: the ring is open, nothing inside it is a hole
    got = _same(lab, 3)
    assert got[H // 2, W // 2] == 0 and got[15, 15] == 1
    # at the capacity itself (the LDS form's largest window), same picture
    lab = np.zeros((rows, cols), np.int32)
    lab[0, :] = lab[-1, :] = lab[:, 0] = lab[:, -1] = 2
    lab[100:110, 100:130] = 5
    _same(lab, 3)


@pytest.mark.parametrize('case', [(64, 64, 10, 1), (96, 80, 24, 2), (50, 120, 20, 3), (128, 128, 40, 4), (33, 65, 6, 5)])
def test_process_micronet_and_dcan(case):
    import torch
    from cdnet_amd import postproc_other
    H, W, n, seed = case
    m = _holes(H, W, n, seed)
    pred = m.astype(np.float32) * 0.8
    for min_size in (10, 3):
        want = postproc_other.process_host(pred, 'micronet', min_size=min_size)
        got = postproc_other.process(pred.copy(), 'micronet', min_size=min_size, ws=True)           # (ws is forced off, postproc_other.py:35)
        assert isinstance(got, np.ndarray) and got.dtype == np.int32
        np.testing.assert_array_equal(got, want)
    got = postproc_other.process(torch.from_numpy(m).cuda(), 'micronet')
    assert torch.is_tensor(got) and got.is_cuda and got.dtype == torch.int32
    np.testing.assert_array_equal(got.cpu().numpy(), postproc_other.process_host(pred, 'micronet'))
    # dcan: blb = the blobs, cnt = a contour map that cuts some of them
    rs = np.random.RandomState(seed)
    blb = m.astype(np.float32) * (0.6 + 0.4 * rs.rand(H, W).astype(np.float32))
    cnt = (_blobs(H, W, n, seed + 50, 2, 5) * rs.rand(H, W)).astype(np.float32)
    dc = np.stack([blb, cnt], axis=-1)
    for dtype in (np.float32, np.float64):
        want = postproc_other.process_host(dc.astype(dtype), 'dcan')
        got = postproc_other.process(dc.astype(dtype), 'dcan')
        assert isinstance(got, np.ndarray) and got.dtype == np.int32 and got.shape == (H, W)
        np.testing.assert_array_equal(got, want)
    assert want.max() >= 1
    got = postproc_other.process(torch.from_numpy(dc).cuda(), 'dcan', min_size=4)
    assert torch.is_tensor(got) and got.is_cuda and got.dtype == torch.int32
    np.testing.assert_array_equal(got.cpu().numpy(), postproc_other.process_host(dc, 'dcan', min_size=4))


def test_process_batches_threshold_and_refusals():
    import torch
    from cdnet_amd import postproc_other
    H, W = 40, 72
    ms = [_holes(H, W, 8, 31), _holes(H, W, 5, 32), np.zeros((H, W), np.uint8)]
    got = postproc_other.process(torch.from_numpy(np.stack(ms)).cuda(), 'micronet')
    assert tuple(got.shape) == (3, H, W)
    for i in range(3):
        np.testing.assert_array_equal(got[i].cpu().numpy(), postproc_other.process_host(ms[i].astype(np.float32), 'micronet'))
    dcs = [np.stack([m.astype(np.float32), 0.5 * _blobs(H, W, 6, 40 + i, 2, 5).astype(np.float32)], -1) for i, m in enumerate(ms)]
    got = postproc_other.process(np.stack(dcs), 'dcan')
    assert isinstance(got, np.ndarray) and got.shape == (3, H, W)
    for i in range(3):
        np.testing.assert_array_equal(got[i], postproc_other.process_host(dcs[i], 'dcan'))
    # the threshold in the array's own type: float32(0.3) and its neighbours, 0.3 and its neighbours
    for dtype in (np.float32, np.float64):
        t32 = np.float32(0.3)
        vals = [dtype(t32), np.nextafter(dtype(t32), dtype(1)), np.nextafter(dtype(t32), dtype(0)),
                dtype(0.3), np.nextafter(dtype(0.3), dtype(1)), np.nextafter(dtype(0.3), dtype(0))]
        pred = np.zeros((len(vals), 12, 12, 2), dtype)
        for i, v in enumerate(vals):
            pred[i, 4:8, 4:8, 0] = v
        got = postproc_other.process(pred, 'dcan')
        for i, v in enumerate(vals):
            np.testing.assert_array_equal(got[i], postproc_other.process_host(pred[i], 'dcan'))
            assert bool(got[i].any()) == bool((np.full(1, v, dtype) > 0.3)[0]), (dtype, i)
    with pytest.raises(AssertionError, match='Prediction should have contour and blb'):
        postproc_other.process(np.zeros((8, 8, 3), np.float32), 'dcan')
    with pytest.raises(AssertionError, match='Prediction shape is not HW'):
        postproc_other.process(np.zeros((2, 2, 8, 8), np.float32), 'micronet')
    with pytest.raises(TypeError):
        postproc_other.process(np.zeros((8, 8, 2), np.uint8), 'dcan')


def test_label_count():
    import torch
    from cdnet_amd import postproc
    lab = np.stack([_instances(50, 120, 12, 21) * 3, np.zeros((50, 120), np.int32), _instances(50, 120, 5, 22)])
    counts, err = postproc.label_count(torch.from_numpy(lab).cuda(), 3000)
    assert int(err.item()) == 0
    assert counts.cpu().tolist() == [len(np.unique(a[a > 0])) for a in lab]
    _, err = postproc.label_count(torch.from_numpy(lab).cuda(), 5)
    assert int(err.item()) == 1
