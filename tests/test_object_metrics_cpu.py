"""No GPU: the host halves of the object-level metrics - stats_utils.aji_plus_from_table, dice2_from_table, size_order and
pair_coordinates - on a numpy pair table against values produced by the reference's stats_utils.py itself (tests/golden/objmetrics.npz,
made by tests/golden/make_golden_objmetrics.py); the work list and work estimate of object_hausdorff; the argument checks of the new
C entries."""
import numpy as np
import pytest


def numpy_pair_table(true, pred):
    """(area_true, area_pred, pairs [K, 3] sorted by (true id, pred id)) with np.bincount / np.unique"""
    t, p = true.astype(np.int64).ravel(), pred.astype(np.int64).ravel()
    cap = int(max(t.max(), p.max())) + 1
    at, ap = np.bincount(t, minlength=cap), np.bincount(p, minlength=cap)
    at[0] = ap[0] = 0
    both = (t > 0) & (p > 0)
    keys, cnt = np.unique(t[both] * 65536 + p[both], return_counts=True)
    return at, ap, np.stack([keys // 65536, keys % 65536, cnt], 1)


def numpy_remap(lab):
    return np.unique(lab, return_inverse=True)[1].reshape(lab.shape).astype(np.int32)


def cases(golden):
    """(name, true, pred remapped in id order, raw prediction) of the four aji.npz cases and of aji_many.npz"""
    z, pp, many = golden('aji'), golden('postproc'), golden('aji_many')
    out = []
    for name in z['names']:
        pred = pp['final_' + str(name)].astype(np.int32)
        out.append((str(name), numpy_remap(z['true_' + str(name)]), numpy_remap(pred), pred))
    out.append(('many', many['true'], many['pred'], many['pred']))
    return out


def test_aji_plus_and_dice2_from_table(golden):
    from cdnet_amd import stats_utils
    z = golden('objmetrics')
    for name, t, p, _ in cases(golden):
        at, ap, pairs = numpy_pair_table(t, p)
        assert abs(stats_utils.aji_plus_from_table(at, ap, pairs) - float(z['ajip_' + name])) < 1e-12, name
        d2 = stats_utils.dice2_from_table(at, ap, pairs)
        assert abs(d2 - float(z['dice2f_' + name])) < 1e-12, name
        if name != 'many':
            assert abs(d2 - float(z['dice2_' + name])) < 1e-12, name


def test_aji_plus_needs_contiguous_ids():
    from cdnet_amd import stats_utils
    t = np.zeros((8, 8), np.int32)
    t[:2, :2], t[4:, 4:] = 1, 3
    with pytest.raises(AssertionError):
        stats_utils.aji_plus_from_table(*numpy_pair_table(t, t))
    r = numpy_remap(t)
    assert stats_utils.aji_plus_from_table(*numpy_pair_table(r, r)) == 1.0
    assert stats_utils.dice2_from_table(*numpy_pair_table(r, r)) == 1.0


def test_size_order_matches_reference(golden):
    from cdnet_amd import stats_utils
    z = golden('objmetrics')
    for raw, want in [(raw, z['bysize_' + name]) for name, _, _, raw in cases(golden)] + [(z['tie_label'], z['tie_bysize'])]:
        lut = stats_utils.size_order(np.bincount(raw.ravel()))
        assert lut.dtype == np.int32 and lut[0] == 0
        assert np.array_equal(lut[raw], want)
    # the tie rule by hand: sizes 12, 30, 12, 30, 6, 12 for ids 2, 3, 5, 7, 9, 12 -> 3, 7 first, then 2, 5, 12 in id order, then 9
    lut = stats_utils.size_order(np.bincount(z['tie_label'].ravel()))
    assert [int(lut[i]) for i in (3, 7, 2, 5, 12, 9)] == [1, 2, 3, 4, 5, 6]
    assert not lut[[0, 1, 4, 6, 8, 10, 11]].any()


def test_pair_coordinates_matches_reference(golden):
    from cdnet_amd import stats_utils
    z = golden('objmetrics')
    pairing, ua, ub = stats_utils.pair_coordinates(z['pc_a'], z['pc_b'], float(z['pc_radius']))
    assert np.array_equal(pairing, z['pc_pairing']) and len(ua) > 0 and len(ub) > 0
    assert ua.dtype == np.int64 and np.array_equal(ua, z['pc_unpaired_a']) and np.array_equal(ub, z['pc_unpaired_b'])


def test_hausdorff_work_list():
    """items cover every source pixel of every selected pair exactly once, tile by tile, and nothing of the others"""
    from cdnet_amd import stats_utils
    cap = 6
    tab_t, tab_p = np.zeros((4, cap), np.int64), np.zeros((4, cap), np.int64)
    tab_t[0], tab_t[1] = [0, 5, 2048, 0, 2049, 1], [0, 4, 100, 0, 90, 1]
    tab_p[0], tab_p[1] = [0, 1024, 1, 3000, 0, 7], [0, 64, 1, 200, 0, 6]
    pairs = np.array([[1, 1], [2, 3], [4, 2], [5, 5], [2, 3]], np.int64)
    work = stats_utils.hausdorff_work(tab_t, tab_p, pairs)
    assert work.tolist() == [1024 * 4 + 5 * 64, 3000 * 100 + 2048 * 200, 1 * 90 + 2049 * 1, 7 * 1 + 1 * 6, 3000 * 100 + 2048 * 200]
    on = np.array([True, True, False, True, True])
    items = stats_utils.hausdorff_items(tab_t, tab_p, pairs, on, 1024)
    assert items.dtype == np.int32
    want = []
    for m in np.flatnonzero(on):
        for d, n in ((0, tab_p[0][pairs[m, 1]]), (1, tab_t[0][pairs[m, 0]])):
            want += [(2 * m + d, k) for k in range(-(-int(n) // 1024))]
    assert [tuple(r) for r in items.tolist()] == want
    assert len(stats_utils.hausdorff_items(tab_t, tab_p, pairs, np.zeros(5, bool), 1024)) == 0


def test_new_entries_check_their_arguments():
    """argument checks return before any HIP call"""
    import ctypes
    from cdnet_amd import _lib
    lib = _lib.load()
    assert lib.cdnet_label_csr_workspace_bytes(1) == 0 and lib.cdnet_label_csr_workspace_bytes(65537) == 0
    assert lib.cdnet_label_csr_workspace_bytes(100) == 800
    tile, chunk = lib.cdnet_hausdorff_tile_pixels(), lib.cdnet_hausdorff_chunk_pixels()
    assert tile >= 64 and chunk >= 64
    buf = ctypes.create_string_buffer(64)
    q = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.cdnet_label_csr(None, 8, 8, 4, q, 64, q, q, q, q, None) == 1 and b'null pointer' in lib.cdnet_last_error()
    assert lib.cdnet_label_csr(q, 8, 32768, 4, q, 64, q, q, q, q, None) == 1 and b'32767' in lib.cdnet_last_error()
    assert lib.cdnet_label_csr(q, 8, 8, 65537, q, 64, q, q, q, q, None) == 1 and b'capacity' in lib.cdnet_last_error()
    assert lib.cdnet_label_csr(q, 8, 8, 100, q, 64, q, q, q, q, None) == 1 and b'workspace' in lib.cdnet_last_error()
    args = [q] * 8 + [8, 8, 4, q, 1, q, 1, q, q, None]
    for k in (0, 7, 11, 15, 16):
        bad = list(args)
        bad[k] = None
        assert lib.cdnet_hausdorff_pairs(*bad) == 1 and b'null pointer' in lib.cdnet_last_error()
    bad = list(args)
    bad[8] = 40000
    assert lib.cdnet_hausdorff_pairs(*bad) == 1 and b'32767' in lib.cdnet_last_error()
    bad = list(args)
    bad[12] = 0
    assert lib.cdnet_hausdorff_pairs(*bad) == 1 and b'count' in lib.cdnet_last_error()
    assert lib.cdnet_label_areas(None, 1, 64, 4, q, q, None) == 1 and lib.cdnet_label_apply(q, 1, 64, 4, None, q, None) == 1
