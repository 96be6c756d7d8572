"""GPU: cdnet_amd.stats_utils (AJI / PQ / Dice / remap_label over csrc/metrics.hip) against values produced by the
reference's stats_utils.py itself (tests/golden/aji.npz and aji_many.npz, made by tests/golden/make_golden.py:gen_aji / gen_aji_many),
and the device pass (label ranks, areas, pair table) against plain numpy where those fixtures do not reach: ids beyond one 256-wide
strip of the rank scan, more pairs than the first table holds, ids next to the 16-bit limit of the pair key, ids out of range."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_matches_reference_values(golden):
    from cdnet_amd import stats_utils
    z, pp = golden('aji'), golden('postproc')
    for name in z['names']:
        pred, true = pp['final_' + str(name)].astype(np.int32), z['true_' + str(name)]
        p, t = stats_utils.remap_label(pred.copy()), stats_utils.remap_label(true.copy())
        aji = stats_utils.get_fast_aji(t, p)
        assert abs(aji[0] - float(z['aji_' + str(name)])) < 1e-12
        assert abs(stats_utils.get_dice_1(t, p) - float(z['dice_' + str(name)])) < 1e-12
        np.testing.assert_allclose(stats_utils.get_fast_pq(t, p)[0], z['pq_' + str(name)], rtol=0, atol=1e-12)


def test_remap_label_and_properties():
    import torch
    from cdnet_amd import stats_utils
    rs = np.random.RandomState(0)
    lab = np.zeros((64, 80), np.int32)
    ids = [3, 7, 8, 20, 41]
    for k, i in enumerate(ids):
        lab[5 + 10 * k: 12 + 10 * k, 4 + 12 * k: 14 + 12 * k] = i
    r = stats_utils.remap_label(lab)
    assert sorted(np.unique(r)) == [0, 1, 2, 3, 4, 5]
    for k, i in enumerate(ids):
        assert (r[lab == i] == k + 1).all()
    # identical images: AJI = PQ = Dice = 1
    assert abs(stats_utils.get_fast_aji(r, r)[0] - 1.0) < 1e-12
    assert abs(stats_utils.get_dice_1(r, r) - 1.0) < 1e-12
    np.testing.assert_allclose(stats_utils.get_fast_pq(r, r)[0], [1.0, 1.0 / (1 + 1e-6 / 5), 1.0 / (1 + 1e-6 / 5)], rtol=1e-9)
    # torch CUDA inputs are accepted as well
    t = torch.from_numpy(r).cuda()
    assert abs(stats_utils.get_fast_aji(t, t)[0] - 1.0) < 1e-12


def test_nuclei_accuracy_object_level_matches_reference(golden):
    """utils.nuclei_accuracy_object_level (greedy per-object matching, Hausdorff, AJI) vs the values of the reference's own function
    (tests/golden/aji.npz `obj_*`, made with the measure.label stand-in of tests/golden/_ref_shims.py)"""
    from cdnet_amd import utils
    z, pp = golden('aji'), golden('postproc')
    for name in z['names']:
        pred, true = pp['final_' + str(name)].astype(np.int32), z['true_' + str(name)]
        got = utils.nuclei_accuracy_object_level(pred, true)
        np.testing.assert_allclose(np.array(got, dtype=np.float64), z['obj_' + str(name)], rtol=1e-12, atol=1e-12)


def _numpy_pair_table(true, pred):
    """(area_true, area_pred, pairs [K, 3] sorted by (true id, pred id)) with np.bincount / np.unique"""
    t, p = true.astype(np.int64).ravel(), pred.astype(np.int64).ravel()
    cap = int(max(t.max(), p.max())) + 1
    at, ap = np.bincount(t, minlength=cap), np.bincount(p, minlength=cap)
    at[0] = ap[0] = 0
    both = (t > 0) & (p > 0)
    keys, cnt = np.unique(t[both] * 65536 + p[both], return_counts=True)
    return at, ap, np.stack([keys // 65536, keys % 65536, cnt], 1)


def _assert_pair_table(true, pred):
    from cdnet_amd import stats_utils
    at, ap, pairs = stats_utils.pair_table(true, pred)
    wt, wp, wpairs = _numpy_pair_table(true, pred)
    assert np.array_equal(at, wt) and np.array_equal(ap, wp)
    assert pairs.shape == wpairs.shape and np.array_equal(pairs, wpairs)
    return pairs


def test_remap_label_across_rank_strips():
    """ids in several 256-wide strips of label_rank_kernel, on both sides of each strip border, and one beyond 16 bits: the carry"""
    import torch
    from cdnet_amd import stats_utils
    ids = [1, 255, 256, 257, 511, 512, 513, 1000, 70000]
    lab = np.zeros((64, 80), np.int32)
    for k, i in enumerate(ids):
        lab[3 + 6 * k: 8 + 6 * k, 2 + 8 * k: 9 + 8 * k] = i
    lab[60:, 70:] = 513                                     # a second region of one id
    want = np.unique(lab, return_inverse=True)[1].reshape(lab.shape).astype(np.int32)      # ranks in id order, 0 stays 0
    assert want.max() == 9
    r = stats_utils.remap_label(lab.copy())
    assert isinstance(r, np.ndarray) and np.array_equal(r, want)
    rt = stats_utils.remap_label(torch.from_numpy(lab).cuda())
    assert torch.is_tensor(rt) and rt.is_cuda and np.array_equal(rt.cpu().numpy(), want)
    bad = lab.copy()
    bad[0, 0] = -3
    with pytest.raises(ValueError):
        stats_utils.remap_label(bad)


def test_pair_table_regrows():
    """99 x 99 pixels, every one a pair of its own: 9 801 pairs against the 4 096 slots of the first table"""
    true = np.repeat(np.arange(1, 100, dtype=np.int32)[:, None], 99, 1)
    pred = np.repeat(np.arange(1, 100, dtype=np.int32)[None, :], 99, 0)
    pairs = _assert_pair_table(true, pred)
    assert pairs.shape == (9801, 3) and (pairs[:, 2] == 1).all()
    assert np.array_equal(pairs[:, 0] * 100 + pairs[:, 1], np.sort(pairs[:, 0] * 100 + pairs[:, 1]))


def test_pair_table_id_limits():
    """ids 1 and 65535 in both images: capacity 65536, the key 0xFFFFFFFF; 65536 and negative ids are refused"""
    from cdnet_amd import stats_utils
    true = np.zeros((16, 24), np.int32)
    pred = np.zeros((16, 24), np.int32)
    true[:8, :12], true[8:, 12:] = 1, 65535
    pred[:8, 6:18], pred[4:, 10:] = 1, 65535
    pairs = _assert_pair_table(true, pred)
    assert [tuple(p[:2]) for p in pairs] == [(1, 1), (1, 65535), (65535, 65535)]
    over = pred.copy()
    over[0, 0] = 65536
    with pytest.raises(ValueError):
        stats_utils.pair_table(true, over)
    neg = pred.copy()
    neg[15, 23] = -1
    with pytest.raises(ValueError):
        stats_utils.pair_table(true, neg)
    with pytest.raises(ValueError):
        stats_utils.pair_table(neg, pred)


def test_pair_table_hundreds_of_instances():
    """two unrelated label images of about 600 instances each: the whole table against numpy"""
    from cdnet_amd import synth
    true = synth.ellipse_instances(200, 240, 3000, np.random.RandomState(1), rmin=2, rmax=5, margin=6)
    pred = synth.ellipse_instances(200, 240, 3000, np.random.RandomState(2), rmin=2, rmax=5, margin=6)
    assert true.max() > 500 and pred.max() > 500
    pairs = _assert_pair_table(true, pred)
    assert len(pairs) > 600


def test_matches_reference_values_many_instances(golden):
    """one 384 x 384 pair with more than 512 instances in each image (aji.npz stops at 76): the same bars as above"""
    from cdnet_amd import stats_utils
    z = golden('aji_many')
    t, p = z['true'], z['pred']
    assert t.max() > 512 and p.max() > 512
    assert np.array_equal(stats_utils.remap_label(t.copy()), t) and np.array_equal(stats_utils.remap_label(p.copy()), p)
    np.testing.assert_allclose(np.array(stats_utils.get_fast_aji(t, p), dtype=np.float64), z['aji'], rtol=0, atol=1e-12)
    assert abs(stats_utils.get_dice_1(t, p) - float(z['dice'])) < 1e-12
    np.testing.assert_allclose(stats_utils.get_fast_pq(t, p)[0], z['pq'], rtol=0, atol=1e-12)
