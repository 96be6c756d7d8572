"""GPU: stats_utils.object_hausdorff (csrc/metrics.hip: per-label coordinate lists + one pair launch) against scipy's directed_hausdorff on
np.argwhere of the two objects, evaluated here - distances must be EQUAL; utils.nuclei_accuracy_object_level against its retained host
helper; get_fast_aji_plus / get_fast_dice_2 / get_dice_2 / remap_label(by_size=True) against values of the reference's stats_utils.py
(tests/golden/objmetrics.npz)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H, W = 48, 80                   # W is no multiple of 64


def scipy_directed(true, pred, pairs):
    """float64 [M, 2]: (h(P -> T), h(T -> P)) by the call the reference makes"""
    from scipy.spatial.distance import directed_hausdorff
    out = np.zeros((len(pairs), 2), np.float64)
    for m, (t, p) in enumerate(pairs):
        a, b = np.argwhere(pred == p), np.argwhere(true == t)
        out[m] = directed_hausdorff(a, b)[0], directed_hausdorff(b, a)[0]
    return out


def boundary_mask(lab):
    """on the image edge, or a 4-neighbour carries another id"""
    pad = np.full((lab.shape[0] + 2, lab.shape[1] + 2), -1, lab.dtype)
    pad[1:-1, 1:-1] = lab
    return (pad[:-2, 1:-1] != lab) | (pad[2:, 1:-1] != lab) | (pad[1:-1, :-2] != lab) | (pad[1:-1, 2:] != lab)


def numpy_tab(lab, cap):
    """rows 0, 1 of cdnet_label_csr's table: pixels and boundary pixels per id"""
    tab = np.zeros((4, cap), np.int64)
    tab[0], tab[1] = np.bincount(lab.ravel(), minlength=cap), np.bincount(lab[boundary_mask(lab)], minlength=cap)
    tab[:, 0] = 0
    return tab


def assert_equal_to_scipy(true, pred, pairs, **kw):
    from cdnet_amd import stats_utils
    pairs = np.asarray(pairs, dtype=np.int64)
    want = scipy_directed(true, pred, pairs)
    got = stats_utils.object_hausdorff(true, pred, pairs, **kw)
    assert got.dtype == np.float64 and got.shape == (len(pairs),)
    assert np.array_equal(got, want.max(1)), (got, want.max(1))
    sq = stats_utils.object_hausdorff(true, pred, pairs, squared_directed=True, **kw)
    assert sq.dtype == np.int64 and sq.shape == (len(pairs), 2)
    assert np.array_equal(np.sqrt(sq.astype(np.float64)), want), (sq, want)
    return got, sq


def hand_built():
    """(true, pred, {name: (true id, pred id)}) in one 48 x 80 image pair"""
    yy, xx = np.mgrid[:H, :W]
    t, p = np.zeros((H, W), np.int32), np.zeros((H, W), np.int32)
    pairs = {}
    t[2:7, 10:16] = p[2:7, 10:16] = 2                                   # identical
    pairs['identical'] = (2, 2)
    p[10:13, 12:15], t[8:16, 9:19] = 3, 3                               # pred strictly inside true
    pairs['nested'] = (3, 3)
    r2 = (yy - 30) ** 2 + (xx - 20) ** 2
    p[r2 <= 9], t[(r2 >= 49) & (r2 <= 100)] = 4, 4                      # a disk inside a ring, 4 pixels of gap
    pairs['disk_in_ring'] = (4, 4)
    t[20, 40], p[21, 41] = 5, 5                                         # two pixels on a diagonal
    pairs['diagonal'] = (5, 5)
    t[0, 0], p[H - 1, W - 1] = 6, 6                                     # opposite corners
    pairs['corners'] = (6, 6)
    t[H - 2, :] = 7                                                     # a line as long as W against a short stub below it
    p[H - 1, 30:34] = 7
    pairs['line'] = (7, 7)
    t[3:5, 30:33], t[16:18, 70:74] = 8, 8                               # ids in several far-apart pieces, disjoint from each other
    p[9:11, 50:52], p[36:39, 60:62] = 8, 8
    pairs['pieces'] = (8, 8)
    t[24:28, 50:56], p[25:30, 52:58] = 1, 65535                         # the id limits, partly overlapping
    p[40:42, 2:5], t[41:44, 3:9] = 1, 65535
    pairs['id_limits'] = (1, 65535)
    pairs['id_limits_swapped'] = (65535, 1)
    pairs['twice'] = (3, 4)                                             # ids 3 and 4 again, in another combination
    assert not ((t == 7) & (p == 8)).any()
    return t, p, pairs


def test_hand_built_pairs():
    t, p, named = hand_built()
    names = list(named)
    got, sq = assert_equal_to_scipy(t, p, [named[n] for n in names])
    d = dict(zip(names, got))
    s = dict(zip(names, sq.tolist()))
    assert d['identical'] == 0.0 and s['identical'] == [0, 0]
    assert s['nested'][0] == 0 and s['nested'][1] == 3 ** 2 + 4 ** 2            # pred in true: P -> T is 0; true's corner (15, 18) to (12, 14)
    assert s['disk_in_ring'][0] == 49                                          # the disk's centre to the ring's inner edge (radius 7)
    assert d['diagonal'] == np.sqrt(2.0)
    assert s['corners'] == [(H - 1) ** 2 + (W - 1) ** 2] * 2
    assert s['line'] == [1, 1 + 46 ** 2]                                       # the line's far end (46, 79) to the stub's (47, 33)


def test_torch_inputs_and_repeated_ids():
    import torch
    from cdnet_amd import stats_utils
    t, p, named = hand_built()
    pairs = np.array([named['nested'], named['twice'], named['nested'], named['disk_in_ring']], np.int64)
    want = scipy_directed(t, p, pairs).max(1)
    got = stats_utils.object_hausdorff(torch.from_numpy(t).cuda(), torch.from_numpy(p).cuda(), pairs)
    assert np.array_equal(got, want) and got[0] == got[2]
    assert stats_utils.object_hausdorff(t, p, np.zeros((0, 2), np.int64)).shape == (0,)


def test_objects_beyond_every_staging_unit():
    """a 96 x 128 chequerboard under one id (6144 pixels, every one a boundary pixel) against a solid 96 x 128 block offset by (5, 7):
    more source pixels than one block's register tile and more boundary pixels than one LDS pass, in both directions' roles"""
    from cdnet_amd import stats_utils
    tile, chunk = stats_utils.hausdorff_limits()
    yy, xx = np.mgrid[:96, :128]
    t, p = np.zeros((112, 150), np.int32), np.zeros((112, 150), np.int32)
    t[:96, :128][(yy + xx) % 2 == 0] = 9
    p[5:101, 7:135] = 4
    assert (t == 9).sum() == 6144 and 6144 > 2 * tile and 6144 > 2 * chunk
    assert (p == 4).sum() == 96 * 128 > 2 * tile
    _, sq = assert_equal_to_scipy(t, p, [(9, 4)])
    assert sq.tolist() == [[5 ** 2 + 7 ** 2, 5 ** 2 + 7 ** 2]]               # P -> T from (100, 134) to (95, 127); T -> P from (0, 0) to (5, 7)
    # the same with sizes that are no multiple of either unit: the last tile and the last pass are ragged
    t[...], p[...] = 0, 0
    t[:75, :101][(yy[:75, :101] + xx[:75, :101]) % 2 == 0] = 9
    p[30:105, 40:141] = 4
    n = int((t == 9).sum())
    assert n > 2 * tile and n > 2 * chunk and n % tile and n % chunk and 75 * 101 % tile
    assert_equal_to_scipy(t, p, [(9, 4)])


@pytest.fixture(scope='module')
def ellipses():
    """about 600 small instances against a copy shifted by (1, 2) with every 7th id dropped"""
    from cdnet_amd import synth
    true = synth.ellipse_instances(200, 240, 3000, np.random.RandomState(1), rmin=2, rmax=5, margin=6)
    pred = np.roll(np.roll(true, 1, axis=0), 2, axis=1)
    lut = np.arange(int(true.max()) + 1, dtype=np.int32)
    lut[7::7] = 0
    return true, lut[pred]


def test_every_overlapping_pair(ellipses):
    from cdnet_amd import stats_utils
    true, pred = ellipses
    pairs = stats_utils.pair_table(true, pred)[2][:, :2]
    assert len(pairs) > 500 and len(np.unique(pairs[:, 0])) < len(pairs)        # neighbours overlap too: ids occur in several pairs
    assert_equal_to_scipy(true, pred, pairs)


def test_max_work_guard_gives_the_same():
    from cdnet_amd import stats_utils
    t, p, named = hand_built()
    pairs = np.array(list(named.values()), np.int64)
    for sq in (False, True):
        host = stats_utils.object_hausdorff(t, p, pairs, squared_directed=sq, max_work=1)
        dev = stats_utils.object_hausdorff(t, p, pairs, squared_directed=sq)
        part = stats_utils.object_hausdorff(t, p, pairs, squared_directed=sq, max_work=2000)     # some pairs on each side
        assert host.dtype == dev.dtype and np.array_equal(host, dev) and np.array_equal(part, dev)
    work = stats_utils.hausdorff_work(numpy_tab(t, 65536), numpy_tab(p, 65536), pairs)
    assert work.min() > 1 and np.sort(work)[:3].sum() < 2000 < work.sum()


def test_label_lists_match_numpy(ellipses):
    """cdnet_label_csr: counts, boundary counts, segment starts and the pixel sets of every segment (the order inside one is free)"""
    import torch
    from cdnet_amd import stats_utils
    t, _, _ = hand_built()
    for lab in (t, ellipses[0]):
        cap = int(lab.max()) + 1
        tab, pix, bpix = [a.cpu().numpy() for a in stats_utils.label_csr(torch.from_numpy(lab).cuda(), cap)]
        want = numpy_tab(lab, cap)
        assert np.array_equal(tab[:2], want[:2])
        for row in (0, 1):
            assert np.array_equal(tab[2 + row], np.cumsum(want[row]) - want[row])
        bd = boundary_mask(lab)
        for i in np.flatnonzero(want[0]):
            seg = pix[tab[2][i]: tab[2][i] + tab[0][i]]
            assert np.array_equal(np.sort(seg), np.sort((np.argwhere(lab == i) * [65536, 1]).sum(1)))
            bseg = bpix[tab[3][i]: tab[3][i] + tab[1][i]]
            assert np.array_equal(np.sort(bseg), np.sort((np.argwhere((lab == i) & bd) * [65536, 1]).sum(1)))


def test_absent_and_oversize_ids_are_refused():
    from cdnet_amd import stats_utils
    t, p, _ = hand_built()
    for bad in ([(9, 2)], [(2, 9)], [(2, 2), (0, 2)], [(2, 65536)], [(70000, 2)], [(-1, 2)], [(2, 40000)]):
        with pytest.raises(ValueError):
            stats_utils.object_hausdorff(t, p, np.array(bad, np.int64))
        with pytest.raises(ValueError):
            stats_utils.object_hausdorff(t, p, np.array(bad, np.int64), max_work=1)
    over = p.copy()
    over[0, 5] = 65536
    with pytest.raises(ValueError):
        stats_utils.object_hausdorff(t, over, np.array([(2, 2)], np.int64))
    neg = t.copy()
    neg[0, 5] = -2
    with pytest.raises(ValueError):
        stats_utils.object_hausdorff(neg, p, np.array([(2, 2)], np.int64))


def test_nuclei_accuracy_object_level_equals_host_helper(ellipses):
    from cdnet_amd import utils
    true, pred = ellipses
    got, want = utils.nuclei_accuracy_object_level(pred, true), utils.nuclei_accuracy_object_level_host(pred, true)
    assert len(got) == 7 and want[5] > 0
    assert [float(v) for v in got] == [float(v) for v in want]


def test_aji_plus_dice2_and_by_size_match_reference(golden):
    import torch
    from cdnet_amd import stats_utils
    z, a, pp, many = golden('objmetrics'), golden('aji'), golden('postproc'), golden('aji_many')
    cases = [(str(n), a['true_' + str(n)], pp['final_' + str(n)].astype(np.int32)) for n in a['names']] + [('many', many['true'], many['pred'])]
    for name, true, pred in cases:
        t, p = stats_utils.remap_label(true.copy()), stats_utils.remap_label(pred.copy())
        for tt, pq in ((t, p), (torch.from_numpy(t).cuda(), torch.from_numpy(p).cuda())):
            assert abs(stats_utils.get_fast_aji_plus(tt, pq) - float(z['ajip_' + name])) < 1e-12
            assert abs(stats_utils.get_fast_dice_2(tt, pq) - float(z['dice2f_' + name])) < 1e-12
            if name != 'many':
                assert abs(stats_utils.get_dice_2(tt, pq) - float(z['dice2_' + name])) < 1e-12
        r = stats_utils.remap_label(pred.copy(), by_size=True)
        assert isinstance(r, np.ndarray) and r.dtype == np.int32 and np.array_equal(r, z['bysize_' + name])
        rt = stats_utils.remap_label(torch.from_numpy(pred).cuda(), by_size=True)
        assert torch.is_tensor(rt) and rt.is_cuda and np.array_equal(rt.cpu().numpy(), z['bysize_' + name])


def test_by_size_ties_and_empty_image(golden):
    import torch
    from cdnet_amd import stats_utils
    z = golden('objmetrics')
    lab = z['tie_label']
    assert np.array_equal(stats_utils.remap_label(lab.copy(), by_size=True), z['tie_bysize'])
    assert np.array_equal(stats_utils.remap_label(torch.from_numpy(lab).cuda(), by_size=True).cpu().numpy(), z['tie_bysize'])
    empty = np.zeros((16, 24), np.int32)
    assert stats_utils.remap_label(empty, by_size=True) is empty
    et = torch.from_numpy(empty).cuda()
    assert stats_utils.remap_label(et, by_size=True) is et
    bad = lab.copy()
    bad[0, 0] = -3
    with pytest.raises(ValueError):
        stats_utils.remap_label(bad, by_size=True)
