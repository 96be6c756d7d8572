"""Regenerate tests/golden/objmetrics.npz: the reference's get_fast_aji_plus (stats_utils.py:108-178), get_fast_dice_2 (:279-317),
get_dice_2 (:338-357), remap_label(by_size=True) (:361-389) and pair_coordinates (:393-439) on the label images the other metric fixtures
use, plus two hand-built inputs.

CONTAINER-ONLY: imports the reference's stats_utils from /root/reference (read-only, never copied) through _ref_shims.  The fixture holds
data only.

    python tests/golden/make_golden_objmetrics.py

Inputs
  the four cases of aji.npz: prediction = postproc.npz 'final_<name>', truth = aji.npz 'true_<name>', both through the reference's
      remap_label first (what tests/test_gpu_metrics.py does on the device).
  aji_many.npz 'true' / 'pred' (more than 512 instances each, already contiguous).  get_dice_2 is left out there: the reference compares
      every true mask with every predicted mask over the whole image.
  'tie': a 24 x 40 image by hand whose ids-by-size order is NOT the id order and has equal areas: id 2 (12 px), 3 (30 px), 5 (12 px),
      7 (30 px), 9 (6 px), 12 (12 px); sorted(..., reverse=True) is stable, so equal sizes keep id order: 3, 7, 2, 5, 12, 9.
  'pc': thirteen points A and twelve points B (float32 XY) and radius 3: some pairs lie further apart than the radius and stay unpaired.

Keys: per aji.npz case '<name>' and for 'many': 'ajip_<name>' f64, 'dice2f_<name>' f64 (get_fast_dice_2), 'dice2_<name>' f64 (get_dice_2;
not for 'many'), 'bysize_<name>' i32 [H,W] (remap_label(pred, by_size=True) of the un-remapped prediction).  'tie_label' i32,
'tie_bysize' i32.  'pc_a', 'pc_b' f32 [n,2], 'pc_radius' f64, 'pc_pairing' i64 [k,2], 'pc_unpaired_a', 'pc_unpaired_b' i64.  'names'.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_shims  # noqa: E402


def tie_label():
    lab = np.zeros((24, 40), np.int32)
    lab[1:4, 1:5] = 2               # 12
    lab[6:11, 2:8] = 3              # 30
    lab[1:3, 10:16] = 5             # 12
    lab[12:18, 12:17] = 7           # 30
    lab[20:22, 30:33] = 9           # 6
    lab[4:8, 20:22] = 12            # 8 + the 4 below, in two separate pieces: 12
    lab[18:20, 36:38] = 12
    return lab


def points():
    rs = np.random.RandomState(3)
    a = (rs.rand(13, 2) * 40).astype(np.float32)
    b = a[:12] + (rs.rand(12, 2).astype(np.float32) - 0.5) * 2
    b[3] += 9
    b[8] -= 7
    b[10, 0] += 3.5
    return a, b[::-1].copy()


def main():
    _ref_shims.install()
    import stats_utils
    out = {}
    z, pp = np.load(os.path.join(HERE, 'aji.npz')), np.load(os.path.join(HERE, 'postproc.npz'))
    for name in z['names']:
        name = str(name)
        pred, true = pp['final_' + name].astype(np.int32), z['true_' + name]
        p, t = stats_utils.remap_label(pred.copy()), stats_utils.remap_label(true.copy())
        out['ajip_' + name] = np.float64(stats_utils.get_fast_aji_plus(t, p))
        out['dice2f_' + name] = np.float64(stats_utils.get_fast_dice_2(t, p))
        out['dice2_' + name] = np.float64(stats_utils.get_dice_2(t, p))
        out['bysize_' + name] = np.asarray(stats_utils.remap_label(pred.copy(), by_size=True), dtype=np.int32)
        print('%-10s %s instances true %d pred %d aji+ %.6f dice2 %.6f / %.6f' % (name, pred.shape, t.max(), p.max(), out['ajip_' + name],
                                                                                 out['dice2f_' + name], out['dice2_' + name]))
    m = np.load(os.path.join(HERE, 'aji_many.npz'))
    t, p = m['true'], m['pred']
    out['ajip_many'] = np.float64(stats_utils.get_fast_aji_plus(t, p))
    out['dice2f_many'] = np.float64(stats_utils.get_fast_dice_2(t, p))
    out['bysize_many'] = np.asarray(stats_utils.remap_label(p.copy(), by_size=True), dtype=np.int32)
    print('many       aji+ %.6f dice2 %.6f' % (out['ajip_many'], out['dice2f_many']))
    lab = tie_label()
    out['tie_label'] = lab
    out['tie_bysize'] = np.asarray(stats_utils.remap_label(lab.copy(), by_size=True), dtype=np.int32)
    order = [int(out['tie_bysize'][lab == i][0]) for i in (3, 7, 2, 5, 12, 9)]
    assert order == [1, 2, 3, 4, 5, 6], order
    a, b = points()
    pairing, ua, ub = stats_utils.pair_coordinates(a, b, 3.0)
    assert len(ua) > 1 and len(ub) > 0 and len(pairing) > 6
    out['pc_a'], out['pc_b'], out['pc_radius'] = a, b, np.float64(3.0)
    out['pc_pairing'], out['pc_unpaired_a'], out['pc_unpaired_b'] = np.asarray(pairing, dtype=np.int64), ua, ub
    print('pair_coordinates: %d paired, unpaired A %s B %s' % (len(pairing), ua.tolist(), ub.tolist()))
    out['names'] = z['names']
    path = os.path.join(HERE, 'objmetrics.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
