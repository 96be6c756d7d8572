"""Instance metrics of the reference's stats_utils.py on the GPU: get_fast_aji (:7-106), get_fast_aji_plus (:108-178),
get_fast_pq (:182-276), get_fast_dice_2 (:279-317), get_dice_1 (:323-335), get_dice_2 (:338-357), remap_label (:361-392),
pair_coordinates (:393-439, host only), and `object_hausdorff`: the exact Hausdorff distances of many object pairs in one launch.

Same names, arguments and return values; `true` / `pred` are numpy HW integer label images (what the reference passes)
or torch CUDA int32 tensors.  The pass over the pixels (per-label areas, sparse pairwise intersections) runs in
csrc/metrics.hip; the per-pair arithmetic is done here in float64 with the reference's formulas, so results agree with
the reference to the last bits (tests/golden/aji.npz, objmetrics.npz).  No CPU fallback: the device pass is required (the one host
path is object_hausdorff's: pairs whose estimated work exceeds max_work are scored by the scipy loop instead of a seconds-long kernel).
The arithmetic after the pixel pass - aji_plus_from_table, dice2_from_table, size_order - takes (area_true, area_pred, pairs) and
needs no GPU."""
import numpy as np
import torch

from . import _lib


def _dev(a):
    if torch.is_tensor(a):
        assert a.is_cuda
        return a.to(torch.int32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def _check(err, who):
    e = int(err.item())
    if e == 1:
        raise ValueError('%s: instance id outside [0, capacity)' % who)
    if e == 2:
        raise RuntimeError('%s: pair table full' % who)


def size_order(area):
    """lookup table old id -> new id of remap_label(by_size=True) from the per-id areas (index = id; entry 0, the background, is
    ignored): present ids are numbered 1..K by area, largest first, equal areas in id order - what Python's stable
    sorted(zip(ids, sizes), key=size, reverse=True) gives the reference (:376-384).  Absent ids map to 0."""
    area = np.asarray(area, dtype=np.int64)
    ids = np.flatnonzero(area[1:] > 0) + 1
    lut = np.zeros(len(area), np.int32)
    lut[ids[np.argsort(-area[ids], kind='stable')]] = np.arange(1, len(ids) + 1, dtype=np.int32)
    return lut


def remap_label(pred, by_size=False):
    """ids -> 1..K in increasing id order, or (by_size=True) by decreasing area with equal areas in id order.  An image without
    labels is returned as it is."""
    is_np = not torch.is_tensor(pred)
    d = _dev(pred)
    cap = int(d.max().item()) + 1 if d.numel() else 1
    if cap <= 1:
        return pred
    scratch = torch.empty((cap,), dtype=torch.int32, device=d.device)
    out = torch.empty_like(d)
    err = torch.empty((1,), dtype=torch.int32, device=d.device)
    if by_size:
        _lib.call('cdnet_label_areas', _lib.ptr(d), 1, d.numel(), cap, _lib.ptr(scratch), _lib.ptr(err), _lib.stream_ptr())
        _check(err, 'remap_label')
        lut = torch.from_numpy(size_order(scratch.cpu().numpy())).to(d.device)
        _lib.call('cdnet_label_apply', _lib.ptr(d), 1, d.numel(), cap, _lib.ptr(lut), _lib.ptr(out), _lib.stream_ptr())
    else:
        _lib.call('cdnet_remap_label', _lib.ptr(d), 1, d.numel(), cap, _lib.ptr(scratch), _lib.ptr(out), _lib.ptr(err), _lib.stream_ptr())
        _check(err, 'remap_label')
    return out.cpu().numpy() if is_np else out


def pair_table(true, pred):
    """(area_true [T+1], area_pred [P+1], pairs: int64 array [K,3] of (true_id, pred_id, intersection) sorted by ids)"""
    t, p = _dev(true), _dev(pred)
    assert t.shape == p.shape
    cap = int(max(t.max().item(), p.max().item())) + 1
    cap = max(cap, 2)
    if cap > 65536:
        raise ValueError('more than 65535 instances: remap_label first')
    slots = 1 << 12
    while slots < 8 * cap:
        slots <<= 1
    while True:
        at = torch.empty((cap,), dtype=torch.int32, device=t.device)
        ap = torch.empty((cap,), dtype=torch.int32, device=t.device)
        hk = torch.empty((slots,), dtype=torch.int32, device=t.device)
        hc = torch.empty((slots,), dtype=torch.int32, device=t.device)
        err = torch.empty((1,), dtype=torch.int32, device=t.device)
        _lib.call('cdnet_label_pair_histogram', _lib.ptr(t), _lib.ptr(p), 1, t.numel(), cap, slots, _lib.ptr(at), _lib.ptr(ap), _lib.ptr(hk),
                  _lib.ptr(hc), _lib.ptr(err), _lib.stream_ptr())
        if int(err.item()) == 2 and slots < (1 << 24):
            slots <<= 2
            continue
        _check(err, 'pair_table')
        break
    keys = hk.cpu().numpy().view(np.uint32)
    cnt = hc.cpu().numpy()
    nz = keys != 0
    keys, cnt = keys[nz].astype(np.int64), cnt[nz].astype(np.int64)
    order = np.argsort(keys, kind='stable')
    keys, cnt = keys[order], cnt[order]
    pairs = np.stack([keys >> 16, keys & 0xffff, cnt], 1) if keys.size else np.zeros((0, 3), np.int64)
    return at.cpu().numpy().astype(np.int64), ap.cpu().numpy().astype(np.int64), pairs


def get_dice_1(true, pred):
    """2 |T & P| / (|T| + |P|) on the binarised label images"""
    at, ap, pairs = pair_table(true, pred)
    return 2.0 * float(pairs[:, 2].sum()) / float(at.sum() + ap.sum())


def get_fast_aji(true, pred):
    """(aji, FP/fm, FN/fm, less/fm, more/fm) exactly as stats_utils.get_fast_aji returns them.  Ids must be contiguous
    (call remap_label first, as the reference requires)."""
    at, ap, pairs = pair_table(true, pred)
    T, P = len(at) - 1, len(ap) - 1
    true_ids = [i for i in range(1, T + 1) if at[i] > 0]
    pred_ids = [i for i in range(1, P + 1) if ap[i] > 0]
    assert true_ids == list(range(1, len(true_ids) + 1)) and pred_ids == list(range(1, len(pred_ids) + 1)), \
        'get_fast_aji needs contiguous instance ids (remap_label)'
    best = {}                                    # true id -> (iou, pred id, inter, union) with np.argmax's first-maximum rule
    for ti, pi, inter in pairs:
        inter = float(inter)
        union = float(at[ti] + ap[pi]) - inter
        iou = inter / (union + 1.0e-6)
        cur = best.get(int(ti))
        if cur is None or iou > cur[0]:
            best[int(ti)] = (iou, int(pi), inter, union)
    overall_inter = overall_union = overall_FP = overall_FN = 0.0
    paired_pred = set()
    for ti in sorted(best):
        iou, pi, inter, union = best[ti]
        if iou > 0.0:
            overall_inter += inter
            overall_union += union
            overall_FP += float(ap[pi]) - inter
            overall_FN += float(at[ti]) - inter
            paired_pred.add(pi)
    less_pred = more_pred = 0
    for ti in true_ids:
        if ti not in best or not best[ti][0] > 0.0:
            less_pred += int(at[ti])
            overall_union += int(at[ti])
    for pi in pred_ids:
        if pi not in paired_pred:
            more_pred += int(ap[pi])
            overall_union += int(ap[pi])
    with np.errstate(divide='ignore', invalid='ignore'):       # numpy float64 semantics as in the reference (nan / inf, no exception)
        f = np.float64
        aji_score = f(overall_inter) / f(overall_union)
        fm = f(overall_union) - f(overall_inter)
        return float(aji_score), float(f(overall_FP) / fm), float(f(overall_FN) / fm), float(f(less_pred) / fm), float(f(more_pred) / fm)


def get_fast_pq(true, pred, match_iou=0.5):
    """[dq, sq, pq], [paired_true, paired_pred, unpaired_true, unpaired_pred] (stats_utils.py:182-276)"""
    assert match_iou >= 0.0, "Cant' be negative"
    at, ap, pairs = pair_table(true, pred)
    true_ids = [i for i in range(1, len(at)) if at[i] > 0]
    pred_ids = [i for i in range(1, len(ap)) if ap[i] > 0]
    iou = {}
    for ti, pi, inter in pairs:
        inter = float(inter)
        total = float(at[ti] + ap[pi])
        iou[(int(ti), int(pi))] = inter / (total - inter)
    if match_iou >= 0.5:
        sel = sorted(k for k, v in iou.items() if v > match_iou)          # np.nonzero order: by true id, then pred id
        paired_true = [k[0] for k in sel]
        paired_pred = [k[1] for k in sel]
        paired_iou = np.array([iou[k] for k in sel], dtype=np.float64)
    else:
        from scipy.optimize import linear_sum_assignment
        m = np.zeros((len(true_ids), len(pred_ids)), np.float64)
        for (ti, pi), v in iou.items():
            m[ti - 1, pi - 1] = v
        r, c = linear_sum_assignment(-m)
        piou = m[r, c]
        paired_true = list(r[piou > match_iou] + 1)
        paired_pred = list(c[piou > match_iou] + 1)
        paired_iou = piou[piou > match_iou]
    unpaired_true = [i for i in true_ids if i not in paired_true]
    unpaired_pred = [i for i in pred_ids if i not in paired_pred]
    tp, fp, fn = len(paired_true), len(unpaired_pred), len(unpaired_true)
    dq = tp / (tp + 0.5 * fp + 0.5 * fn)
    sq = paired_iou.sum() / (tp + 1.0e-6)
    return [dq, sq, dq * sq], [paired_true, paired_pred, unpaired_true, unpaired_pred]


def _contiguous_ids(at, ap, who):
    T, P = int((at[1:] > 0).sum()), int((ap[1:] > 0).sum())
    assert (at[1:T + 1] > 0).all() and (ap[1:P + 1] > 0).all(), who + ' needs contiguous instance ids (remap_label)'
    return T, P


def aji_plus_from_table(at, ap, pairs):
    """get_fast_aji_plus (:108-178) from pair_table's output: the dense IoU matrix inter / (union + 1e-6) with zeros elsewhere,
    scipy's linear_sum_assignment on its negative (the same matrix, so ties resolve as in the reference), pairs of IoU 0 dropped,
    the areas of unpaired instances added to the union."""
    from scipy.optimize import linear_sum_assignment
    at, ap = np.asarray(at, dtype=np.int64), np.asarray(ap, dtype=np.int64)
    T, P = _contiguous_ids(at, ap, 'get_fast_aji_plus')
    inter = np.zeros((T, P), np.float64)
    union = np.zeros((T, P), np.float64)
    if len(pairs):
        ti, pi, it = pairs[:, 0], pairs[:, 1], pairs[:, 2]
        inter[ti - 1, pi - 1] = it
        union[ti - 1, pi - 1] = at[ti] + ap[pi] - it
    iou = inter / (union + 1.0e-6)
    r, c = linear_sum_assignment(-iou)
    keep = iou[r, c] > 0.0
    r, c = r[keep], c[keep]
    overall_inter, overall_union = inter[r, c].sum(), union[r, c].sum()
    overall_union += at[1:T + 1].sum() - at[r + 1].sum() + ap[1:P + 1].sum() - ap[c + 1].sum()      # (integers: exact in any order)
    with np.errstate(divide='ignore', invalid='ignore'):
        return float(np.float64(overall_inter) / np.float64(overall_union))


def dice2_from_table(at, ap, pairs):
    """get_fast_dice_2 (:279-317) and get_dice_2 (:338-357): 2 * sum of intersections / sum of (|t| + |p|) over the overlapping
    pairs; integer sums, one division (ZeroDivisionError without any overlap, as the reference's)."""
    at, ap = np.asarray(at, dtype=np.int64), np.asarray(ap, dtype=np.int64)
    inter = int(pairs[:, 2].sum()) if len(pairs) else 0
    total = int((at[pairs[:, 0]] + ap[pairs[:, 1]]).sum()) if len(pairs) else 0
    return 2 * inter / total


def get_fast_aji_plus(true, pred):
    """AJI+ (one-to-one pairing by maximal total IoU).  Ids must be contiguous (remap_label)."""
    return aji_plus_from_table(*pair_table(true, pred))


def get_fast_dice_2(true, pred):
    """ensemble Dice over the overlapping pairs"""
    return dice2_from_table(*pair_table(true, pred))


def get_dice_2(true, pred):
    """the reference's slower spelling of get_fast_dice_2: the same value"""
    return dice2_from_table(*pair_table(true, pred))


def pair_coordinates(setA, setB, radius):
    """(pairing [k, 2], unpairedA, unpairedB): the minimum-total-distance one-to-one pairing of the points of setA [n, 2] and
    setB [m, 2] (scipy's linear_sum_assignment on the Euclidean distance matrix, computed in the inputs' type), pairs further
    apart than `radius` dropped (:393-439).  Host only."""
    from scipy.optimize import linear_sum_assignment
    setA, setB = np.asarray(setA), np.asarray(setB)
    dist = np.sqrt(np.sum((setA[:, None, :] - setB[None, :, :]) ** 2, axis=-1))
    ia, ib = linear_sum_assignment(dist)
    near = dist[ia, ib] <= radius
    pairedA, pairedB = ia[near], ib[near]
    unpairedA = np.array([i for i in range(setA.shape[0]) if i not in set(pairedA.tolist())], dtype=np.int64)
    unpairedB = np.array([i for i in range(setB.shape[0]) if i not in set(pairedB.tolist())], dtype=np.int64)
    return np.array(list(zip(pairedA, pairedB))), unpairedA, unpairedB


# object_hausdorff: most distance evaluations one call puts on the device (the rest of the pairs are scored on the host).  The pair
# kernel measured 7.9e12 evaluations a second on an MI355X (tools/bench_metrics.py): about half a second of
# kernel time at the most when the launch fills the chip, and the estimate is an upper bound.
HAUSDORFF_MAX_WORK = 4 * 10 ** 12


def hausdorff_limits():
    """(pixels of the source object one block holds in registers, boundary pixels of the other object per LDS pass)"""
    lib = _lib.load()
    return int(lib.cdnet_hausdorff_tile_pixels()), int(lib.cdnet_hausdorff_chunk_pixels())


def label_csr(lab, cap):
    """device lists of one HW int32 label image: (tab [4, cap]: pixels per id, boundary pixels per id, segment starts in pix and in
    bpix; pix [H*W], bpix [H*W]: coordinates y << 16 | x grouped by id, all pixels / boundary pixels only)"""
    H, W = lab.shape
    tab = torch.empty((4, cap), dtype=torch.int32, device=lab.device)
    pix = torch.empty((H * W,), dtype=torch.int32, device=lab.device)
    bpix = torch.empty((H * W,), dtype=torch.int32, device=lab.device)
    nws = int(_lib.load().cdnet_label_csr_workspace_bytes(cap))
    ws = torch.empty((nws,), dtype=torch.uint8, device=lab.device)
    err = torch.empty((1,), dtype=torch.int32, device=lab.device)
    _lib.call('cdnet_label_csr', _lib.ptr(lab), H, W, cap, _lib.ptr(ws), nws, _lib.ptr(tab), _lib.ptr(pix), _lib.ptr(bpix), _lib.ptr(err),
              _lib.stream_ptr())
    _check(err, 'object_hausdorff')
    return tab, pix, bpix


def hausdorff_work(tab_true, tab_pred, pairs):
    """upper estimate of the distance evaluations of each pair, both directions: |P| * |boundary of T| + |T| * |boundary of P|
    (the kernel skips the pixels of one object that lie inside the other, which the areas alone do not tell).  int64 [M]"""
    tt, tp = np.asarray(tab_true, dtype=np.int64), np.asarray(tab_pred, dtype=np.int64)
    return tp[0][pairs[:, 1]] * tt[1][pairs[:, 0]] + tt[0][pairs[:, 0]] * tp[1][pairs[:, 1]]


def hausdorff_items(tab_true, tab_pred, pairs, on_device, tile):
    """the pair kernel's work list, int32 [n, 2] rows (2 * pair + direction, tile): one row per `tile` pixels of the direction's
    source object (0: the predicted one, 1: the true one) for every pair selected by the mask `on_device`"""
    sel = np.flatnonzero(on_device)
    n_src = np.stack([np.asarray(tab_pred)[0][pairs[sel, 1]], np.asarray(tab_true)[0][pairs[sel, 0]]], 1).astype(np.int64)     # [m, 2]
    tiles = (n_src + tile - 1) // tile
    slots = (2 * sel[:, None] + np.arange(2)[None, :]).ravel()
    tiles = tiles.ravel()
    first = np.cumsum(tiles) - tiles
    slot = np.repeat(slots, tiles)
    return np.stack([slot, np.arange(int(tiles.sum())) - np.repeat(first, tiles)], 1).astype(np.int32)


def object_hausdorff(true, pred, pairs, squared_directed=False, max_work=None):
    """Hausdorff distance max(h(P -> T), h(T -> P)) of every pair (true id, pred id) of `pairs` [M, 2], float64 [M], bit-equal to
    scipy's directed_hausdorff on np.argwhere of the two objects (what utils.nuclei_accuracy_object_level asks for); with
    squared_directed=True the exact squares (h(P -> T)^2, h(T -> P)^2) as int64 [M, 2].  true / pred: HW label images (numpy or
    CUDA int32), ids in [0, 65536), H and W at most 32767.  Pairs are arbitrary: objects may be disjoint, nested, identical, in
    several pieces, and an id may occur in several pairs.  An id without pixels in its image raises ValueError.
    All pairs run in one launch (csrc/metrics.hip).  max_work (default HAUSDORFF_MAX_WORK) bounds the distance evaluations of that
    launch as estimated by hausdorff_work: pairs are admitted cheapest first while the sum stays within it, the others are scored
    by utils.object_hausdorff_host (scipy)."""
    t, p = _dev(true), _dev(pred)
    if t.dim() != 2 or t.shape != p.shape:
        raise ValueError('object_hausdorff: two HW label images of one shape')
    H, W = t.shape
    if H > 32767 or W > 32767:
        raise ValueError('object_hausdorff: image sides above 32767')
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    M = len(pairs)
    if M == 0 or t.numel() == 0:
        if M:
            raise ValueError('object_hausdorff: id without pixels')
        return np.zeros((0, 2), np.int64) if squared_directed else np.zeros((0,), np.float64)
    cap = max(int(max(t.max().item(), p.max().item())) + 1, 2)
    if cap > 65536 or pairs.min() < 0 or pairs.max() >= 65536:
        raise ValueError('object_hausdorff: instance id outside [0, 65536)')
    tab_t, pix_t, bpix_t = label_csr(t, cap)
    tab_p, pix_p, bpix_p = label_csr(p, cap)
    ht, hp = tab_t.cpu().numpy(), tab_p.cpu().numpy()
    if pairs.max() >= cap or (ht[0][pairs[:, 0]] == 0).any() or (hp[0][pairs[:, 1]] == 0).any() or pairs.min() == 0:
        raise ValueError('object_hausdorff: a pair names an id without pixels in its image')
    work = hausdorff_work(ht, hp, pairs)
    order = np.argsort(work, kind='stable')
    on_device = np.zeros(M, bool)
    on_device[order[np.cumsum(work[order]) <= (HAUSDORFF_MAX_WORK if max_work is None else max_work)]] = True
    d2 = np.zeros((M, 2), np.int64)
    if on_device.any():
        tile, _ = hausdorff_limits()
        items = torch.from_numpy(hausdorff_items(ht, hp, pairs, on_device, tile)).to(t.device)
        dpairs = torch.from_numpy(pairs.astype(np.int32)).to(t.device)
        out = torch.empty((M, 2), dtype=torch.int32, device=t.device)
        err = torch.empty((1,), dtype=torch.int32, device=t.device)
        _lib.call('cdnet_hausdorff_pairs', _lib.ptr(t), _lib.ptr(tab_t), _lib.ptr(pix_t), _lib.ptr(bpix_t), _lib.ptr(p), _lib.ptr(tab_p),
                  _lib.ptr(pix_p), _lib.ptr(bpix_p), H, W, cap, _lib.ptr(dpairs), M, _lib.ptr(items), len(items), _lib.ptr(out), _lib.ptr(err),
                  _lib.stream_ptr())
        e = int(err.item())
        if e:
            raise RuntimeError('object_hausdorff: pair kernel refused its work list (%d)' % e)
        d2[on_device] = out.cpu().numpy()[on_device]
    if not on_device.all():
        from . import utils
        host = utils.object_hausdorff_host(t.cpu().numpy(), p.cpu().numpy(), pairs[~on_device])
        d2[~on_device] = np.rint(host * host).astype(np.int64)                 # sqrt of an integer below 2^31, squared: off by < 2^-20
    return d2 if squared_directed else np.sqrt(d2.max(1).astype(np.float64))
