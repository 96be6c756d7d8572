"""Cost of object-level scoring (utils.nuclei_accuracy_object_level) with the Hausdorff distances on the device (csrc/metrics.hip), one process.

    python tools/bench_metrics.py [--reps 5] [--warmup 2] [--host-reps 1] [--rate-side 1024] [--launches 5] [--no-box]

Input: synth.ellipse_instances(1000, 1000, 3000, rmin=8, rmax=16) as the ground truth (seed 0) and, as the prediction, the same image shifted by
(2, 3) with every 7th object removed.

1. Wall time of utils.nuclei_accuracy_object_level (host clock; the call ends in device-to-host copies): --warmup calls, then --reps; the
   median.  Beside it utils.nuclei_accuracy_object_level_host --host-reps times: the same function with one scipy directed_hausdorff call pair per
   matched object, which is what this function did before the device path existed.  The two 7-tuples must be equal.
2. The Hausdorff launches alone on the matched pairs of that image (device events): the two cdnet_label_csr calls and cdnet_hausdorff_pairs.
3. The pair kernel's rate: two complementary chequerboards of --rate-side squared pixels, one id each (every pixel a boundary pixel, no pixel of
   one inside the other, so the evaluations are exactly 2 * n * n for n = side * side / 2), timed with device events; evaluations per second.
   stats_utils.HAUSDORFF_MAX_WORK is sized from this number.
The JSON line printed at the end quotes the device and (unless --no-box) bench.py's box_calibration."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def image_pair():
    from cdnet_amd import synth
    true = synth.ellipse_instances(1000, 1000, 3000, np.random.RandomState(0), rmin=8, rmax=16)
    pred = np.roll(np.roll(true, 2, axis=0), 3, axis=1)
    lut = np.arange(int(true.max()) + 1, dtype=np.int32)
    lut[7::7] = 0
    return true, lut[pred]


def wall(f, reps, warmup):
    for _ in range(warmup):
        f()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out, r


def events(f, reps, warmup):
    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in ev:
        e0.record()
        f()
        e1.record()
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) for e0, e1 in ev]


def pair_launch(t, p, pairs):
    """(callable that runs the two list builds, callable that runs the pair kernel on them, d2 tensor, estimated work)"""
    from cdnet_amd import _lib, stats_utils
    cap = max(int(max(t.max().item(), p.max().item())) + 1, 2)
    H, W = t.shape
    state = {}

    def lists():
        state['t'], state['p'] = stats_utils.label_csr(t, cap), stats_utils.label_csr(p, cap)
    lists()
    ht, hp = state['t'][0].cpu().numpy(), state['p'][0].cpu().numpy()
    tile, _ = stats_utils.hausdorff_limits()
    items = torch.from_numpy(stats_utils.hausdorff_items(ht, hp, pairs, np.ones(len(pairs), bool), tile)).to(t.device)
    dpairs = torch.from_numpy(pairs.astype(np.int32)).to(t.device)
    d2 = torch.empty((len(pairs), 2), dtype=torch.int32, device=t.device)
    err = torch.empty((1,), dtype=torch.int32, device=t.device)

    def kernel():
        (tt, tpix, tb), (pt, ppix, pb) = state['t'], state['p']
        _lib.call('cdnet_hausdorff_pairs', _lib.ptr(t), _lib.ptr(tt), _lib.ptr(tpix), _lib.ptr(tb), _lib.ptr(p), _lib.ptr(pt), _lib.ptr(ppix),
                  _lib.ptr(pb), H, W, cap, _lib.ptr(dpairs), len(pairs), _lib.ptr(items), len(items), _lib.ptr(d2), _lib.ptr(err), _lib.stream_ptr())
    return lists, kernel, d2, err, int(stats_utils.hausdorff_work(ht, hp, pairs).sum()), len(items)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--host-reps', type=int, default=1)
    ap.add_argument('--rate-side', type=int, default=1024)
    ap.add_argument('--launches', type=int, default=5)
    ap.add_argument('--no-box', action='store_true')
    a = ap.parse_args()
    from cdnet_amd import stats_utils, utils
    dev = torch.device('cuda:0')
    line = {'tool': 'bench_metrics', 'device': torch.cuda.get_device_name(0), 'max_work_default': stats_utils.HAUSDORFF_MAX_WORK}
    if not a.no_box:
        from bench import box_calibration
        line['box'] = box_calibration(torch, dev)

    true, pred = image_pair()
    ts, got = wall(lambda: utils.nuclei_accuracy_object_level(pred, true), a.reps, a.warmup)
    line['object_level_device'] = {'s_median': round(statistics.median(ts), 4), 's_min': round(min(ts), 4), 's_max': round(max(ts), 4), 'reps': a.reps,
                                   'objects_true': int(true.max()), 'values': [float(v) for v in got]}
    print('nuclei_accuracy_object_level, Hausdorff on the device: %.4f s median (%.4f .. %.4f)' % (statistics.median(ts), min(ts), max(ts)), flush=True)
    if a.host_reps > 0:
        th, want = wall(lambda: utils.nuclei_accuracy_object_level_host(pred, true), a.host_reps, 0)
        equal = [float(v) for v in got] == [float(v) for v in want]
        line['object_level_host_helper'] = {'s_median': round(statistics.median(th), 4), 'reps': a.host_reps, 'equal_to_device': equal,
                                            'note': 'the retained scipy loop: what nuclei_accuracy_object_level did before the device path'}
        print('nuclei_accuracy_object_level_host (the scipy loop this function ran before the device path): %.4f s; results equal: %s' %
              (statistics.median(th), equal), flush=True)
        assert equal

    # the matched pairs of this image, as nuclei_accuracy_object_level collects them
    seen = {}
    utils.nuclei_accuracy_object_level(pred, true, hausdorff=lambda g, p, m: seen.update(g=g, p=p, m=m) or np.zeros(len(m)))
    t, p = torch.from_numpy(seen['g']).to(dev), torch.from_numpy(seen['p']).to(dev)
    lists, kernel, d2, err, work, n_items = pair_launch(t, p, seen['m'])
    ml, mk = events(lists, a.launches, 2), events(kernel, a.launches, 2)
    assert int(err.item()) == 0
    line['hausdorff_launches'] = {'pairs': len(seen['m']), 'blocks': n_items, 'lists_us_median': round(statistics.median(ml) * 1e3, 1),
                                  'pair_kernel_us_median': round(statistics.median(mk) * 1e3, 1), 'estimated_evaluations': work}
    print('Hausdorff launches alone, %d pairs: lists %.1f us, pair kernel %.1f us (%d blocks, estimate %.3g evaluations)' %
          (len(seen['m']), statistics.median(ml) * 1e3, statistics.median(mk) * 1e3, n_items, work), flush=True)

    s = a.rate_side
    yy, xx = np.mgrid[:s, :s]
    ct = torch.from_numpy(((yy + xx) % 2 == 0).astype(np.int32)).to(dev)
    cp = torch.from_numpy(((yy + xx) % 2 == 1).astype(np.int32)).to(dev)
    n = s * s // 2
    _, kernel, d2, err, work, n_items = pair_launch(ct, cp, np.array([[1, 1]], np.int64))
    assert work == 2 * n * n
    mk = events(kernel, 3, 1)
    assert int(err.item()) == 0 and d2.cpu().tolist() == [[1, 1]]
    rate = work / (statistics.median(mk) * 1e-3)
    line['pair_kernel_rate'] = {'side': s, 'evaluations': work, 'blocks': n_items, 'ms_median': round(statistics.median(mk), 2), 'ms_min': round(min(mk), 2),
                                'ms_max': round(max(mk), 2), 'evaluations_per_s': float('%.4g' % rate)}
    print('pair kernel, two %d x %d chequerboards: %.3g evaluations in %.2f ms: %.4g evaluations / s' % (s, s, work, statistics.median(mk), rate), flush=True)
    print(json.dumps(line))


if __name__ == '__main__':
    main()
