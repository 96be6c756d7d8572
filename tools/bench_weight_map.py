"""Cost of one border weight map (cdnet_amd/data_prepare/weight_maps.py) on the device against the numpy / scipy path, one process.

    python tools/bench_weight_map.py [--reps 20] [--warmup 3] [--host-reps 3] [--no-box]

Input: synth.ellipse_instances(1000, 1000, 3000, rmin=8, rmax=16) (seed 0), the instance map of tools/bench_metrics.py.

1. The cdnet_weight_map launch alone on the resident map (device events): --warmup launches, then --reps; the median.
2. weight_map(numpy array) as a caller sees it: upload, launch, download (host clock, ends in the device-to-host copy).
3. weight_map_host, --host-reps times (host clock): one scipy EDT per instance on its bounding box grown by R.
The bytes of 1 and 3 must be equal.  The JSON line printed at the end quotes the device and (unless --no-box) bench.py's box_calibration."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def instance_map():
    from cdnet_amd import synth
    return synth.ellipse_instances(1000, 1000, 3000, np.random.RandomState(0), rmin=8, rmax=16)


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


def wall(f, reps, warmup):
    for _ in range(warmup):
        f()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = f()
        out.append(time.perf_counter() - t0)
    return out, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--w0', type=float, default=10.0)
    ap.add_argument('--sigma', type=float, default=5.0)
    ap.add_argument('--no-box', action='store_true')
    a = ap.parse_args()
    from cdnet_amd import _lib
    from cdnet_amd.data_prepare import weight_maps
    dev = torch.device('cuda:0')
    line = {'tool': 'bench_weight_map', 'device': torch.cuda.get_device_name(0), 'w0': a.w0, 'sigma': a.sigma, 'radius': weight_maps.radius(a.w0, a.sigma)}
    if not a.no_box:
        from bench import box_calibration
        line['box'] = box_calibration(torch, dev)

    L = instance_map()
    H, W = L.shape
    line['image'] = {'H': H, 'W': W, 'instances': int(len(np.unique(L)) - 1), 'background_share': round(float((L == 0).mean()), 3)}
    lab = torch.from_numpy(L).to(dev)
    out = torch.empty((H, W), dtype=torch.uint8, device=dev)
    launch = lambda: _lib.call('cdnet_weight_map', _lib.ptr(lab), H, W, a.w0, a.sigma, _lib.ptr(out), _lib.stream_ptr())
    ms = events(launch, a.reps, a.warmup)
    got = out.cpu().numpy()
    line['launch'] = {'ms_median': round(statistics.median(ms), 4), 'ms_min': round(min(ms), 4), 'ms_max': round(max(ms), 4), 'reps': a.reps}
    print('cdnet_weight_map, %d x %d, %d instances: %.4f ms median (%.4f .. %.4f)' % (H, W, line['image']['instances'], statistics.median(ms),
                                                                                   min(ms), max(ms)), flush=True)
    ts, whole = wall(lambda: weight_maps.weight_map(L, a.w0, a.sigma, device=dev), a.reps, a.warmup)
    line['call'] = {'ms_median': round(statistics.median(ts) * 1e3, 3), 'ms_min': round(min(ts) * 1e3, 3), 'ms_max': round(max(ts) * 1e3, 3)}
    print('weight_map() with upload and download: %.3f ms median' % (statistics.median(ts) * 1e3), flush=True)
    th, want = wall(lambda: weight_maps.weight_map_host(L, a.w0, a.sigma), a.host_reps, 0)
    equal = bool(np.array_equal(got, want) and np.array_equal(whole, want))
    line['host'] = {'s_median': round(statistics.median(th), 4), 's_min': round(min(th), 4), 's_max': round(max(th), 4), 'reps': a.host_reps}
    line['bytes_equal'], line['max_byte'] = equal, int(want.max())
    line['host_over_launch'] = round(statistics.median(th) * 1e3 / statistics.median(ms), 1)
    line['host_over_call'] = round(statistics.median(th) / statistics.median(ts), 1)
    print('weight_map_host: %.4f s median; bytes equal: %s (%d differ)' % (statistics.median(th), equal, int((got != want).sum())), flush=True)
    print(json.dumps(line))
    assert equal


if __name__ == '__main__':
    main()
