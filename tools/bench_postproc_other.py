"""Cost of postproc_other's per-instance re-dilation (cdnet_amd/postproc_other.py, csrc/instance_fill.hip) on the device against the
numpy / scipy path, one process.

    python tools/bench_postproc_other.py [--reps 20] [--warmup 3] [--host-reps 3] [--literal-ids 32] [--no-box]

Input: synth.ellipse_instances(1000, 1000, 3000, rmin=8, rmax=16) (seed 0), the instance map of tools/bench_metrics.py and
tools/bench_weight_map.py.

1. The cdnet_instance_redilate call alone on the resident map (device events), r = 1 and r = 3, cap = the largest id: --warmup calls, then
   --reps; the median.
2. process(numpy array, 'micronet') on the map's foreground as a caller sees it: upload, fill holes / label / remove small, the re-dilation,
   download (host clock, ends in the device-to-host copy).
3. The host path (host clock): the reference's literal loop (redilate_host: a whole-image dilation and fill per instance) on the first
   --literal-ids ids only - the whole map would take most of a minute - and the same loop restricted to every instance's bounding box grown
   by r, on the whole map, --host-reps times.
The outputs must be equal: 1 and the bounding-box form on the whole map, the literal form, the bounding-box form and the device on the map of
the --literal-ids ids alone, and 2 against scipy's fill / label followed by the bounding-box form.  The JSON line printed at the end quotes
the device and (unless --no-box) bench.py's box_calibration."""
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


def redilate_host_boxed(lab, r):
    """redilate_host with every instance confined to its bounding box grown by r (clipped): the same result, without the whole-image work"""
    from scipy import ndimage as ndi
    diamond = ndi.iterate_structure(ndi.generate_binary_structure(2, 1), r)
    H, W = lab.shape
    canvas = np.zeros(lab.shape, np.int32)
    for k, box in enumerate(ndi.find_objects(lab), start=1):
        if box is None:
            continue
        win = (slice(max(box[0].start - r, 0), min(box[0].stop + r, H)), slice(max(box[1].start - r, 0), min(box[1].stop + r, W)))
        inst = ndi.binary_fill_holes(ndi.binary_dilation(lab[win] == k, structure=diamond))
        canvas[win][inst] = k
    return canvas


def stats(xs, scale, digits):
    return {'median': round(statistics.median(xs) * scale, digits), 'min': round(min(xs) * scale, digits), 'max': round(max(xs) * scale, digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--literal-ids', type=int, default=32)
    ap.add_argument('--no-box', action='store_true')
    a = ap.parse_args()
    from scipy import ndimage as ndi
    from cdnet_amd import _lib, postproc_other
    dev = torch.device('cuda:0')
    line = {'tool': 'bench_postproc_other', 'device': torch.cuda.get_device_name(0), 'lds_window': list(postproc_other.redilate_limits())}
    if not a.no_box:
        from bench import box_calibration
        line['box'] = box_calibration(torch, dev)

    L = np.ascontiguousarray(instance_map(), np.int32)
    H, W = L.shape
    ids = np.unique(L[L > 0])
    cap = int(ids.max())
    line['image'] = {'H': H, 'W': W, 'instances': int(len(ids)), 'largest_id': cap, 'background_share': round(float((L == 0).mean()), 3)}
    lib = _lib.load()
    lab = torch.from_numpy(L).to(dev)
    out = torch.empty_like(lab)
    err = torch.empty((1,), dtype=torch.int32, device=dev)
    ws = torch.empty((lib.cdnet_instance_redilate_workspace_bytes(1, H, W, cap),), dtype=torch.uint8, device=dev)
    equal = True
    got = {}
    for r in (1, 3):
        call = lambda: _lib.call('cdnet_instance_redilate', _lib.ptr(lab), 1, H, W, r, cap, _lib.ptr(ws), ws.numel(), _lib.ptr(out), _lib.ptr(err),
                                 _lib.stream_ptr())
        ms = events(call, a.reps, a.warmup)
        assert int(err.item()) == 0
        got[r] = out.cpu().numpy()
        line['redilate_r%d_ms' % r] = dict(stats(ms, 1.0, 4), reps=a.reps)
        print('cdnet_instance_redilate r = %d, %d x %d, %d instances: %.4f ms median (%.4f .. %.4f)' % (r, H, W, len(ids), statistics.median(ms),
                                                                                                      min(ms), max(ms)), flush=True)
        th, want = wall(lambda: redilate_host_boxed(L, r), a.host_reps, 0)
        line['host_boxed_r%d_s' % r] = dict(stats(th, 1.0, 4), reps=a.host_reps)
        line['host_boxed_over_redilate_r%d' % r] = round(statistics.median(th) * 1e3 / statistics.median(ms), 1)
        same = bool(np.array_equal(got[r], want))
        equal &= same
        print('bounding-box host form r = %d: %.4f s median; equal: %s' % (r, statistics.median(th), same), flush=True)
        # the literal loop on the first ids only
        sub_ids = ids[:a.literal_ids]
        lit = np.where(np.isin(L, sub_ids), L, 0).astype(np.int32)
        top = int(sub_ids.max())
        tl, want_lit = wall(lambda: postproc_other.redilate_host(lit, r), 1, 0)
        n_loop = top                                                       # the literal loop visits every id up to the largest, present or not
        dev_lit = postproc_other.redilate_instances(torch.from_numpy(lit).to(dev), r).cpu().numpy()
        same = bool(np.array_equal(want_lit, redilate_host_boxed(lit, r)) and np.array_equal(want_lit, dev_lit))
        equal &= same
        line['host_literal_r%d' % r] = {'ids_present': int(len(sub_ids)), 'ids_visited': n_loop, 's': round(tl[0], 3),
                                        'ms_per_visited_id': round(tl[0] * 1e3 / max(n_loop, 1), 2),
                                        's_whole_map_extrapolated': round(tl[0] / max(n_loop, 1) * cap, 1)}
        print('literal host loop r = %d on %d ids (%d visited): %.3f s = %.2f ms per id; equal: %s' % (r, len(sub_ids), n_loop, tl[0],
                                                                                                   tl[0] * 1e3 / max(n_loop, 1), same), flush=True)

    pred = (L > 0).astype(np.float32)
    ts, whole = wall(lambda: postproc_other.process(pred, 'micronet'), a.reps, a.warmup)
    line['process_micronet_ms'] = stats(ts, 1e3, 3)
    print("process(numpy, 'micronet') with upload and download: %.3f ms median" % (statistics.median(ts) * 1e3), flush=True)
    t0 = time.perf_counter()
    labelled = ndi.label(ndi.binary_fill_holes(pred > 0.5))[0].astype(np.int32)
    labelled = postproc_other._remove_small_host(labelled, 10)
    want = redilate_host_boxed(labelled, 1)
    line['process_micronet_host_boxed_s'] = round(time.perf_counter() - t0, 4)
    same = bool(np.array_equal(whole, want))
    equal &= same
    line['process_micronet_components'] = int(len(np.unique(labelled)) - 1)
    print("scipy fill / label / remove small + bounding-box form: %.4f s; equal: %s" % (line['process_micronet_host_boxed_s'], same), flush=True)
    line['outputs_equal'] = equal
    print(json.dumps(line))
    assert equal


if __name__ == '__main__':
    main()
