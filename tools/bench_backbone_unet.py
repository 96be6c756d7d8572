"""Training step of the backbone U-Net `UNet_vgg16` beside `UNet2RevA1_vgg16`'s on the same box, one JSON line per record.

    python3 tools/bench_backbone_unet.py [--precision fp32|bf16] [--batch 16] [--size 256] [--steps 20] [--warmup 5]
                                         [--model UNet_vgg16|UNet2RevA1_vgg16|both] [--no-box]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o t -- python3 tools/bench_backbone_unet.py --model UNet_vgg16 --no-box
        per-kernel durations: final_conv1x1_c16_kernel, final_conv_c16_bwd_kernel and the two small kernels behind it (csrc/classifier16.hip)

Records: `box` (bench.box_calibration: what this GPU grants - copy rate, MFMA rate, clock), then for each model `train_step` with the mean
and the median step time over --steps steps after --warmup (events around every step, one synchronisation at the end), and `classifier16`:
the two library entries of the 16-channel classifier timed with events around each call over the same steps.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def say(**kw):
    print(json.dumps(kw), flush=True)


def build(name, dev):
    from cdnet_amd import utils

    class _Opt:
        model = {'modelName': name, 'out_c': 3, 'in_c': 3}
    torch.manual_seed(0)
    m = utils.chooseModel(_Opt()).to(dev)
    return m, utils.trainer_class(m)(m)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--precision', default='fp32', choices=['fp32', 'bf16'])
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--model', default='both', choices=['UNet_vgg16', 'UNet2RevA1_vgg16', 'both'])
    ap.add_argument('--no-box', action='store_true')
    a = ap.parse_args()
    import cdnet_amd
    from cdnet_amd import _lib, synth
    cdnet_amd.set_precision(a.precision)
    dev = torch.device('cuda:0')
    torch.cuda.set_device(0)
    if not a.no_box:
        import bench
        say(what='box', **bench.box_calibration(torch, dev))
    x, lab, dirn, point, weight = synth.synthetic_batch(a.batch, dev, seed=2022, H=a.size, W=a.size)
    for name in (['UNet_vgg16', 'UNet2RevA1_vgg16'] if a.model == 'both' else [a.model]):
        m, tr = build(name, dev)
        batch = (x, lab, weight) if name == 'UNet_vgg16' else (x, lab, dirn, point, weight)
        for _ in range(a.warmup):
            tr.train_step(*batch)
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
        calls, real = [], _lib.call

        def timed(entry, *args):
            if 'c16' not in entry:
                return real(entry, *args)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = real(entry, *args)
            e1.record()
            calls.append((entry, e0, e1))
            return r
        _lib.call = timed
        try:
            for e0, e1 in ev:
                e0.record()
                tr.train_step(*batch)
                e1.record()
            torch.cuda.synchronize()
        finally:
            _lib.call = real
        ms = np.array([e0.elapsed_time(e1) for e0, e1 in ev])
        say(what='train_step', model=name, precision=a.precision, batch=a.batch, size=a.size, steps=a.steps, ms_mean=round(float(ms.mean()), 4),
            ms_median=round(float(np.median(ms)), 4), tiles_per_s=round(a.batch / float(np.median(ms)) * 1e3, 1))
        for entry in sorted({c[0] for c in calls}):
            t = np.array([e0.elapsed_time(e1) for n, e0, e1 in calls if n == entry])
            say(what='classifier16', model=name, precision=a.precision, entry=entry, calls=len(t), ms_median=round(float(np.median(t)), 4),
                share_of_step=round(float(np.median(t)) / float(np.median(ms)), 5))
        del m, tr
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
