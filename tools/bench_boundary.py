"""Cost of the boundary / focal term (--boundary-loss 1|2|3; csrc/boundary.hip), one process, one box.

    python tools/bench_boundary.py [--batch 16] [--launches 40] [--steps 24] [--warmup 6] [--no-step] [--no-box]

1. cdnet_boundary_loss alone at B x 3 x 256 x 256 on the synthetic batch's labels (random logits x 3), kinds 1 and 2, value and gradient:
   --warmup calls, then --launches calls with a pair of device events around each; the median.  Beside it the algorithmic traffic - the logits
   read twice (kind 1: once per pass) or once (kind 2), dmask read and written once, the label once per pass - and the time that traffic
   alone would take at the box's measured copy rate (the `box` record of bench.py): the factor over it is compute and LDS time.
2. The fp32 training step of bench.py's workload (trainer.synthetic_batch, seed 2022, UNet2RevA1_vgg16) with boundary = 0 and boundary = 1:
   two trainers on equal models, their steps ALTERNATED (A B A B ...) with device events around each step, median of --steps steps each after
   --warmup; the ratio boundary=1 / boundary=0 of the medians.
One JSON line is printed at the end."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed_each(fns, n, warmup):
    """alternate the callables: per callable the list of its n device times in ms"""
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    evs = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)] for _ in fns]
    for i in range(n):
        for k, f in enumerate(fns):
            evs[k][i][0].record()
            f()
            evs[k][i][1].record()
    torch.cuda.synchronize()
    return [[e0.elapsed_time(e1) for e0, e1 in ev] for ev in evs]


def copy_rate(box):
    """bytes per second (read + write counted) of the box record's 1 GiB device copy"""
    return float(box['copy_GBs']) * 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--launches', type=int, default=40)
    ap.add_argument('--steps', type=int, default=24)
    ap.add_argument('--warmup', type=int, default=6)
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--no-box', action='store_true')
    a = ap.parse_args()
    import cdnet_amd
    from cdnet_amd import _lib, trainer
    from cdnet_amd.models.dam.model_unet_rev1 import Unet
    dev = torch.device('cuda:0')
    line = {'tool': 'bench_boundary', 'batch': a.batch}
    rate = None
    if not a.no_box:
        from bench import box_calibration
        line['box'] = box_calibration(torch, dev)
        rate = copy_rate(line['box'])
    B, K, H, W = a.batch, 3, 256, 256
    batch = trainer.synthetic_batch(B, dev, seed=2022)
    label = batch[1]
    torch.manual_seed(0)
    logits = torch.randn((B, K, H, W), device=dev) * 3
    dmask = torch.zeros_like(logits)
    out = torch.zeros((1,), device=dev)
    for kind in (1, 2):
        need = _lib.load().cdnet_boundary_loss_workspace_bytes(kind, B, K, H, W)
        ws = torch.empty(((need + 3) // 4,), dtype=torch.float32, device=dev)

        def kernel():
            _lib.call('cdnet_boundary_loss', _lib.ptr(logits), _lib.ptr(label), kind, B, K, H, W, 1.0, _lib.ptr(ws), need, _lib.ptr(out), None,
                      _lib.ptr(dmask), _lib.stream_ptr())
        ms = timed_each([kernel], a.launches, a.warmup)[0]
        us = statistics.median(ms) * 1e3
        passes = 2 if kind == 1 else 1
        traffic = B * (passes * K * H * W * 4 + 2 * K * H * W * 4 + passes * H * W)
        rec = {'us_median': round(us, 1), 'us_min': round(min(ms) * 1e3, 1), 'us_max': round(max(ms) * 1e3, 1), 'launches': a.launches,
               'algorithmic_MB': round(traffic / 1e6, 1), 'GBps': round(traffic / us * 1e-3, 1), 'workspace_KB': round(need / 1e3, 1),
               'loss': float(out[0])}
        if rate:
            rec['us_traffic_at_copy_rate'] = round(traffic / rate * 1e6, 1)
            rec['factor_over_traffic'] = round(us / (traffic / rate * 1e6), 2)
        line['kind%d' % kind] = rec
        print('cdnet_boundary_loss kind %d B=%d: %.1f us median (%.1f .. %.1f), %.1f MB algorithmic, %.1f GB/s%s' %
              (kind, B, us, min(ms) * 1e3, max(ms) * 1e3, traffic / 1e6, traffic / us * 1e-3,
               ', %.2f x its traffic at the copy rate' % rec['factor_over_traffic'] if rate else ''), flush=True)
    if not a.no_step:
        before = cdnet_amd.get_precision()
        cdnet_amd.set_precision('fp32')
        trs = []
        for boundary in (0, 1):
            torch.manual_seed(2022)
            tr = trainer.Trainer(Unet(backbone_name='vgg16_bn', pretrained=False, classes=3).to(dev))
            tr.boundary = boundary
            trs.append(tr)
        t0, t1 = timed_each([lambda tr=tr: tr.train_step(*batch) for tr in trs], a.steps, a.warmup)
        m0, m1 = statistics.median(t0), statistics.median(t1)
        line['step_fp32'] = {'ms_boundary0': round(m0, 3), 'ms_boundary1': round(m1, 3), 'ratio': round(m1 / m0, 4), 'steps': a.steps,
                             'spread_boundary0': [round(min(t0), 3), round(max(t0), 3)],
                             'spread_boundary1': [round(min(t1), 3), round(max(t1), 3)], 'loss_boundary': float(trs[1].loss_boundary[0])}
        print('fp32 step: boundary=0 %.3f ms, boundary=1 %.3f ms, ratio %.4f' % (m0, m1, m1 / m0), flush=True)
        del trs
        torch.cuda.empty_cache()
        cdnet_amd.set_precision(before)
    print(json.dumps(line))


if __name__ == '__main__':
    main()
