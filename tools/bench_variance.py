"""Cost of the instance variance term (--alpha 1; csrc/variance.hip), one process, one box.

    python tools/bench_variance.py [--batch 16] [--launches 40] [--steps 24] [--warmup 6] [--no-step] [--no-box]

1. cdnet_variance_loss alone at B x 3 x 256 x 256 on the synthetic batch's labels (random logits x 3): --warmup calls, then --launches calls with
   a pair of device events around each; the median.  Beside it the algorithmic traffic (3 reads of the logits, one read-modify-write of dmask,
   the label three times, three passes over the forest, the accumulators' memset) over that time.
2. The training step of bench.py's workload (trainer.synthetic_batch, seed 2022, UNet2RevA1_vgg16) in fp32 and in bf16 with alpha = 0 and
   alpha = 1: two trainers on equal models, their steps ALTERNATED (A B A B ...) with device events around each step, median of --steps steps
   each after --warmup; the ratio alpha=1 / alpha=0 of the medians.
The `box` record (bench.py's box_calibration: what this GPU grants) is quoted in the JSON line printed at the end."""
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
    line = {'tool': 'bench_variance', 'batch': a.batch}
    if not a.no_box:
        from bench import box_calibration
        line['box'] = box_calibration(torch, dev)
    B, K, H, W = a.batch, 3, 256, 256
    batch = trainer.synthetic_batch(B, dev, seed=2022)
    label = batch[1]
    torch.manual_seed(0)
    logits = torch.randn((B, K, H, W), device=dev) * 3
    dmask = torch.zeros_like(logits)
    out = torch.zeros((1,), device=dev)
    counts = torch.zeros((B,), dtype=torch.int32, device=dev)
    need = _lib.load().cdnet_variance_loss_workspace_bytes(B, K, H, W)
    ws = torch.empty(((need + 3) // 4,), dtype=torch.float32, device=dev)

    def kernel():
        _lib.call('cdnet_variance_loss', _lib.ptr(logits), _lib.ptr(label), 1, B, K, H, W, 1.0, _lib.ptr(ws), need, _lib.ptr(out), None,
                  _lib.ptr(dmask), None, _lib.ptr(counts), _lib.stream_ptr())
    ms = timed_each([kernel], a.launches, a.warmup)[0]
    us = statistics.median(ms) * 1e3
    slots = ((H + 1) // 2) * ((W + 1) // 2)
    traffic = B * (3 * K * H * W * 4 + 2 * K * H * W * 4 + 3 * H * W + 3 * 2 * H * W * 4 + slots * 32)
    line['kernel'] = {'us_median': round(us, 1), 'us_min': round(min(ms) * 1e3, 1), 'us_max': round(max(ms) * 1e3, 1), 'launches': a.launches,
                      'algorithmic_MB': round(traffic / 1e6, 1), 'GBps': round(traffic / us * 1e-3, 1), 'workspace_MB': round(need / 1e6, 1),
                      'instances': counts.cpu().tolist(), 'loss_var': float(out[0])}
    print('cdnet_variance_loss B=%d: %.1f us median (%.1f .. %.1f), %.1f MB algorithmic, %.1f GB/s' %
          (B, us, min(ms) * 1e3, max(ms) * 1e3, traffic / 1e6, traffic / us * 1e-3), flush=True)
    if not a.no_step:
        before = cdnet_amd.get_precision()
        for precision in ('fp32', 'bf16'):
            cdnet_amd.set_precision(precision)
            trs = []
            for alpha in (0.0, 1.0):
                torch.manual_seed(2022)
                tr = trainer.Trainer(Unet(backbone_name='vgg16_bn', pretrained=False, classes=3).to(dev))
                tr.alpha = alpha
                trs.append(tr)
            t0, t1 = timed_each([lambda tr=tr: tr.train_step(*batch) for tr in trs], a.steps, a.warmup)
            m0, m1 = statistics.median(t0), statistics.median(t1)
            line['step_' + precision] = {'ms_alpha0': round(m0, 3), 'ms_alpha1': round(m1, 3), 'ratio': round(m1 / m0, 4), 'steps': a.steps,
                                         'spread_alpha0': [round(min(t0), 3), round(max(t0), 3)],
                                         'spread_alpha1': [round(min(t1), 3), round(max(t1), 3)], 'loss_var': float(trs[1].loss_var[0])}
            print('%s step: alpha=0 %.3f ms, alpha=1 %.3f ms, ratio %.4f' % (precision, m0, m1, m1 / m0), flush=True)
            del trs
            torch.cuda.empty_cache()
        cdnet_amd.set_precision(before)
    print(json.dumps(line))


if __name__ == '__main__':
    main()
