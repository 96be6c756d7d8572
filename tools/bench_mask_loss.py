"""The plain UNet's loss step: the earlier route against cdnet_mask_loss (csrc/mask_loss.hip), one process, one box.

    python tools/bench_mask_loss.py [--batch 16] [--launches 60] [--warmup 10] [--no-box]

At B x 3 x 256 x 256 (the plain UNet's own batch; labels of the synthetic batch, logits randn x 3, value and gradient):
  parent route   the four zero_() fills of the constant point / direction branches + cdnet_dam_loss_classes (9 classes) with the three
                 gradient outputs - what UNetTrainer.loss_and_grads did before; the library still contains the entry unchanged
  new route      cdnet_mask_loss(WMAP | CE | DICE) with dmask
--warmup rounds, then --launches rounds that ALTERNATE the two routes with a pair of device events around each; the medians and their ratio.
Expected from the kernels' loads and stores: 40 B against 211 B per pixel = 0.19; the bar is 0.5 (at one million pixels both routes are a
handful of 5-20 us launches, and launch gaps weigh as much as bytes).  One JSON line is printed at the end."""
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
    ap.add_argument('--launches', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--no-box', action='store_true')
    a = ap.parse_args()
    from cdnet_amd import _lib, trainer
    dev = torch.device('cuda:0')
    line = {'tool': 'bench_mask_loss', 'batch': a.batch}
    if not a.no_box:
        from bench import box_calibration
        line['box'] = box_calibration(torch, dev)
    B, H, W = a.batch, 256, 256
    P = H * W
    lib = _lib.load()
    batch = trainer.synthetic_batch(B, dev, seed=2022)
    label, weight = batch[1], batch[4]
    torch.manual_seed(0)
    logits = torch.randn((B, 3, H, W), device=dev) * 3
    z = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    point, dirn, dirlab, pt = z((B, 1, H, W), torch.float32), z((B, 9, H, W), torch.float32), z((B, H, W), torch.uint8), z((B, H, W), torch.float16)
    dm_old, dp, dd = torch.empty_like(logits), torch.empty_like(point), torch.empty_like(dirn)
    ws_old = torch.empty((lib.cdnet_dam_loss_classes_workspace_floats(B, P, 9),), dtype=torch.float32, device=dev)
    losses_old = torch.zeros(11, device=dev)
    dm_new = torch.empty_like(logits)
    ws_new = torch.empty((lib.cdnet_mask_loss_workspace_floats(B, P),), dtype=torch.float32, device=dev)
    losses_new = torch.zeros(8, device=dev)

    def parent_route():
        for t in (point, dirn, dirlab, pt):
            t.zero_()
        _lib.call('cdnet_dam_loss_classes', _lib.ptr(logits), _lib.ptr(point), _lib.ptr(dirn), _lib.ptr(label), _lib.ptr(dirlab), _lib.ptr(pt),
                  _lib.ptr(weight), B, H, W, 9, 1, _lib.ptr(ws_old), ws_old.numel(), _lib.ptr(losses_old), _lib.ptr(dm_old), _lib.ptr(dp),
                  _lib.ptr(dd), _lib.stream_ptr())

    def new_route():
        _lib.call('cdnet_mask_loss', _lib.ptr(logits), _lib.ptr(label), _lib.ptr(weight), B, H, W, 7, _lib.ptr(ws_new), ws_new.numel(),
                  _lib.ptr(losses_new), _lib.ptr(dm_new), _lib.stream_ptr())

    t_old, t_new = timed_each([parent_route, new_route], a.launches, a.warmup)
    same = bool(torch.equal(dm_old, dm_new) and torch.equal(losses_old[4:6], losses_new[1:3]))
    m_old, m_new = statistics.median(t_old) * 1e3, statistics.median(t_new) * 1e3
    line.update({'us_parent_route': round(m_old, 1), 'us_new_route': round(m_new, 1), 'ratio': round(m_new / m_old, 3), 'bar': 0.5,
                 'bar_met': bool(m_new / m_old <= 0.5), 'expected_from_bytes': round(40 / 211, 2), 'launches': a.launches,
                 'spread_parent_us': [round(min(t_old) * 1e3, 1), round(max(t_old) * 1e3, 1)],
                 'spread_new_us': [round(min(t_new) * 1e3, 1), round(max(t_new) * 1e3, 1)],
                 'new_GBps': round(B * P * 40 / m_new * 1e-3, 1), 'bit_equal': same})
    print('B=%d 256x256: parent route %.1f us (%.1f .. %.1f), cdnet_mask_loss %.1f us (%.1f .. %.1f), ratio %.3f (bar 0.5: %s), results bit-equal: %s'
          % (B, m_old, min(t_old) * 1e3, max(t_old) * 1e3, m_new, min(t_new) * 1e3, max(t_new) * 1e3, m_new / m_old,
             'met' if m_new / m_old <= 0.5 else 'MISSED', same), flush=True)
    print(json.dumps(line))


if __name__ == '__main__':
    main()
