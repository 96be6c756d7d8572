"""The frozen-encoder training step (`encoder_freeze=True`) beside the unfrozen one of `UNet2RevA1_vgg16`, in one process on one box.

    python3 tools/bench_finetune.py [--batch 16] [--size 256] [--rounds 12] [--warmup 4] [--precisions fp32,bf16]

Two models from the same seed, two trainers, the same synthetic batch.  After --warmup steps of each, --rounds rounds of
(unfrozen step, frozen step), alternating, a device event pair around every step and one synchronisation per round; the record holds the
median and the quartiles of each, and the median of the per-round differences (neighbouring steps see the same clocks).  A second record
counts the library calls of one step of each (forward / loss / backward / optimiser) by wrapping `_lib.call`.  One JSON line per record.
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


def build(freeze, dev):
    from cdnet_amd import trainer
    from cdnet_amd.models.dam.model_unet_rev1 import Unet
    torch.manual_seed(0)
    m = Unet(backbone_name='vgg16_bn', pretrained=False, encoder_freeze=freeze, classes=3).to(dev)
    return m, trainer.Trainer(m)


def count_calls(tr, batch):
    from cdnet_amd import _lib
    counts, phase, real = {}, ['forward'], _lib.call

    def call(name, *args):
        counts.setdefault(phase[0], {}).setdefault(name, 0)
        counts[phase[0]][name] += 1
        return real(name, *args)
    _lib.call = call
    try:
        out = tr.forward(batch[0])
        phase[0] = 'loss'
        g = tr.loss_and_grads(out[0], out[1], out[2], *batch[1:])
        phase[0] = 'backward'
        tr.backward(*g)
        phase[0] = 'step'
        tr.allreduce_and_step()
        torch.cuda.synchronize()
    finally:
        _lib.call = real
    return counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--rounds', type=int, default=12)
    ap.add_argument('--warmup', type=int, default=4)
    ap.add_argument('--precisions', default='fp32,bf16')
    a = ap.parse_args()
    import cdnet_amd
    from cdnet_amd import synth
    dev = torch.device('cuda:0')
    torch.cuda.set_device(0)
    batch = synth.synthetic_batch(a.batch, dev, seed=2022, H=a.size, W=a.size)
    for prec in a.precisions.split(','):
        cdnet_amd.set_precision(prec)
        runs = {name: build(freeze, dev) for name, freeze in (('unfrozen', False), ('frozen', True))}
        for _ in range(a.warmup):
            for m, tr in runs.values():
                tr.train_step(*batch)
        torch.cuda.synchronize()
        ms = {name: [] for name in runs}
        for _ in range(a.rounds):
            ev = {}
            for name, (m, tr) in runs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                tr.train_step(*batch)
                e1.record()
                ev[name] = (e0, e1)
            torch.cuda.synchronize()
            for name, (e0, e1) in ev.items():
                ms[name].append(e0.elapsed_time(e1))
        u, f = np.array(ms['unfrozen']), np.array(ms['frozen'])
        q = lambda v: [round(float(x), 3) for x in np.percentile(v, [25, 50, 75])]
        say(what='train_step', precision=prec, batch=a.batch, size=a.size, rounds=a.rounds, unfrozen_ms_q25_q50_q75=q(u),
            frozen_ms_q25_q50_q75=q(f), saved_ms_median_of_pairs=round(float(np.median(u - f)), 3),
            saved_ms_q25_q75=[round(float(x), 3) for x in np.percentile(u - f, [25, 75])],
            tiles_per_s=dict(unfrozen=round(a.batch / float(np.median(u)) * 1e3, 1), frozen=round(a.batch / float(np.median(f)) * 1e3, 1)))
        cu, cf = (count_calls(runs[name][1], batch) for name in ('unfrozen', 'frozen'))
        gone = {ph: {n: c - cf.get(ph, {}).get(n, 0) for n, c in names.items() if c != cf.get(ph, {}).get(n, 0)} for ph, names in cu.items()}
        say(what='calls', precision=prec, unfrozen={ph: sum(v.values()) for ph, v in cu.items()},
            frozen={ph: sum(v.values()) for ph, v in cf.items()}, gone={ph: v for ph, v in gone.items() if v},
            narrowed_backward_data=runs['frozen'][1].narrowed)
        del runs
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
