"""Rate of the device training augmentation (cdnet_amd/augment.py, csrc/augment.hip) against its host implementation.

    python tools/bench_augment.py [--batch 16] [--src 1000] [--size 256] [--iters 50] [--host-samples 2] [--recipe full] [--channels 1]

Prints one JSON line: ms per batch of B sources of src x src into size x size tiles for augmentation alone (default recipe: alpha 1,
sigma 50), augmentation + label encoding, and the host implementation (PIL + numpy + scipy, one core) per batch (extrapolated from
--host-samples samples), with the box record (device name, clocks as torch reports them).  With --recipe full the nine-step recipe
(random_resize [1, 2], random_affine 0.3 and random_rotation added) is timed beside the default one in the same process, and the line
carries both times and their ratio.  --channels 1 times the mode-L path (grey-scale sources, the channels = 1 entries) the same way."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def epoch_rates(a, items):
    """last-epoch tiles/s of the training entry (3 epochs, the first two warm) on 2 x batch rendered sources, plain and --device-augment"""
    import logging
    import re
    import tempfile
    from PIL import Image
    from cdnet_amd import train
    from cdnet_amd.options import Options
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, 'data', Options(isTrain=True).dataset)
        dirs = [os.path.join(root, d, 'train') for d in ('images', 'weight_maps', 'labels')]
        for d in dirs:
            os.makedirs(d)
        for k in range(2 * a.batch):
            img, w, lab = items[k % len(items)]
            lab3 = np.zeros(lab.shape + (3,), np.uint8)
            lab3[..., 0], lab3[..., 2] = lab, 255 - lab
            Image.fromarray(img).save(os.path.join(dirs[0], 'im%d.png' % k))
            Image.fromarray(w).save(os.path.join(dirs[1], 'im%d_weight.png' % k))
            Image.fromarray(lab3).save(os.path.join(dirs[2], 'im%d_label.png' % k))
        cwd = os.getcwd()
        os.chdir(tmp)
        try:
            for name, extra in (('plain', []), ('device_augment', ['--device-augment'])):
                rec = []
                h = logging.Handler()
                h.emit = lambda r: rec.append(r.getMessage())
                logging.getLogger('cdnet_amd.train').addHandler(h)
                train.main(extra + ['--epochs', '3', '--batch-size', str(a.batch), '--input-size', str(a.size), '--save-dir', os.path.join(tmp, name)])
                logging.getLogger('cdnet_amd.train').removeHandler(h)
                rates = [float(m.group(1)) for m in (re.search(r'\(([0-9.]+) tiles/s', x) for x in rec) if m]
                out[name] = rates[-1]
        finally:
            os.chdir(cwd)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--src', type=int, default=1000)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--host-samples', type=int, default=2)
    ap.add_argument('--recipe', choices=('default', 'full'), default='default',
                    help='full: also time all nine steps (resize, affine and rotation added) beside the default recipe')
    ap.add_argument('--channels', type=int, choices=(1, 3), default=3, help='1: mode-L sources (a grey-scale dataset), the channels = 1 entries')
    ap.add_argument('--epoch-rate', action='store_true',
                    help='also: tiles/s of `python -m cdnet_amd.train` epochs over a folder of --batch x 2 sources, with and without --device-augment')
    a = ap.parse_args()
    from cdnet_amd import augment, synth
    from cdnet_amd.my_transforms_direction import label_encoding_batch
    dev = torch.device('cuda:0')
    rs = np.random.RandomState(0)
    items = []
    for k in range(a.batch):
        inst = synth.ellipse_instances(a.src, a.src, 300, rs, 6, 14, 8)
        lab = np.where(inst > 0, 255, 0).astype(np.uint8)
        img = rs.randint(0, 256, (a.src, a.src, 3)).astype(np.uint8)
        items.append((img if a.channels == 3 else np.ascontiguousarray(img[..., 0]), np.full((a.src, a.src), 20, np.uint8), lab))
    srcs = [augment.Source(*it, dev) for it in items]
    rec = augment.Recipe(size=a.size)
    params = [[augment.draw_params(rs, a.src, a.src, rec) for _ in srcs] for _ in range(a.iters)]

    def run(with_le, params=params):
        for it in range(3):
            augment.augment_batch(srcs, params[it], a.size)
        torch.cuda.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for ps in params:
            img, w, lab, varied = augment.augment_batch(srcs, ps, a.size)
            if with_le:
                label_encoding_batch(lab)
        ev1.record()
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1) / a.iters
    aug_ms = run(False)
    aug_le_ms = run(True)
    full = None
    if a.recipe == 'full':
        frec = augment.Recipe(size=a.size, resize=(1, 2), affine=0.3, rotation=True)
        fparams = [[augment.draw_params(rs, a.src, a.src, frec) for _ in srcs] for _ in range(a.iters)]
        full_ms, again_ms = run(False, fparams), run(False)              # the default recipe once more after it: drift shows as a gap
        edges = [max(augment.field_box(p, *p.dims(a.src, a.src), a.size)[2] for p in ps) for ps in fparams]
        full = {'augment_ms_per_batch': round(full_ms, 4), 'default_again_ms_per_batch': round(again_ms, 4),
                'full_over_default': round(full_ms / aug_ms, 2), 'mean_field_edge': round(float(np.mean(edges)), 1),
                'default_field_edge': a.size + 2 * augment.HALO}
    t0 = time.perf_counter()
    for k in range(a.host_samples):
        augment.augment_host(*items[k], params[0][k], a.size)
    host_ms = (time.perf_counter() - t0) / a.host_samples * a.batch * 1e3
    if a.epoch_rate and a.channels != 3:
        raise SystemExit('--epoch-rate renders an RGB folder for the default dataset: run it with --channels 3')
    epochs = epoch_rates(a, items) if a.epoch_rate else None
    p = torch.cuda.get_device_properties(0)
    print(json.dumps({'tool': 'bench_augment', 'batch': a.batch, 'src': a.src, 'size': a.size, 'iters': a.iters, 'channels': a.channels,
                      'augment_ms_per_batch': round(aug_ms, 4), 'augment_label_encoding_ms_per_batch': round(aug_le_ms, 4),
                      'tiles_per_s': round(a.batch / aug_le_ms * 1e3, 1), 'host_ms_per_batch': round(host_ms, 1),
                      'host_over_device': round(host_ms / aug_le_ms, 1), 'epoch_tiles_per_s': epochs, 'full_recipe': full,
                      'box': {'device': p.name, 'gcn_arch': getattr(p, 'gcnArchName', ''), 'cus': p.multi_processor_count}}))


if __name__ == '__main__':
    main()
