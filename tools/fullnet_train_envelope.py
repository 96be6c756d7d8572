"""CPU check of the bar of tests/test_gpu_fullnet_train.py: for every one-step case the envelope (tests/_fullnet_train_ref.py: the fp64
mirror's change under independent relative 2^-16 errors at every product site, maximum over the test's seeds) against one more,
independent seed.  The bar of the GPU test is 3 envelopes; it is sound when an independent draw of the same error model stays well inside it (1.5).
Without a device the sign masks are those of the clean forward and the dropout masks Bernoulli draws.  --net FCN_pooling: the cases of
tests/test_gpu_fcn_pooling.py on tests/_fcn_pooling_ref.py, whose pools' arg-max indices are those of the clean forward too.

  python tools/fullnet_train_envelope.py [--net FullNet|FCN_pooling] [--seeds 8] [--probe 9]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seeds', type=int, default=0, help="default: the tests' own count per case")
    ap.add_argument('--probe', type=int, default=9)
    ap.add_argument('--net', choices=['FullNet', 'FCN_pooling'], default='FullNet')
    args = ap.parse_args()
    import _fullnet_ref as fr
    import _fullnet_train_ref as tr
    import _fcn_pooling_ref as pr
    from oracle import train as ot
    from cdnet_amd.models.FullNet import FCN_pooling, FullNet
    pooled = args.net == 'FCN_pooling'
    cls, cases, base = (FCN_pooling, pr.CASES, 100) if pooled else (FullNet, tr.CASES, 0)
    print('%-12s %6s %8s %12s %12s  %s' % ('network', 'seeds', 'tensors', 'worst ratio', 'median env', 'worst tensor'))
    for k, (name, (kw, dil, shape)) in enumerate(cases.items()):
        nseeds = args.seeds or len(pr.ENVELOPE_SEEDS[name] if pooled else tr.ENVELOPE_SEEDS)
        m = fr.randomize(cls(**kw), base + 60 + k)
        sd = {n: v.clone() for n, v in m.state_dict().items()}
        x, label, weight = tr.batch(shape, base + 70 + k)
        p = float(kw.get('drop_rate', 0.1))
        g = torch.Generator().manual_seed(80 + k)
        drops = {}
        if p > 0:
            for prefix, _, last in tr.conv_prefixes(sd, dil):
                if last:
                    c = sd[prefix + '.conv.weight'].shape[0]
                    d = (1, 2, 4, 8, 16, 4, 1)[int(prefix.split('.')[1][5:]) - 1] if pooled else 1       # the block's map size
                    drops[prefix] = torch.rand((shape[0], c, shape[2] // d, shape[3] // d), generator=g) >= p
        loss_fn = lambda lg: ot.unet_losses(lg, label, weight)['total']
        signs = {}
        if pooled:
            pools = {}
            clean, env = pr.envelope(sd, x, dil, signs, drops, p, pools, loss_fn, range(1, nseeds + 1))
            _, probe = pr.envelope(sd, x, dil, signs, drops, p, pools, loss_fn, [args.probe + 1000], clean=clean)
        else:
            clean, env = tr.envelope(sd, x, dil, signs, drops, p, loss_fn, range(1, nseeds + 1))
            _, probe = tr.envelope(sd, x, dil, signs, drops, p, loss_fn, [args.probe + 1000], clean=clean)
        ratios = {n: probe[n] / env[n] for n in env if env[n] > 0}
        worst = max(ratios, key=ratios.get)
        med = sorted(env.values())[len(env) // 2]
        print('%-12s %6d %8d %12.2f %12.3e  %s' % (name, nseeds, len(env), ratios[worst], med, worst))


if __name__ == '__main__':
    main()
