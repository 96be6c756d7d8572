"""Rate of the optimiser kernels (csrc/optim.hip: moment_kernel, sgd_kernel, adam_kernel), one process, one box.

    python tools/bench_optim.py [--n 20470000] [--launches 40] [--warmup 10] [--offset 0]

Every rule is launched --warmup times, then --launches times with a pair of device events around each launch; the figure is the
median.  GB/s counts algorithmic traffic: Adam and the moment rules read p, g, m, v and write p, m, v (7 streams x 4 B per element),
Ranger on a lookahead step also reads and writes the slow weights (9), a step that leaves the parameters alone (RAdam_4step, steps 1-4)
moves 5, SGD reads p, g, buf and writes p, buf (5).  --offset k starts every buffer k elements behind a 16-byte boundary (the slices
of bucket-wise stepping).  Prints one line per rule and one JSON line at the end."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=20470000)
    ap.add_argument('--launches', type=int, default=40)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--offset', type=int, default=0)
    a = ap.parse_args()
    from cdnet_amd import _lib, optim
    dev = torch.device('cuda:0')
    n, o = a.n, a.offset
    torch.manual_seed(0)
    bufs = {k: torch.zeros(n + 8, device=dev)[o:o + n] for k in ('p', 'g', 'm', 'v', 's')}
    bufs['p'].normal_(0, 0.05)
    bufs['g'].normal_(0, 0.1)
    bufs['s'].copy_(bufs['p'])
    P, G, M, V, S = (_lib.ptr(bufs[k]) for k in ('p', 'g', 'm', 'v', 's'))
    lr, wd = 1e-3, 1e-4

    def moment(rule, t):
        s = optim.moment_scalars(rule, t, lr, wd)
        return lambda: _lib.call('cdnet_moment_step', P, G, M, V, S if s['sync'] else None, n, 0.9, 0.99, 1.0, s['move'], s['rect'], s['decay'],
                                 s['step_size'], s['v_div'], s['eps'], s['sync'], s['alpha'], _lib.stream_ptr())
    rules = [('adam (adam_kernel)', 7, lambda: _lib.call('cdnet_adam_step', P, G, M, V, n, lr, 0.9, 0.99, 1e-8, wd, 7, 1.0, _lib.stream_ptr())),
             ('radam, rectified (step 7)', 7, moment('radam', 7)),
             ('radam, plain (step 3)', 7, moment('radam', 3)),
             ('radam4s, no move (step 3)', 5, moment('radam4s', 3)),
             ('radam4s (step 7)', 7, moment('radam4s', 7)),
             ('adamw (step 7)', 7, moment('adamw', 7)),
             ('ranger (step 7)', 7, moment('ranger', 7)),
             ('ranger, lookahead (step 6)', 9, moment('ranger', 6)),
             ('sgd (step 7)', 5, lambda: _lib.call('cdnet_sgd_step', P, G, M, n, lr, 0.95, wd, 7, 1.0, _lib.stream_ptr()))]
    out = {}
    for name, streams, fn in rules:
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.launches)]
        for e0, e1 in evs:
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()
        us = statistics.median(e0.elapsed_time(e1) for e0, e1 in evs) * 1e3
        gbs = streams * 4 * n / us * 1e-3
        out[name] = {'us': round(us, 1), 'streams': streams, 'GBps': round(gbs, 1)}
        print('%-30s %8.1f us  %d streams  %7.1f GB/s' % (name, us, streams, gbs), flush=True)
    base = out['adam (adam_kernel)']['GBps']
    p = torch.cuda.get_device_properties(0)
    print(json.dumps({'tool': 'bench_optim', 'n': n, 'offset': o, 'launches': a.launches, 'warmup': a.warmup, 'rules': out,
                      'GBps_over_adam': {k: round(v['GBps'] / base, 3) for k, v in out.items()},
                      'box': {'device': p.name, 'gcn_arch': getattr(p, 'gcnArchName', ''), 'cus': p.multi_processor_count}}))


if __name__ == '__main__':
    main()
