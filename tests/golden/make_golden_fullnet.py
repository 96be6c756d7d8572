"""Regenerate tests/golden/fullnet.npz from the reference's FullNet class (models/FullNet.py:90-138).

CONTAINER-ONLY: imports the reference's class from /root/reference (read-only, never copied) through _ref_shims.  The fixture holds data only.

    python tests/golden/make_golden_fullnet.py

Keys:
  'keys_basic' / 'shapes_basic', 'keys_bottleneck' / 'shapes_bottleneck'   state_dict key names and shapes ('24,3,3,3'; '' for a scalar) of
        FullNet(3, 3) and FullNet(3, 3, layer_type='bottleneck') at the reference's defaults
  'nparams_basic'   parameter count of FullNet(3, 3) at the defaults (1 780 233)
  'small/keys', 'small/w/<i>'   the state_dict of FullNet(3, 3, n_layers=4, growth_rate=8, dilations=(1, 2, 8)) after
        tests/_fullnet_ref.randomize(model, 11), in key order
  'small/x'         f32 [2,3,40,36], bf16-exact
  'small/logits64'  f64 [2,3,40,36]: the reference class in eval mode, .double()
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _ref_shims  # noqa: E402
import _fullnet_ref as fr  # noqa: E402


def main():
    _ref_shims.install()
    from models.FullNet import FullNet
    out = {}
    for tag, kw in (('basic', {}), ('bottleneck', {'layer_type': 'bottleneck'})):
        sd = FullNet(3, 3, **kw).state_dict()
        out['keys_' + tag] = np.array(list(sd))
        out['shapes_' + tag] = np.array([','.join(str(d) for d in v.shape) for v in sd.values()])
    out['nparams_basic'] = np.int64(sum(p.numel() for p in FullNet(3, 3).parameters()))
    torch.manual_seed(0)
    m = fr.randomize(FullNet(**fr.SMALL), 11).eval()
    sd = m.state_dict()
    out['small/keys'] = np.array(list(sd))
    for i, v in enumerate(sd.values()):
        out['small/w/%d' % i] = v.numpy()
    x = fr.bf16_exact_input((2, 3, 40, 36), 12)
    out['small/x'] = x.numpy()
    with torch.no_grad():
        out['small/logits64'] = m.double()(x.double()).numpy()
    path = os.path.join(HERE, 'fullnet.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes;', sum(p.numel() for p in m.parameters()), 'parameters in the small network;',
          int(out['nparams_basic']), 'in the default one')


if __name__ == '__main__':
    main()
