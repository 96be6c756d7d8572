"""Regenerate tests/golden/fcn_pooling.npz from the reference's FCN_pooling class (models/FullNet.py:141-193).

Needs a checkout of the reference: its class is imported (read-only, never copied) through _ref_shims, as make_golden_fullnet.py does.  The fixture
holds data only.

    python tests/golden/make_golden_fcn_pooling.py

Keys:
  'keys_basic' / 'shapes_basic', 'keys_bottleneck' / 'shapes_bottleneck'   state_dict key names and shapes of FCN_pooling(3, 3) and
        FCN_pooling(3, 3, layer_type='bottleneck') at the reference's defaults
  'children'        names of the children of `blocks`, in order (block1, trans1, pool1, ..., trans5, upsample5, ..., block7, trans7)
  'small/keys', 'small/shapes', 'small/w'   the state_dict of FCN_pooling(3, 3, n_layers=4, growth_rate=4, dilations=(1, 2, 4, 8, 16, 4, 1))
        after tests/_fullnet_ref.randomize(model, 11): names, shapes and every tensor's values in key order in ONE flat f32 array (one zip
        member, not 217; num_batches_tracked is 0).  tests/_fcn_pooling_ref.golden_state splits it
  'small/x'         f32 [2,3,32,48], bf16-exact
  'small/logits64'  f64 [2,3,32,48]: the reference class in eval mode, .double()
  'small/label', 'small/weight'   u8 [2,32,48]: the fixed label (0..2) and weight map (1..60) of the training step
  'small/train_logits64', 'small/train_loss64', 'small/grad_keys', 'small/grads'   the same network with drop_rate=0 in train(), .double():
        logits, the 'total' of oracle.train.unet_losses and the gradient of every parameter in named_parameters() order, one flat f64 array
        (tests/_fcn_pooling_ref.golden_grads splits it by the state_dict's shapes)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _ref_shims  # noqa: E402
import _fullnet_ref as fr  # noqa: E402
import _fullnet_train_ref as tr  # noqa: E402
import _fcn_pooling_ref as pr  # noqa: E402


def main():
    _ref_shims.install()
    from models.FullNet import FCN_pooling
    from oracle import train as ot
    out = {}
    for tag, kw in (('basic', {}), ('bottleneck', {'layer_type': 'bottleneck'})):
        sd = FCN_pooling(3, 3, **kw).state_dict()
        out['keys_' + tag] = np.array(list(sd))
        out['shapes_' + tag] = np.array([','.join(str(d) for d in v.shape) for v in sd.values()])
    out['children'] = np.array([n for n, _ in FCN_pooling(3, 3).blocks.named_children()])
    torch.manual_seed(0)
    m = fr.randomize(FCN_pooling(**pr.GOLDEN), 11).eval()
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    out['small/keys'] = np.array(list(sd))
    out['small/shapes'] = np.array([','.join(str(d) for d in v.shape) for v in sd.values()])
    out['small/w'] = np.concatenate([v.numpy().astype(np.float32).ravel() for v in sd.values()])
    x = fr.bf16_exact_input(pr.GOLDEN_SHAPE, 12)
    out['small/x'] = x.numpy()
    with torch.no_grad():
        out['small/logits64'] = m.double()(x.double()).numpy()
    _, label, weight = tr.batch(pr.GOLDEN_SHAPE, 13)
    out['small/label'], out['small/weight'] = label.numpy(), weight.numpy()
    t = FCN_pooling(drop_rate=0.0, **pr.GOLDEN)
    t.load_state_dict(sd, strict=True)
    t = t.double().train()
    logits = t(x.double())
    loss = ot.unet_losses(logits, label, weight)['total']
    loss.backward()
    out['small/train_logits64'] = logits.detach().numpy()
    out['small/train_loss64'] = loss.detach().numpy().reshape(1)
    out['small/grad_keys'] = np.array([n for n, _ in t.named_parameters()])
    out['small/grads'] = np.concatenate([p.grad.numpy().ravel() for _, p in t.named_parameters()])
    path = os.path.join(HERE, 'fcn_pooling.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes;', sum(p.numel() for p in m.parameters()), 'parameters in the small network')


if __name__ == '__main__':
    main()
