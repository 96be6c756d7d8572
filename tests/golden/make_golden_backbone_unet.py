"""Regenerate tests/golden/backbone_unet.npz from the reference's backbone U-Net class (models/model_unet.py:136-196, `UNet_vgg16`).

Needs a checkout of the reference: its class is imported (read-only, never copied) through _ref_shims, whose stand-in for
torchvision.models.vgg16_bn needs no torchvision.  The class is constructed DIRECTLY with pretrained=False - never through the reference's
chooseModel, which asks torchvision for the ImageNet weights.  The fixture holds data only; the weights are closed-form
(cdnet_amd.synth.det_fill_state_dict) and are not stored.

    python tests/golden/make_golden_backbone_unet.py

Keys:
  'keys'            state_dict key names of Unet(backbone_name='vgg16_bn', pretrained=False, encoder_freeze=False, classes=3), in order
  'n_params'        [number of parameters]
  'x_cfg', 'x_ragged_cfg'   [N, C, H, W, seed] of cdnet_amd.synth.det_input for the two inputs
  'y_eval', 'y_eval_ragged' f16: the reference class's eval logits under det_fill weights for those inputs
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _ref_shims  # noqa: E402

CASES = {'y_eval': ((2, 3, 64, 64), 1), 'y_eval_ragged': ((1, 3, 48, 64), 12)}


def main():
    _ref_shims.install()
    from models.model_unet import Unet
    from cdnet_amd import synth
    m = Unet(backbone_name='vgg16_bn', pretrained=False, encoder_freeze=False, classes=3)
    bn = {n for n, mod in m.named_modules() if isinstance(mod, torch.nn.BatchNorm2d)}
    with torch.no_grad():
        synth.det_fill_state_dict(m.state_dict(), bn)
    m.eval()
    out = {'keys': np.array(list(m.state_dict().keys())), 'n_params': np.array([sum(p.numel() for p in m.parameters())], np.int64)}
    for key, (shape, seed) in CASES.items():
        with torch.no_grad():
            y = m(torch.from_numpy(synth.det_input(shape, seed)))
        assert tuple(y.shape) == (shape[0], 3) + shape[2:] and float(y.abs().max()) < 6e4
        out[key] = y.numpy().astype(np.float16)
        out[key.replace('y_eval', 'x') + '_cfg'] = np.array(list(shape) + [seed], np.int64)
    path = os.path.join(HERE, 'backbone_unet.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes;', int(out['n_params'][0]), 'parameters; max |logit|',
          [float(np.abs(out[k].astype(np.float32)).max()) for k in CASES])


if __name__ == '__main__':
    main()
