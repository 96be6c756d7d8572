"""`Unet` - the backbone U-Net baseline `UNet_vgg16` of the reference (models/model_unet.py:136-196): CDNet's VGG16-BN encoder and
transposed-conv decoder with a plain 1x1 classifier (`final_conv`, 16 -> classes) where the direction-aware head would be.

Same constructor arguments, same `forward(x) -> logits [N,classes,H,W]` (float32 NCHW), same state_dict keys in the same order
(backbone.N.*, upsample_blocks.i.{up,bn1,conv2,bn2}.*, final_conv.*, and the reference's never-used child0 / child_conv1), so
checkpoints interchange.  The class is the 'plain' variant of models/dam/model_unet_rev1.Unet: encoder and decoder run on that class's
kernels (ragged sizes through its pad_offsets path included), the classifier on cdnet_final_conv1x1_c16.  Training:
cdnet_amd.trainer.BackboneUNetTrainer (the plain UNet's loss around the rev1 tape).  There is no CPU fallback.

Only the 'vgg16_bn' backbone is built: the ResNet encoders (UNet_resnet50 / UNet_resnet101) need a 7x7 stride-2 stem, a 3x3 stride-2
max-pool and strided bottlenecks this library has no kernels for.  `pretrained` (False, True or a path) and `encoder_freeze` mean what
they mean for models/dam/model_unet_rev1.Unet: a torchvision vgg16_bn file from disk into `backbone` (get_backbone; nothing is
downloaded), and an encoder that gets no gradient and no step.
"""
import ctypes as C

import torch

from .. import _lib, runtime
from .dam.model_unet_rev1 import Unet as _Rev1


class Unet(_Rev1):
    VARIANT = 'plain'
    # parameters the reference's forward never touches for 3-channel input (no gradient, never stepped); final_conv IS used here
    UNUSED_PREFIXES = ('child0.', 'child_conv1.')

    def __init__(self, backbone_name='vgg16_bn', pretrained=True, encoder_freeze=False, classes=21,
                 decoder_filters=(256, 128, 64, 32, 16), parametric_upsampling=True, shortcut_features='default',
                 decoder_use_batchnorm=True):
        if backbone_name != 'vgg16_bn':
            raise NotImplementedError("backbone '{}': only 'vgg16_bn' is built; the ResNet encoders of models/model_unet.py "
                                      '(UNet_resnet50 / UNet_resnet101) are not built'.format(backbone_name))
        super().__init__(backbone_name=backbone_name, pretrained=pretrained, encoder_freeze=encoder_freeze, classes=classes,
                         decoder_filters=decoder_filters, parametric_upsampling=parametric_upsampling,
                         shortcut_features=shortcut_features, decoder_use_batchnorm=decoder_use_batchnorm)
        assert self.final_conv.in_channels == 16, 'cdnet_final_conv1x1_c16 serves the default decoder (16 channels at full resolution)'

    def forward(self, *input):
        x = input[0]
        if not x.is_cuda:
            raise RuntimeError('cdnet_amd.models.model_unet.Unet runs on the MI355X only (no CPU fallback)')
        return self._head(self.forward_features(x, self.training))

    def forward_packed(self, x16):
        """forward on already packed NHWC windows [N,H,W,16] (sliding-window / TTA inference).  Returns `(logits,)`."""
        return (self._head(self.forward_features_packed(x16, self.training)),)

    def _head(self, t):
        """final_conv (:166,194) on the last decoder block's feature: raw output with BatchNorm + ReLU pending in training, a stored
        activated tensor in eval"""
        N, H, W, _ = t.x.shape
        K = self.final_conv.out_channels
        out = torch.empty((N, K, H, W), dtype=torch.float32, device=t.x.device)
        hf = runtime.head_feat16(t)
        _lib.call('cdnet_final_conv1x1_c16', C.byref(hf), _lib.ptr(self.final_conv.weight.detach().reshape(K, 16).contiguous()),
                  _lib.ptr(self.final_conv.bias.detach()), K, N, H, W, _lib.ptr(out), _lib.stream_ptr())
        self._last_feat = t
        return out
