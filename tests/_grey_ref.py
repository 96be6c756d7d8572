"""CPU mirror of the one-channel backbone U-Net: tests/_backbone_unet_ref.py's BackboneUnet with `child0` (Conv2d(1, 64, 3, padding=1))
applied in place of backbone child '0', as the reference's forward_backbone does for x.shape[1] != 3; backbone child '1' (its BatchNorm)
and everything behind are the three-channel network's.  Plain PyTorch, no device code.

  GreyBackboneUnet                  the network; forward(x [N,1,H,W]) in the dtype of its parameters (.double(): the fp64 mirror)
  eval_rounded_forward(net, x)      eval-mode forward with the 16-bit path's rounding points (_backbone_unet_ref.eval_rounded_forward's)
  embed(net)                        the three-channel BackboneUnet whose stem is cat(child0.weight, 0, 0) with child0's bias
"""
import torch

import _backbone_unet_ref as br
from oracle import models as om


class GreyBackboneUnet(br.BackboneUnet):
    def forward(self, x):
        feats = {}
        for name, child in self.backbone.named_children():
            x = self.child0(x) if name == '0' else child(x)
            if name in br.SKIPS:
                feats[name] = x
            if name == br.BB_OUT:
                break
        for skip_name, blk in zip(br.SKIPS[::-1], self.upsample_blocks):
            x = blk(x, feats[skip_name])
        return self.final_conv(x)


class _Child0Stem:
    """view of a GreyBackboneUnet for _backbone_unet_ref's walkers: the same modules, child0 standing where backbone child '0' stands"""

    def __init__(self, net):
        children = [(n, net.child0 if n == '0' else m) for n, m in net.backbone.named_children()]
        self.backbone = torch.nn.Sequential()
        for n, m in children:
            self.backbone.add_module(n, m)
        self.upsample_blocks, self.final_conv = net.upsample_blocks, net.final_conv


def eval_rounded_forward(net, x):
    return br.eval_rounded_forward(_Child0Stem(net), x)


def det_model(classes=3):
    """the closed-form weights of the golden fixtures (oracle.models.det_fill), child0 included"""
    return om.det_fill(GreyBackboneUnet(classes))


def random_model(seed=0, classes=3):
    ref = br.random_model(seed, classes)
    net = GreyBackboneUnet(classes)
    net.load_state_dict(ref.state_dict())
    return net


def embed(net):
    """the three-channel network that computes the same function of cat(x, 0, 0)"""
    out = br.BackboneUnet(net.final_conv.out_channels)
    out.load_state_dict(net.state_dict())
    with torch.no_grad():
        w = out.backbone[0].weight
        w.zero_()
        w[:, :1].copy_(net.child0.weight)
        out.backbone[0].bias.copy_(net.child0.bias)
    return out.to(next(net.parameters()).dtype)
