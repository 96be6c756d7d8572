"""Plain functional PyTorch forward of FullNet from a state dict: conv2d with dilation -> leaky_relu(0.01) -> eval batch_norm -> cat.
The fp64 reference of the FullNet GPU tests (tests/test_fullnet_cpu.py pins it to the reference class through tests/golden/fullnet.npz).

The state dict does not say which dilation a layer has: `dilations` is one tuple per dense block."""
import numpy as np
import torch
import torch.nn.functional as F

SMALL = dict(color_channels=3, output_channels=3, n_layers=4, growth_rate=8, dilations=(1, 2, 8))     # the golden configuration
SMALL_DILATIONS = ((1, 1, 1, 1), (1, 2, 3, 2), (3, 7, 10, 13))
DEFAULT_DILATIONS = ((1, 1, 1, 1, 1, 1), (1, 2, 3, 1, 2, 3), (1, 2, 3, 5, 6, 7), (2, 5, 7, 9, 11, 14), (10, 13, 16, 17, 19, 21),
                     (1, 2, 3, 5, 6, 7), (1, 1, 1, 1, 1, 1))


def bf16_round(t):
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def _conv_layer(sd, prefix, x, dilation, quant):
    w = quant(sd[prefix + '.conv.weight'].to(x.dtype))
    three = w.shape[2] == 3
    y = F.conv2d(x, w, padding=dilation if three else 0, dilation=dilation if three else 1)
    y = F.leaky_relu(y, 0.01)
    g = lambda k: sd[prefix + '.bn.' + k].to(x.dtype)
    y = F.batch_norm(y, g('running_mean'), g('running_var'), g('weight'), g('bias'), training=False, eps=1e-5)
    return quant(y)


def forward(sd, x, dilations, dtype=torch.float64, quant=None):
    """logits [N,K,H,W] in `dtype`.  quant (e.g. bf16_round) is applied to every convolution weight and to every stored layer output (not to
    the input, the BatchNorm parameters or the logits)."""
    quant = quant or (lambda t: t)
    sd = {k: v.detach().cpu() for k, v in sd.items()}
    x = _conv_layer(sd, 'conv1', x.to(dtype), 1, quant)
    for i, ds in enumerate(dilations):
        for j, d in enumerate(ds):
            p = 'blocks.block%d.denselayer%d' % (i + 1, j + 1)
            if p + '.conv.conv.weight' in sd:
                out = _conv_layer(sd, p + '.conv', x, d, quant)
            else:
                out = _conv_layer(sd, p + '.conv2', _conv_layer(sd, p + '.conv1', x, 1, quant), d, quant)
            x = torch.cat([x, out], 1)
        x = _conv_layer(sd, 'blocks.trans%d' % (i + 1), x, 1, quant)
    return F.conv2d(x, quant(sd['conv2.weight'].to(dtype)), padding=1)


def randomize(model, seed):
    """seeded parameters that keep activations O(1) through 50 layers: convolution weights randn / sqrt(Cin * taps); BatchNorm weight
    U(0.5, 1.5) with every fifth one negative, bias and running_mean 0.1 randn, running_var U(0.5, 1.5)"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, m in model.named_modules():
            if isinstance(m, torch.nn.Conv2d):
                k = m.weight.shape[1] * m.weight.shape[2] * m.weight.shape[3]
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) / np.sqrt(k))
            elif isinstance(m, torch.nn.BatchNorm2d):
                c = m.weight.numel()
                w = 0.5 + torch.rand(c, generator=g)
                w[torch.arange(c) % 5 == 2] *= -1
                m.weight.copy_(w)
                m.bias.copy_(0.1 * torch.randn(c, generator=g))
                m.running_mean.copy_(0.1 * torch.randn(c, generator=g))
                m.running_var.copy_(0.5 + torch.rand(c, generator=g))
    return model


def bf16_exact_input(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(torch.bfloat16).to(torch.float32)


def perturbed(sd, seed, rel=2.0 ** -16):
    """the state dict in fp64 with every weight (convolution and BatchNorm `weight`) multiplied by 1 + rel U(-1, 1)"""
    g = torch.Generator().manual_seed(seed)
    return {k: (v.double() * (1 + rel * (2 * torch.rand(v.shape, generator=g, dtype=torch.float64) - 1)) if k.endswith('.weight') else v)
            for k, v in sd.items()}
