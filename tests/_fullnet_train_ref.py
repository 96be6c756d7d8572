"""fp64 mirror of FullNet in training mode on plain functional PyTorch with autograd (reference models/FullNet.py:14-52 in train()):
conv2d -> LeakyReLU -> batch-statistics BatchNorm (running statistics with momentum 0.1 and the unbiased variance) -> dropout on the
channels a dense layer appends -> cat.

The dropout masks AND the LeakyReLU sign masks are inputs: z = c * where(sign, 1, 0.01).  With free signs a single flip moves a gradient
discontinuously (two independent 2^-16 perturbations of one network differed by up to 37x per tensor; with the signs held 2.3-3.4x), so the
device hands over the masks it used and the mirror - and every perturbed copy of it - computes with them.

`perturb` (a torch.Generator) gives every product site an independent relative 2^-16 U(-1, 1) error, the size of a split-bf16 product's:
the weights in forward, the weights and g in backward-data, x and g in the weight gradient, and the network input.  The change of the
mirror's results under it is the envelope of tests/test_gpu_fullnet_train.py."""
import torch
import torch.nn.functional as F
from torch.nn import grad as G

REL = 2.0 ** -16


def _noise(t, gen):
    return t * (1 + REL * (2 * torch.rand(t.shape, generator=gen, dtype=torch.float64) - 1))


class _PerturbedConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, pad, dil, gen):
        ctx.save_for_backward(x, w)
        ctx.pad, ctx.dil, ctx.gen = pad, dil, gen
        return F.conv2d(x, _noise(w, gen), padding=pad, dilation=dil)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        gen = ctx.gen
        dx = G.conv2d_input(x.shape, _noise(w, gen), _noise(g, gen), padding=ctx.pad, dilation=ctx.dil) if ctx.needs_input_grad[0] else None
        dw = G.conv2d_weight(_noise(x, gen), w.shape, _noise(g, gen), padding=ctx.pad, dilation=ctx.dil)
        return dx, dw, None, None, None


def _conv(x, w, d, gen):
    pad, dil = (d, d) if w.shape[2] == 3 else (0, 1)
    if gen is None:
        return F.conv2d(x, w, padding=pad, dilation=dil)
    return _PerturbedConv.apply(x, w, pad, dil, gen)


def conv_prefixes(sd, dilations):
    """[(prefix of a ConvLayer, dilation, is the last ConvLayer of a dense layer)] in forward order, then the transitions in place"""
    out = [('conv1', 1, False)]
    for i, ds in enumerate(dilations):
        for j, d in enumerate(ds):
            p = 'blocks.block%d.denselayer%d' % (i + 1, j + 1)
            if p + '.conv.conv.weight' in sd:
                out.append((p + '.conv', d, True))
            else:
                out += [(p + '.conv1', 1, False), (p + '.conv2', d, True)]
        out.append(('blocks.trans%d' % (i + 1), 1, False))
    return out


def forward(params, buffers, x, dilations, signs, drops, p_drop, perturb=None):
    """params: {name: fp64 leaf tensor} (convolution and BatchNorm weights / biases); buffers: {name: fp64} running statistics;
    signs: {ConvLayer prefix: bool [N,C,H,W]}; drops: {ConvLayer prefix: kept mask [N,C,H,W]} (empty with p_drop = 0).
    Returns (logits, {running statistic name: its value after this forward})."""
    gen = perturb
    stats = {}
    x = x.double()
    if gen is not None:
        x = _noise(x, gen)

    def layer(prefix, x, d):
        c = _conv(x, params[prefix + '.conv.weight'], d, gen)
        if prefix not in signs:                     # (CPU studies without a device: the signs of this very forward, recorded for the next ones)
            signs[prefix] = c.detach() > 0
        z = c * torch.where(signs[prefix], 1.0, 0.01)
        n = z.numel() // z.shape[1]
        mean, var = z.mean((0, 2, 3)), z.var((0, 2, 3), unbiased=False)
        y = (z - mean.view(1, -1, 1, 1)) / torch.sqrt(var.view(1, -1, 1, 1) + 1e-5)
        y = y * params[prefix + '.bn.weight'].view(1, -1, 1, 1) + params[prefix + '.bn.bias'].view(1, -1, 1, 1)
        stats[prefix + '.bn.running_mean'] = 0.9 * buffers[prefix + '.bn.running_mean'] + 0.1 * mean.detach()
        stats[prefix + '.bn.running_var'] = 0.9 * buffers[prefix + '.bn.running_var'] + 0.1 * var.detach() * n / (n - 1)
        if prefix in drops:
            y = y * drops[prefix].double() / (1.0 - p_drop)
        return y
    x = layer('conv1', x, 1)
    for i, ds in enumerate(dilations):
        for j, d in enumerate(ds):
            p = 'blocks.block%d.denselayer%d' % (i + 1, j + 1)
            if p + '.conv.conv.weight' in params:
                out = layer(p + '.conv', x, d)
            else:
                out = layer(p + '.conv2', layer(p + '.conv1', x, 1), d)
            x = torch.cat([x, out], 1)
        x = layer('blocks.trans%d' % (i + 1), x, 1)
    return _conv(x, params['conv2.weight'], 1, gen), stats


def step(sd, x, dilations, signs, drops, p_drop, loss_fn, perturb=None):
    """one forward + loss + backward from the state dict `sd`: dict(logits, loss, grads {parameter name: fp64}, stats)"""
    params = {k: v.detach().double().clone().requires_grad_(True) for k, v in sd.items() if k.endswith(('.weight', '.bias'))}
    buffers = {k: v.detach().double() for k, v in sd.items() if 'running_' in k}
    logits, stats = forward(params, buffers, x, dilations, signs, drops, p_drop, perturb)
    loss = loss_fn(logits)
    loss.backward()
    return dict(logits=logits.detach(), loss=loss.detach(), grads={k: p.grad for k, p in params.items()}, stats=stats)


def tensors(res):
    """the compared quantities of a step by name"""
    out = {'logits': res['logits'], 'loss': res['loss'].reshape(1)}
    out.update({'grad ' + k: v for k, v in res['grads'].items()})
    out.update(res['stats'])
    return out


def envelope(sd, x, dilations, signs, drops, p_drop, loss_fn, seeds, clean=None):
    """per compared tensor max |perturbed - clean| / max |clean| over the seeds; returns (clean step, {name: envelope})"""
    clean = clean or step(sd, x, dilations, signs, drops, p_drop, loss_fn)
    ct = tensors(clean)
    env = {k: 0.0 for k in ct}
    for s in seeds:
        pt = tensors(step(sd, x, dilations, signs, drops, p_drop, loss_fn, perturb=torch.Generator().manual_seed(s)))
        for k in ct:
            env[k] = max(env[k], float((pt[k] - ct[k]).abs().max()) / float(ct[k].abs().max()))
    return clean, env


# the one-step cases of tests/test_gpu_fullnet_train.py: name -> (FullNet arguments, dilations per block, input shape)
CASES = {
    'small-p0': (dict(color_channels=3, output_channels=3, n_layers=4, growth_rate=8, dilations=(1, 2, 8), drop_rate=0.0),
                 ((1, 1, 1, 1), (1, 2, 3, 2), (3, 7, 10, 13)), (2, 3, 24, 20)),
    'small-p0.1': (dict(color_channels=3, output_channels=3, n_layers=4, growth_rate=8, dilations=(1, 2, 8), drop_rate=0.1),
                   ((1, 1, 1, 1), (1, 2, 3, 2), (3, 7, 10, 13)), (2, 3, 24, 20)),
    'default': (dict(color_channels=3, output_channels=3),
                ((1, 1, 1, 1, 1, 1), (1, 2, 3, 1, 2, 3), (1, 2, 3, 5, 6, 7), (2, 5, 7, 9, 11, 14), (10, 13, 16, 17, 19, 21), (1, 2, 3, 5, 6, 7),
                 (1, 1, 1, 1, 1, 1)), (2, 3, 40, 36)),
    'bottleneck': (dict(color_channels=3, output_channels=3, n_layers=4, growth_rate=8, dilations=(1, 2), layer_type='bottleneck'),
                   ((1, 1, 1, 1), (1, 2, 3, 2)), (1, 3, 24, 20)),
}
ENVELOPE_SEEDS = tuple(range(1, 9))       # 8: with 4 a fifth seed left 1.5 envelopes on the CPU (tools/fullnet_train_envelope.py)


def batch(shape, seed):
    """(x f32 [N,3,H,W], label u8 [N,H,W] in {0,1,2}, weight map u8 [N,H,W] in [1, 60])"""
    g = torch.Generator().manual_seed(seed)
    n, _, h, w = shape
    x = torch.randn(shape, generator=g)
    label = torch.randint(0, 3, (n, h, w), generator=g).to(torch.uint8)
    weight = torch.randint(1, 61, (n, h, w), generator=g).to(torch.uint8)
    return x, label, weight
