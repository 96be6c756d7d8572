"""fp64 mirror of FCN_pooling (reference models/FullNet.py:141-193) on plain functional PyTorch: FullNet's mirrors (tests/_fullnet_ref.py
for eval, tests/_fullnet_train_ref.py for train()) with F.max_pool2d(2, 2) behind trans1..trans4 and
F.interpolate(scale_factor=4, mode='bilinear', align_corners=True) behind trans5 and trans6.  The convolution, the noise model and the
compared-tensor list are imported from those two files; only the walk over the blocks (and, in training, the BatchNorm lines that
_fullnet_train_ref keeps inside its forward) is written here.

Training: like the LeakyReLU signs, the pools' arg-max positions are INPUTS - pooled = gather(windows, index).  A free arg-max moves a
gradient discontinuously when a perturbation swaps two near-equal window elements; with the indices held, the mirror and every perturbed
copy of it route the gradient as the device did.  Without given indices (CPU studies) the mirror records those of its own clean forward
(the first maximum in raster order, index 2 dy + dx)."""
import torch
import torch.nn.functional as F

import _fullnet_ref as fr
import _fullnet_train_ref as tr

POOL_AFTER, UP_AFTER = (1, 2, 3, 4), (5, 6)              # transition numbers (1-based) with a pool / an upsampling behind them

GOLDEN = dict(color_channels=3, output_channels=3, n_layers=4, growth_rate=4, dilations=(1, 2, 4, 8, 16, 4, 1))
GOLDEN_DILATIONS = ((1, 1, 1, 1), (1, 2, 3, 2), (1, 2, 5, 9), (3, 7, 10, 13), (13, 15, 17, 19), (1, 2, 5, 9), (1, 1, 1, 1))
GOLDEN_SHAPE = (2, 3, 32, 48)


def _split(flat, keys, shapes):
    out, at = {}, 0
    for k, shp in zip(keys, shapes):
        shape = tuple(int(d) for d in str(shp).split(',') if d)
        n = 1
        for d in shape:
            n *= d
        out[str(k)] = torch.from_numpy(flat[at:at + n].copy()).view(shape)
        at += n
    assert at == flat.size
    return out


def golden_state(g):
    """the state dict of tests/golden/fcn_pooling.npz (one flat f32 array there; num_batches_tracked back to int64)"""
    sd = _split(g['small/w'], g['small/keys'], g['small/shapes'])
    return {k: v.long() if k.endswith('num_batches_tracked') else v for k, v in sd.items()}


def golden_grads(g):
    """{parameter name: fp64 gradient} of the fixture's training step"""
    shapes = dict(zip((str(k) for k in g['small/keys']), g['small/shapes']))
    keys = [str(k) for k in g['small/grad_keys']]
    return _split(g['small/grads'], keys, [shapes[k] for k in keys])


def upsample4(x):
    return F.interpolate(x, scale_factor=4, mode='bilinear', align_corners=True)


def forward(sd, x, dilations, dtype=torch.float64, quant=None):
    """eval logits [N,K,H,W]; quant as in _fullnet_ref.forward, also applied to the upsampled maps (stored in the activation type; a pooled
    value is one of its inputs and needs no rounding)"""
    quant = quant or (lambda t: t)
    sd = {k: v.detach().cpu() for k, v in sd.items()}
    x = fr._conv_layer(sd, 'conv1', x.to(dtype), 1, quant)
    for i, ds in enumerate(dilations):
        for j, d in enumerate(ds):
            p = 'blocks.block%d.denselayer%d' % (i + 1, j + 1)
            if p + '.conv.conv.weight' in sd:
                out = fr._conv_layer(sd, p + '.conv', x, d, quant)
            else:
                out = fr._conv_layer(sd, p + '.conv2', fr._conv_layer(sd, p + '.conv1', x, 1, quant), d, quant)
            x = torch.cat([x, out], 1)
        x = fr._conv_layer(sd, 'blocks.trans%d' % (i + 1), x, 1, quant)
        if i + 1 in POOL_AFTER:
            x = F.max_pool2d(x, 2, 2)
        elif i + 1 in UP_AFTER:
            x = quant(upsample4(x))
    return F.conv2d(x, quant(sd['conv2.weight'].to(dtype)), padding=1)


def windows(x):
    """[N,C,H,W] -> [N,C,H/2,W/2,4], the 2x2 windows in raster order"""
    n, c, h, w = x.shape
    return x.reshape(n, c, h // 2, 2, w // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, h // 2, w // 2, 4)


def pool_by_index(x, index):
    return windows(x).gather(4, index.long().unsqueeze(4)).squeeze(4)


def train_forward(params, buffers, x, dilations, signs, drops, p_drop, pools, perturb=None):
    """_fullnet_train_ref.forward with the resampling steps.  pools: {'blocks.pool<i>': index [N,C,h/2,w/2] in 0..3}; a missing entry is
    recorded from this forward.  Returns (logits, running statistics after this forward)."""
    gen = perturb
    stats = {}
    x = x.double()
    if gen is not None:
        x = tr._noise(x, gen)

    def layer(prefix, x, d):                       # (the lines of _fullnet_train_ref.forward's `layer`, which is local to that function)
        c = tr._conv(x, params[prefix + '.conv.weight'], d, gen)
        if prefix not in signs:
            signs[prefix] = c.detach() > 0
        z = c * (0.01 + 0.99 * signs[prefix].double())         # (slope 0.01 in fp64: the reference class's own, to 1e-16)
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
        if i + 1 in POOL_AFTER:
            name = 'blocks.pool%d' % (i + 1)
            if name not in pools:
                pools[name] = windows(x.detach()).argmax(4)
            x = pool_by_index(x, pools[name])
        elif i + 1 in UP_AFTER:
            x = upsample4(x)
    return tr._conv(x, params['conv2.weight'], 1, gen), stats


def step(sd, x, dilations, signs, drops, p_drop, pools, loss_fn, perturb=None):
    params = {k: v.detach().double().clone().requires_grad_(True) for k, v in sd.items() if k.endswith(('.weight', '.bias'))}
    buffers = {k: v.detach().double() for k, v in sd.items() if 'running_' in k}
    logits, stats = train_forward(params, buffers, x, dilations, signs, drops, p_drop, pools, perturb)
    loss = loss_fn(logits)
    loss.backward()
    return dict(logits=logits.detach(), loss=loss.detach(), grads={k: p.grad for k, p in params.items()}, stats=stats)


def envelope(sd, x, dilations, signs, drops, p_drop, pools, loss_fn, seeds, clean=None):
    """_fullnet_train_ref.envelope for this network: (clean step, {compared tensor: max over the seeds of |perturbed - clean| / max|clean|})"""
    clean = clean or step(sd, x, dilations, signs, drops, p_drop, pools, loss_fn)
    ct = tr.tensors(clean)
    env = {k: 0.0 for k in ct}
    for s in seeds:
        pt = tr.tensors(step(sd, x, dilations, signs, drops, p_drop, pools, loss_fn, perturb=torch.Generator().manual_seed(s)))
        for k in ct:
            env[k] = max(env[k], float((pt[k] - ct[k]).abs().max()) / float(ct[k].abs().max()))
    return clean, env


# the one-step cases of tests/test_gpu_fcn_pooling.py: name -> (FCN_pooling arguments, dilations per block, input shape)
CASES = {
    'golden-p0': (dict(GOLDEN, drop_rate=0.0), GOLDEN_DILATIONS, GOLDEN_SHAPE),
    'golden-p0.1': (dict(GOLDEN, drop_rate=0.1), GOLDEN_DILATIONS, GOLDEN_SHAPE),
    'default': (dict(color_channels=3, output_channels=3), fr.DEFAULT_DILATIONS, (2, 3, 32, 32)),
    'bottleneck': (dict(GOLDEN, layer_type='bottleneck'), GOLDEN_DILATIONS, (2, 3, 32, 32)),
}
# seeds of the envelope per case (tools/fullnet_train_envelope.py --net FCN_pooling): with FullNet's 8 an independent
# ninth draw reached 2.4 / 3.2 / 1.2 / 2.0 envelopes (BatchNorm over the 12 - 32 values of the pooled maps amplifies a 2^-16 error a few
# hundred times, and the tails are long), beyond the 1.5 asked for; with 32 three independent draws stay within 1.65 on the small networks,
# with 16 within 1.16 on the default one
ENVELOPE_SEEDS = {'golden-p0': tuple(range(1, 33)), 'golden-p0.1': tuple(range(1, 33)), 'default': tuple(range(1, 17)),
                  'bottleneck': tuple(range(1, 33))}
