"""One-channel models (in_c = 1) on the MI355X, both precision modes.

Exactness by embedding.  A one-channel model with stem weights w [Cout, 1, 3, 3] and bias b computes, bit for bit, what the
three-channel model with stem cat(w, 0, 0) and bias b computes on cat(x, 0, 0): the one-channel stem runs on the zero-extended pack of
the RGB stem (1 -> 16 reduction channels where RGB has 3 -> 16), so both launches see the same operands.  Checked for the eval logits of
the Unet family, the plain UNet and FullNet, for one training step (losses, every gradient) and five Adam steps of UNet_vgg16 and
UNet2RevA1_vgg16, with encoder_freeze, for window batches (forward_packed) and for pipeline.infer_image with sliding windows and TTA.

One anchor outside the kernels: the eval logits of the one-channel UNet_vgg16 against the plain-PyTorch CPU mirror that applies child0 in
place of backbone child '0' (tests/_grey_ref.py).  Bars: those of tests/test_gpu_backbone_unet.py - fp32 mode 5e-4 of the output scale;
bf16 mode tests/test_gpu_model.py: _check (max <= 3e-2, mean <= 6e-3 of the scale, arg-max agreement >= 0.99).  Before they were taken over,
the envelope was measured on the CPU as that file did: the mirror with the 16-bit path's rounding points (_grey_ref.eval_rounded_forward
in fp64) against the fp64 mirror, det_fill weights, the two inputs of this test:
    (2, 1, 48, 64) seed 41:  max 3.86e-3, mean 7.19e-4 of the scale (12.16), arg-max agreement 1.0
    (1, 1, 40, 56) seed 42:  max 3.46e-3, mean 7.01e-4 of the scale (12.44), arg-max agreement 1.0
(random_model(3) weights: max 3.88e-3 / 3.69e-3, mean 7.69e-4 / 7.84e-4.)  The rule: a bar the envelope alone exceeds becomes twice the
measured envelope.  None does, so the bars stand.  fp32 mode: the fp32 mirror is within 5.2e-7 of the fp64 one."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SHAPES = (((2, 1, 48, 64), 41), ((1, 1, 40, 56), 42))


@pytest.fixture(params=['fp32', 'bf16'])
def precision(request):
    import cdnet_amd
    before = cdnet_amd.get_precision()
    cdnet_amd.set_precision(request.param)
    yield request.param
    cdnet_amd.set_precision(before)


def _rgb(x):
    import torch
    return torch.cat([x, torch.zeros_like(x), torch.zeros_like(x)], 1)


def _embed_state(sd1, stem, grey_stem=None):
    """the three-channel state dict of a one-channel one: `stem` (.weight / .bias) = cat(w, 0, 0), b of `grey_stem` (default: itself)"""
    import torch
    sd = {k: v.clone() for k, v in sd1.items()}
    g = grey_stem or stem
    w = sd1[g + '.weight']
    assert w.shape[1] == 1
    sd[stem + '.weight'] = torch.cat([w, torch.zeros_like(w), torch.zeros_like(w)], 1)
    sd[stem + '.bias'] = sd1[g + '.bias'].clone()
    return sd


def _bn_spread(m, seed):
    """well-conditioned BatchNorm parameters and statistics, so that the eval logits are not a constant"""
    import torch
    g = torch.Generator().manual_seed(seed)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            with torch.no_grad():
                mod.weight.copy_(0.5 + torch.rand(mod.weight.shape, generator=g))
                mod.bias.copy_(0.2 * torch.randn(mod.bias.shape, generator=g))
                mod.running_mean.copy_(0.1 * torch.randn(mod.running_mean.shape, generator=g))
                mod.running_var.copy_(0.5 + torch.rand(mod.running_var.shape, generator=g))
    return m


def _unet_family_pair(name, seed=0, freeze=False):
    """(one-channel model, embedded three-channel model) of a Unet-family name, on the device"""
    import importlib
    import torch
    torch.manual_seed(seed)
    if name == 'UNet2RevA1_vgg16':
        from cdnet_amd.models.dam.model_unet_rev1 import Unet
    elif name == 'UNet_vgg16':
        from cdnet_amd.models.model_unet import Unet
    else:
        Unet = importlib.import_module('cdnet_amd.models.dam.' + name).Unet
    m1 = _bn_spread(Unet(backbone_name='vgg16_bn', pretrained=False, encoder_freeze=freeze, classes=3), seed + 100)
    m1.set_input_channels(1)
    m3 = Unet(backbone_name='vgg16_bn', pretrained=False, classes=3)
    assert list(m1.state_dict().keys()) == list(m3.state_dict().keys())
    m3.load_state_dict(_embed_state(m1.state_dict(), 'backbone.0', 'child0'))
    return m1.cuda(), m3.cuda()


def _same_bits(a, b, what):
    a, b = a.detach().float().cpu().numpy(), b.detach().float().cpu().numpy()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (what, int((a.view(np.uint32) != b.view(np.uint32)).sum()), float(np.abs(a - b).max()))


def _inputs():
    import torch
    from cdnet_amd import synth
    return [torch.from_numpy(synth.det_input(shape, seed)).cuda() for shape, seed in SHAPES]


@pytest.mark.parametrize('name', ['UNet2RevA1_vgg16', 'UNet_vgg16', 'model_unet_MandDandP'])
def test_eval_logits_equal_the_embedded_model(precision, name):
    import torch
    m1, m3 = _unet_family_pair(name, seed=2)
    m1.eval(), m3.eval()
    for x in _inputs():
        with torch.no_grad():
            got, want = m1(x), m3(_rgb(x))
        got, want = (got, want) if isinstance(got, tuple) else ((got,), (want,))
        assert len(got) == (1 if name == 'UNet_vgg16' else 3)
        for k, (a, b) in enumerate(zip(got, want)):
            assert a.shape[0] == x.shape[0] and tuple(a.shape[2:]) == tuple(x.shape[2:]) and float(a.std()) > 0
            _same_bits(a, b, (name, k, tuple(x.shape)))
    # eval mode without a trainer follows the input's channel count, as the reference does; a training forward never switches
    with torch.no_grad():
        y3 = m1(_rgb(_inputs()[1]))
    assert m1.input_channels == 3 and m1.UNUSED_PREFIXES == type(m1).UNUSED_PREFIXES
    m1.train()
    with pytest.raises(ValueError, match='channels'):
        m1(_inputs()[1])
    assert torch.is_tensor(y3) or len(y3) == 3


def test_eval_logits_plain_unet_and_fullnet(precision):
    import torch
    from _fullnet_train_ref import CASES
    from cdnet_amd.models.FullNet import FullNet
    from cdnet_amd.models.unet import UNet
    torch.manual_seed(3)
    pairs = []
    u1 = _bn_spread(UNet(3, in_channels=1), 7)
    u3 = UNet(3, in_channels=3)
    u3.load_state_dict(_embed_state(u1.state_dict(), 'down1.down_conv.0'))
    pairs.append(('UNet', u1, u3))
    kw = dict(CASES['small-p0'][0])
    kw.pop('color_channels'), kw.pop('output_channels')
    f1 = _bn_spread(FullNet(1, 3, **kw), 8)
    f3 = FullNet(3, 3, **kw)
    sd = {k: v.clone() for k, v in f1.state_dict().items()}
    w = sd['conv1.conv.weight']                                      # the stem: Conv2d(1, 24, 3, padding=1, bias=False)
    assert w.shape[1] == 1
    sd['conv1.conv.weight'] = torch.cat([w, torch.zeros_like(w), torch.zeros_like(w)], 1)
    f3.load_state_dict(sd)
    pairs.append(('FullNet', f1, f3))
    for name, m1, m3 in pairs:
        m1, m3 = m1.cuda().eval(), m3.cuda().eval()
        for x in _inputs():
            with torch.no_grad():
                got, want = m1(x), m3(_rgb(x))
            assert tuple(got.shape) == (x.shape[0], 3) + tuple(x.shape[2:]) and float(got.std()) > 0
            _same_bits(got, want, (name, tuple(x.shape)))


def _batch(B=2, S=64):
    import torch
    from cdnet_amd import synth
    lab, dirn, point, weight = synth.train_targets(B, S, S, 31)
    x = torch.from_numpy(synth.det_input((B, 1, S, S), 12))
    return [t.cuda() for t in (x, torch.from_numpy(lab), torch.from_numpy(dirn), torch.from_numpy(point), torch.from_numpy(weight)[:, 0].contiguous())]


def _trainer(name, m):
    from cdnet_amd import trainer
    return trainer.Trainer(m) if name == 'UNet2RevA1_vgg16' else trainer.BackboneUNetTrainer(m)


def _backward(name, tr, x, batch):
    """forward, loss and backward of one step (no optimiser step) -> the loss values"""
    import torch
    _, lab, dirn, point, weight = batch
    if name == 'UNet2RevA1_vgg16':
        out = tr.forward(x)
        tr.backward(*tr.loss_and_grads(*out, lab, dirn, point, weight))
        losses = tr.losses
    else:
        tr.backward(tr.loss_and_grads(tr.forward(x), lab, weight))
        losses = tr.mask_losses
    torch.cuda.synchronize()
    return losses.detach().cpu().clone()


def _steps(name, tr, x, batch, n=5):
    _, lab, dirn, point, weight = batch
    out = []
    for _ in range(n):
        r = tr.train_step(x, lab, dirn, point, weight) if name == 'UNet2RevA1_vgg16' else tr.train_step(x, lab, weight)
        out.append(r.detach().cpu().clone())
    return out


@pytest.mark.parametrize('name', ['UNet_vgg16', 'UNet2RevA1_vgg16'])
def test_training_step_equals_the_embedded_model(precision, name):
    import torch
    batch = _batch()
    x = batch[0]
    m1, m3 = _unet_family_pair(name, seed=5)
    p0 = {n: p.detach().cpu().clone() for n, p in m1.named_parameters()}
    t1, t3 = _trainer(name, m1), _trainer(name, m3)
    with pytest.raises(RuntimeError, match='trainer'):
        m1.set_input_channels(3)                                   # the trainer laid out its buffers for child0: the rule of freeze_encoder
    with pytest.raises(ValueError, match='channels'):
        t1.forward(_rgb(x))                                        # a training input of another channel count
    l1, l3 = _backward(name, t1, x, batch), _backward(name, t3, _rgb(x), batch)
    assert np.isfinite(l1.numpy()).all() and float(l1[0]) > 0
    _same_bits(l1, l3, 'losses')
    g1 = {n: p.grad.detach().clone() for n, p in m1.named_parameters()}
    g3 = {n: p.grad.detach().clone() for n, p in m3.named_parameters()}
    _same_bits(g1['child0.weight'], g3['backbone.0.weight'][:, :1].contiguous(), 'child0.weight.grad')
    _same_bits(g1['child0.bias'], g3['backbone.0.bias'], 'child0.bias.grad')
    assert float(g1['child0.weight'].abs().max()) > 0
    assert float(g3['backbone.0.weight'][:, 1:].abs().max()) == 0.0   # the zero planes of the embedded input
    for n in g1:
        if n.startswith(('child0.', 'backbone.0.')):
            continue
        _same_bits(g1[n], g3[n], n + '.grad')
    # backbone.0.* takes no part: no gradient, and five Adam steps leave it alone while child0.* moves (the reference's behaviour)
    assert float(g1['backbone.0.weight'].abs().max()) == 0.0 and float(g1['backbone.0.bias'].abs().max()) == 0.0
    s1, s3 = _steps(name, t1, x, batch), _steps(name, t3, _rgb(x), batch)
    for k, (a, b) in enumerate(zip(s1, s3)):
        _same_bits(a, b, ('loss of step', k))
    sd = {n: p.detach().cpu() for n, p in m1.named_parameters()}
    for n in ('backbone.0.weight', 'backbone.0.bias', 'child_conv1.weight'):
        assert torch.equal(sd[n], p0[n]), n
    for n in ('child0.weight', 'child0.bias', 'backbone.1.weight', 'backbone.3.weight'):
        assert not torch.equal(sd[n], p0[n]), n
    e3 = {n: p.detach().cpu() for n, p in m3.named_parameters()}
    _same_bits(sd['child0.weight'], e3['backbone.0.weight'][:, :1].contiguous(), 'child0.weight after five steps')
    _same_bits(sd['child0.bias'], e3['backbone.0.bias'], 'child0.bias after five steps')
    assert float(e3['backbone.0.weight'][:, 1:].abs().max()) == 0.0


@pytest.mark.parametrize('name', ['UNet_vgg16', 'UNet2RevA1_vgg16'])
def test_encoder_freeze_keeps_child0_training(precision, name):
    """encoder_freeze freezes backbone.* only (the reference's rule): the losses and every trainable parameter's gradient are those of the
    embedded model (which is not frozen: a frozen three-channel stem gets no gradient to compare with), and child0.* still moves"""
    import torch
    batch = _batch()
    x = batch[0]
    m1, m3 = _unet_family_pair(name, seed=6, freeze=True)
    assert m1.child0.weight.requires_grad and not m1.backbone[0].weight.requires_grad and not m1.backbone[40].weight.requires_grad
    p0 = {n: p.detach().cpu().clone() for n, p in m1.named_parameters()}
    rm0 = m1.backbone[1].running_mean.detach().cpu().clone()
    t1, t3 = _trainer(name, m1), _trainer(name, m3)
    l1, l3 = _backward(name, t1, x, batch), _backward(name, t3, _rgb(x), batch)
    _same_bits(l1, l3, 'losses')
    g1 = {n: p.grad.detach().clone() for n, p in m1.named_parameters()}
    g3 = {n: p.grad.detach().clone() for n, p in m3.named_parameters()}
    _same_bits(g1['child0.weight'], g3['backbone.0.weight'][:, :1].contiguous(), 'child0.weight.grad')
    _same_bits(g1['child0.bias'], g3['backbone.0.bias'], 'child0.bias.grad')
    for n in g1:
        if not n.startswith(('child0.', 'backbone.')):
            _same_bits(g1[n], g3[n], n + '.grad')
    assert float(g1['backbone.0.weight'].abs().max()) == 0.0
    losses = _steps(name, t1, x, batch)
    assert all(np.isfinite(v.numpy()).all() for v in losses)
    sd = {n: p.detach().cpu() for n, p in m1.named_parameters()}
    for n in p0:
        if n.startswith('backbone.') or n.startswith('child_conv1.'):
            assert torch.equal(sd[n], p0[n]), n                    # frozen (or never used): no step
    for n in ('child0.weight', 'child0.bias', 'upsample_blocks.0.up.weight'):
        assert not torch.equal(sd[n], p0[n]), n
    assert not torch.equal(m1.backbone[1].running_mean.cpu(), rm0)  # the frozen BatchNorm layers still track their statistics


@pytest.mark.parametrize('name', ['UNet2RevA1_vgg16', 'UNet_vgg16'])
def test_forward_packed_windows_do_not_depend_on_their_batch(precision, name):
    import torch
    from cdnet_amd import runtime, synth
    m1, _ = _unet_family_pair(name, seed=3)
    m1.eval()
    x = torch.from_numpy(synth.det_input((5, 1, 48, 64), 7)).cuda()
    with torch.no_grad():
        x16 = runtime.input_pack(x)
        assert tuple(x16.shape) == (5, 48, 64, 16) and float(x16[..., 1:].float().abs().max()) == 0.0
        out = m1.forward_packed(x16)
        whole = m1(x)
        whole = whole if isinstance(whole, tuple) else (whole,)
        for a, b in zip(out, whole):
            _same_bits(a, b, 'forward_packed vs forward')
        for i in range(5):
            one = m1.forward_packed(x16[i:i + 1].contiguous())
            for k, (a, b) in enumerate(zip(one, out)):
                _same_bits(a, b[i:i + 1], (i, k))


def test_infer_image_windows_and_tta_equal_the_embedded_model(precision):
    import torch
    from cdnet_amd import pipeline, synth
    m1, m3 = _unet_family_pair('UNet2RevA1_vgg16', seed=1)
    m1.eval(), m3.eval()
    img = torch.from_numpy(synth.det_input((1, 100, 90), 8)).cuda()
    kw = dict(tta=True, all_img_test=0, patch_size=64, overlap=16, want_stages=True)
    r1 = pipeline.infer_image(m1, img, **kw)
    r3 = pipeline.infer_image(m3, _rgb(img[None])[0].contiguous(), **kw)
    assert tuple(r1['final'].shape) == (100, 90)
    for k in ('pred', 'final'):
        assert torch.equal(r1[k], r3[k]), k
    assert r1['count'] == r3['count']
    _same_bits(r1['prob_mean'], r3['prob_mean'], 'prob_mean')


def test_eval_logits_against_the_cpu_mirror(precision):
    """the anchor outside the kernels: UNet_vgg16 with the one-channel stem against plain PyTorch (tests/_grey_ref.py)"""
    import torch
    import _grey_ref as gr
    from cdnet_amd import synth
    from cdnet_amd.models.model_unet import Unet
    from test_gpu_model import _check
    ref = gr.det_model().eval()
    m = Unet(backbone_name='vgg16_bn', pretrained=False, classes=3)
    assert list(m.state_dict().keys()) == list(ref.state_dict().keys())
    m.load_state_dict(ref.state_dict())
    m.set_input_channels(1)
    m = m.cuda().eval()
    for shape, seed in SHAPES:
        x = torch.from_numpy(synth.det_input(shape, seed))
        with torch.no_grad():
            want = ref(x).numpy()
            got = m(x.cuda())
        assert tuple(got.shape) == want.shape and got.dtype == torch.float32
        scale = np.abs(want).max()
        err = np.abs(got.cpu().numpy() - want)
        print('one-channel UNet_vgg16 eval %s %s: max %.3g mean %.3g of the scale %.3g, arg-max agreement %.4f'
              % (precision, shape, err.max() / scale, err.mean() / scale, scale, (got.cpu().numpy().argmax(1) == want.argmax(1)).mean()))
        if precision == 'bf16':
            _check(got, want, 'one-channel UNet_vgg16 eval %s' % (shape,))
        else:
            assert err.max() <= 5e-4 * scale, (err.max(), scale)


def test_grey_transformed_on_the_device_is_pillows_convert_l():
    """what pipeline.infer_image makes of a true-colour image the test_dam entry read as RGB, on device tensors: the bits of loading the
    file with convert('L'), with and without `normalize`; infer_image on the three-plane image gives the label maps of the L image"""
    import torch
    from PIL import Image
    from cdnet_amd import pipeline
    from cdnet_amd.options import Options
    rs = np.random.RandomState(3)
    rgb = Image.fromarray(rs.randint(0, 256, (70, 61, 3)).astype(np.uint8))
    opt = Options(isTrain=False).parse(['--dataset', 'BBBC039V1', '--patch-size', '64', '--overlap', '16'])
    opt.all_img_test = 0
    for norm in (None, [[0.7, 0.5, 0.6], [0.2, 0.25, 0.3]]):
        if norm:
            opt.transform['test']['normalize'] = norm
        x3 = pipeline.host_input(rgb, opt.transform['test'], 3).cuda()
        x1 = pipeline.host_input(rgb, opt.transform['test'], 1).cuda()
        _same_bits(pipeline.grey_transformed(x3, opt), x1, ('grey_transformed', norm))
    m1, _ = _unet_family_pair('UNet2RevA1_vgg16', seed=1)
    m1.eval()
    r3, r1 = pipeline.infer_image(m1, x3, opt), pipeline.infer_image(m1, x1, opt)
    assert torch.equal(r3['final'], r1['final']) and torch.equal(r3['pred'], r1['pred']) and r3['count'] == r1['count']
