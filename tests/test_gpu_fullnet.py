"""FullNet on the device against the fp64 mirror (tests/_fullnet_ref.py), both precisions.

Errors are max|got - mirror| / max|mirror logit|.  The envelopes are CPU quantities that do not depend on the code under test:
  fp32 mode: E = the mirror's own change when every weight is perturbed by a relative 2^-16 U(-1, 1) (the size of a split-product error;
             the rule and the factor 3 of tests/test_gpu_fp32.py's perturbed-oracle test);
  bf16 mode: E_bf16 = the distance between the fp64 mirror and the same mirror with the convolution weights and every stored layer output
             rounded to bf16.
The device must stay within 3 E."""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(params=['fp32', 'bf16'])
def precision(request):
    import cdnet_amd
    before = cdnet_amd.get_precision()
    cdnet_amd.set_precision(request.param)
    yield request.param
    cdnet_amd.set_precision(before)


def _model(kw, seed):
    import _fullnet_ref as fr
    from cdnet_amd.models.FullNet import FullNet
    return fr.randomize(FullNet(**kw), seed).eval()


@functools.lru_cache(maxsize=None)
def _default_case():
    """the default network, its input and the CPU quantities (computed once, shared, never modified)"""
    import torch
    import _fullnet_ref as fr
    m = _model(dict(color_channels=3, output_channels=3), 21)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    x = fr.bf16_exact_input((2, 3, 40, 36), 22)
    want = fr.forward(sd, x, fr.DEFAULT_DILATIONS)
    sdp = fr.perturbed(sd, 23)
    scale = float(want.abs().max())
    E = float((fr.forward(sdp, x, fr.DEFAULT_DILATIONS) - want).abs().max()) / scale
    E16 = float((fr.forward(sd, x, fr.DEFAULT_DILATIONS, quant=fr.bf16_round) - want).abs().max()) / scale
    return m, x, want, scale, E, E16


def test_default_network_within_three_envelopes(precision):
    import torch
    m, x, want, scale, E, E16 = _default_case()
    with torch.no_grad():
        got = m.cuda()(x.cuda()).cpu().double()
    assert got.shape == want.shape == (2, 3, 40, 36) and bool(torch.isfinite(got).all())
    err = float((got - want).abs().max()) / scale
    env = E if precision == 'fp32' else E16
    agree = float((got.argmax(1) == want.argmax(1)).double().mean())
    print('FullNet default %s: err %.3e of max|logit| %.3g, envelope %.3e, ratio %.2f, arg-max agreement %.4f'
          % (precision, err, scale, env, err / env, agree))
    assert err <= 3 * env, (precision, err, env)


def test_small_golden_network(precision, golden):
    """the golden weights through the device model against the REFERENCE class's fp64 logits (not the mirror's), same envelopes on this network"""
    import torch
    import _fullnet_ref as fr
    from cdnet_amd.models.FullNet import FullNet
    g = golden('fullnet')
    sd = {str(k): torch.from_numpy(g['small/w/%d' % i]) for i, k in enumerate(g['small/keys'])}
    m = FullNet(**fr.SMALL)
    m.load_state_dict(sd, strict=True)
    x, want = torch.from_numpy(g['small/x']), torch.from_numpy(g['small/logits64'])
    scale = float(want.abs().max())
    if precision == 'fp32':
        sdp = fr.perturbed(sd, 5)
        env = float((fr.forward(sdp, x, fr.SMALL_DILATIONS) - want).abs().max()) / scale
    else:
        env = float((fr.forward(sd, x, fr.SMALL_DILATIONS, quant=fr.bf16_round) - want).abs().max()) / scale
    with torch.no_grad():
        got = m.cuda().eval()(x.cuda()).cpu().double()
    err = float((got - want).abs().max()) / scale
    print('FullNet small golden %s: err %.3e, envelope %.3e, ratio %.2f' % (precision, err, env, err / env))
    assert err <= 3 * env, (precision, err, env)


def test_bottleneck_network(precision):
    import torch
    import _fullnet_ref as fr
    m = _model(dict(color_channels=3, output_channels=2, layer_type='bottleneck'), 31)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    x = fr.bf16_exact_input((1, 3, 24, 20), 32)
    want = fr.forward(sd, x, fr.DEFAULT_DILATIONS)
    scale = float(want.abs().max())
    if precision == 'fp32':
        sdp = fr.perturbed(sd, 33)
        env = float((fr.forward(sdp, x, fr.DEFAULT_DILATIONS) - want).abs().max()) / scale
    else:
        env = float((fr.forward(sd, x, fr.DEFAULT_DILATIONS, quant=fr.bf16_round) - want).abs().max()) / scale
    with torch.no_grad():
        got = m.cuda()(x.cuda()).cpu().double()
    assert got.shape == (1, 2, 24, 20)
    err = float((got - want).abs().max()) / scale
    print('FullNet bottleneck %s: err %.3e, envelope %.3e, ratio %.2f' % (precision, err, env, err / env))
    assert err <= 3 * env, (precision, err, env)


def test_forward_packed_sub_batches_are_bit_equal(precision, monkeypatch):
    import torch
    import _fullnet_ref as fr
    from cdnet_amd import runtime
    from cdnet_amd.models import FullNet as fn
    m = _model(fr.SMALL, 41).cuda()
    x16 = runtime.input_pack(fr.bf16_exact_input((5, 3, 24, 40), 42).cuda())
    calls = []
    orig = fn.FullNet._forward_nhwc
    monkeypatch.setattr(fn.FullNet, '_forward_nhwc', lambda self, x, out: (calls.append(x.shape[0]), orig(self, x, out))[1])
    with torch.no_grad():
        one, = m.forward_packed(x16)
        assert calls == [5]
        del calls[:]
        per_window = m._channels_per_pixel() * 24 * 40 * x16.element_size()
        monkeypatch.setattr(fn, 'WORKSPACE_BYTES', 2 * per_window + per_window // 2)           # room for two windows, not three
        cut, = m.forward_packed(x16)
    assert calls == [2, 2, 1]
    assert torch.equal(one.view(torch.int32), cut.view(torch.int32))
    with torch.no_grad():
        assert torch.equal(m(fr.bf16_exact_input((5, 3, 24, 40), 42).cuda()).view(torch.int32), one.view(torch.int32))


def test_module_prefixed_checkpoint_round_trip(tmp_path):
    import torch
    import _fullnet_ref as fr
    from cdnet_amd import checkpoint
    from cdnet_amd.models.FullNet import FullNet
    a = _model(fr.SMALL, 51).cuda()
    x = fr.bf16_exact_input((1, 3, 24, 20), 52).cuda()
    with torch.no_grad():
        want = a(x)
    state = {'epoch': 3, 'state_dict': checkpoint.model_state(a), 'best_iou': 0.0, 'best_loss': 1.0, 'optimizer': None}
    assert all(k.startswith('module.') for k in state['state_dict'])
    path = str(tmp_path / 'checkpoint_best.pth.tar')
    torch.save(state, path)
    b = FullNet(**fr.SMALL).cuda().eval()
    with torch.no_grad():
        assert not torch.equal(b(x), want)                      # (other weights: the packs below must be rebuilt after the load)
    ck = checkpoint.load_checkpoint(path, b)
    assert ck['epoch'] == 3
    with torch.no_grad():
        assert torch.equal(b(x).view(torch.int32), want.view(torch.int32))
