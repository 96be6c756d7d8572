"""FullNet without a GPU: the fp64 mirror against the reference's logits, the model's state_dict layout, the factory and entry wiring,
the refused forwards, the new struct's size and every rejected argument of cdnet_dilated_conv_forward."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _small_state(g):
    import torch
    return {str(k): torch.from_numpy(g['small/w/%d' % i]) for i, k in enumerate(g['small/keys'])}


def test_mirror_reproduces_the_reference_logits(golden):
    import torch
    import _fullnet_ref as fr
    g = golden('fullnet')
    want = g['small/logits64']
    got = fr.forward(_small_state(g), torch.from_numpy(g['small/x']), fr.SMALL_DILATIONS).numpy()
    assert got.shape == want.shape == (2, 3, 40, 36)
    assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()


@pytest.mark.parametrize('layer_type', ['basic', 'bottleneck'])
def test_state_dict_layout_is_the_reference_s(golden, layer_type):
    from cdnet_amd.models.FullNet import FullNet
    g = golden('fullnet')
    m = FullNet(3, 3, layer_type=layer_type)
    sd = m.state_dict()
    assert list(sd) == [str(k) for k in g['keys_' + layer_type]]
    assert [','.join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in g['shapes_' + layer_type]]
    if layer_type == 'basic':
        assert len(sd) == 301 and sum(p.numel() for p in m.parameters()) == int(g['nparams_basic']) == 1780233


def test_initialisation_is_the_reference_s():
    import torch
    from cdnet_amd.models.FullNet import FullNet
    torch.manual_seed(3)
    m = FullNet(3, 3)
    w = m.blocks.block5.denselayer6.conv.conv.weight.detach()
    assert tuple(w.shape) == (24, 136 + 5 * 24, 3, 3)
    assert abs(float(w.std()) - np.sqrt(2.0 / (9 * 24))) < 0.05 * np.sqrt(2.0 / (9 * 24))          # normal(0, sqrt(2 / (k k out)))
    t = m.blocks.trans1.conv.weight.detach()
    assert tuple(t.shape) == (84, 168, 1, 1) and abs(float(t.std()) - np.sqrt(2.0 / 84)) < 0.05 * np.sqrt(2.0 / 84)
    assert all(float(b.weight.min()) == float(b.weight.max()) == 1 and float(b.bias.abs().max()) == 0
               for b in m.modules() if isinstance(b, torch.nn.BatchNorm2d))
    assert [c.dilation[0] for c in m.blocks.block5.modules() if isinstance(c, torch.nn.Conv2d)] == [10, 13, 16, 17, 19, 21]
    assert m.blocks.block4.denselayer6.conv.conv.padding == (14, 14)


def test_strict_load_of_the_golden_weights(golden):
    import _fullnet_ref as fr
    from cdnet_amd.models.FullNet import FullNet
    g = golden('fullnet')
    m = FullNet(**fr.SMALL)
    assert sum(p.numel() for p in m.parameters()) == 41177
    res = m.load_state_dict(_small_state(g), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert [c.dilation[0] for c in m.blocks.block3.modules() if c.__class__.__name__ == 'Conv2d'] == list(fr.SMALL_DILATIONS[2])
    assert [m.blocks.trans1.conv.out_channels, m.blocks.trans2.conv.out_channels, m.blocks.trans3.conv.out_channels] == [28, 30, 31]


def test_choose_model_and_entry_wiring():
    from cdnet_amd import test, utils
    from cdnet_amd.models.FullNet import FullNet
    from cdnet_amd.options import Options
    opt = Options(isTrain=False)
    opt.model['modelName'] = 'FullNet'
    opt.model.pop('dilations', None)
    m = utils.chooseModel(opt)
    assert isinstance(m, FullNet) and len(m.state_dict()) == 301 and m.conv2.out_channels == opt.model['out_c']
    opt.model['dilations'] = [1, 2]
    opt.model['n_layers'] = 4
    opt.model['layer_type'] = 'bottleneck'
    m = utils.chooseModel(opt)
    assert [n for n, _ in m.blocks.named_children()] == ['block1', 'trans1', 'block2', 'trans2']
    assert tuple(m.blocks.block2.denselayer3.conv2.conv.dilation) == (3, 3) and m.blocks.block2.denselayer3.conv1.conv.out_channels == 96
    opt.model['modelName'] = 'FCN_pooling'
    with pytest.raises(NotImplementedError):
        utils.chooseModel(opt)
    test.check_model_name('FullNet')
    assert 'FullNet' in test.MASK_MODELS
    with pytest.raises(ValueError):
        test.check_model_name('FCN_pooling')


def test_cpu_and_training_forwards_are_refused():
    import torch
    import _fullnet_ref as fr
    from cdnet_amd.models.FullNet import FullNet
    m = FullNet(**fr.SMALL).eval()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m(torch.zeros(1, 3, 8, 8))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m.forward_packed(torch.zeros(1, 8, 8, 16))
    m.train()
    with pytest.raises(RuntimeError, match='inference only'):
        m.forward_packed(torch.zeros(1, 8, 8, 16))


def test_struct_size_and_pack_size():
    from cdnet_amd import _lib
    lib = _lib.load()
    assert C.sizeof(_lib.DilatedConvArgs) == lib.cdnet_abi_sizeof(b'cdnet_dilated_conv_args') > 0
    # per (tap, 16-channel K step, 32-wide tile) one 64 x 8 image; K steps come in pairs (32 channels)
    assert lib.cdnet_dilated_packed_weight_elems(168, 24, 9, 0) == 9 * 12 * 1 * 512
    assert lib.cdnet_dilated_packed_weight_elems(286, 143, 1, 1) == 1 * 18 * 5 * 512 * 2
    assert lib.cdnet_dilated_packed_weight_elems(3, 24, 5, 0) == 0


def _args(**kw):
    from cdnet_amd import _lib
    a = _lib.DilatedConvArgs()
    a.in_, a.w, a.out = 0x10000, 0x20000, 0x30000            # never dereferenced: every case below is refused before any HIP call
    a.N, a.H, a.W = 1, 8, 8
    a.Cin, a.in_cstride, a.Cout, a.out_cstride, a.out_coff = 24, 48, 24, 48, 0
    a.taps, a.dilation, a.leaky, a.slope, a.f32, a.out_nchw = 9, 1, 1, 0.01, 0, 0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


BAD = {
    'null in': dict(in_=None), 'null w': dict(w=None), 'null out': dict(out=None),
    'taps 3': dict(taps=3), 'taps 0': dict(taps=0), 'dilation 0': dict(dilation=0), 'dilation -2': dict(dilation=-2),
    'N 0': dict(N=0), 'H 0': dict(H=0), 'W -1': dict(W=-1), 'Cin 0': dict(Cin=0), 'Cout 0': dict(Cout=0),
    'in stride < Cin': dict(Cin=56), 'in stride not 8': dict(in_cstride=28), 'out stride < Cout': dict(out_cstride=16),
    'out slice past stride': dict(out_coff=32), 'negative out_coff': dict(out_coff=-8),
    'in place overlap': dict(out=0x10000, out_coff=16), 'in place overlap at 0': dict(out=0x10000),
    'in place strides differ': dict(out=0x10000, out_coff=24, out_cstride=56),
    'nchw in place': dict(out=0x10000, out_nchw=1), 'nchw with out_coff': dict(out_nchw=1, out_coff=8),
}


@pytest.mark.parametrize('case', sorted(BAD))
def test_rejected_arguments(case):
    from cdnet_amd import _lib
    lib = _lib.load()
    rc = lib.cdnet_dilated_conv_forward(C.byref(_args(**BAD[case])), None)
    assert rc == 1, case                                       # CDNET_E_ARG
    assert b'cdnet_dilated_conv_forward' in lib.cdnet_last_error()


def test_rejected_pack_arguments():
    from cdnet_amd import _lib
    lib = _lib.load()
    assert lib.cdnet_dilated_conv_forward(None, None) == 1
    assert lib.cdnet_dilated_pack_weights(None, 0x1000, 3, 24, 9, 0, None) == 1
    assert lib.cdnet_dilated_pack_weights(0x1000, 0x2000, 0, 24, 9, 0, None) == 1
    assert lib.cdnet_dilated_pack_weights(0x1000, 0x2000, 3, 24, 4, 0, None) == 1
    assert b'cdnet_dilated_pack_weights' in lib.cdnet_last_error()
