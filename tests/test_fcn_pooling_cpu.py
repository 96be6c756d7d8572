"""FCN_pooling without a GPU: the fp64 mirror (tests/_fcn_pooling_ref.py) against the reference class's eval logits and its training
step (tests/golden/fcn_pooling.npz), the model's state_dict layout and children, the refused forwards and every rejected argument of the
four resampling entries (csrc/resample.hip)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _rel(got, want):
    return float(np.abs(np.asarray(got) - np.asarray(want)).max()) / float(np.abs(np.asarray(want)).max())


def test_mirror_reproduces_the_reference_eval_logits(golden):
    import torch
    import _fcn_pooling_ref as pr
    g = golden('fcn_pooling')
    want = g['small/logits64']
    got = pr.forward(pr.golden_state(g), torch.from_numpy(g['small/x']), pr.GOLDEN_DILATIONS).numpy()
    assert got.shape == want.shape == (2, 3, 32, 48)
    assert _rel(got, want) <= 1e-10


def test_mirror_reproduces_the_reference_training_step(golden):
    """drop_rate 0 in train(): logits, loss and every parameter's gradient; the pools' indices are those of the mirror's own forward"""
    import torch
    import _fcn_pooling_ref as pr
    from oracle import train as ot
    g = golden('fcn_pooling')
    label, weight = torch.from_numpy(g['small/label']), torch.from_numpy(g['small/weight'])
    pools = {}
    res = pr.step(pr.golden_state(g), torch.from_numpy(g['small/x']), pr.GOLDEN_DILATIONS, {}, {}, 0.0, pools,
                  lambda lg: ot.unet_losses(lg, label, weight)['total'])
    assert sorted(pools) == ['blocks.pool1', 'blocks.pool2', 'blocks.pool3', 'blocks.pool4']
    assert tuple(pools['blocks.pool4'].shape) == (2, 16, 2, 3)
    assert _rel(res['logits'].numpy(), g['small/train_logits64']) <= 1e-10
    assert _rel(res['loss'].numpy().reshape(1), g['small/train_loss64']) <= 1e-10
    want = pr.golden_grads(g)
    assert sorted(want) == sorted(res['grads']) and len(want) == 109
    for k, w in want.items():
        assert res['grads'][k].shape == w.shape, k
        assert _rel(res['grads'][k].numpy(), w.numpy()) <= 1e-10, k
    # the recorded indices reproduce F.max_pool2d, and given back they give the same step
    x = torch.randn(2, 3, 6, 10, dtype=torch.float64)
    assert torch.equal(pr.pool_by_index(x, pr.windows(x).argmax(4)), torch.nn.functional.max_pool2d(x, 2, 2))


@pytest.mark.parametrize('layer_type', ['basic', 'bottleneck'])
def test_state_dict_layout_and_children_are_the_reference_s(golden, layer_type):
    import torch
    from cdnet_amd.models.FullNet import FCN_pooling, FullNet
    g = golden('fcn_pooling')
    m = FCN_pooling(3, 3, layer_type=layer_type)
    sd = m.state_dict()
    assert list(sd) == [str(k) for k in g['keys_' + layer_type]]
    assert [','.join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in g['shapes_' + layer_type]]
    assert [n for n, _ in m.blocks.named_children()] == [str(n) for n in g['children']]
    assert isinstance(m, FullNet) and len(sd) == len(FullNet(3, 3, layer_type=layer_type).state_dict())
    assert isinstance(m.blocks.pool4, torch.nn.MaxPool2d) and m.blocks.pool4.kernel_size == 2 and m.blocks.pool4.stride == 2
    assert isinstance(m.blocks.upsample6, torch.nn.UpsamplingBilinear2d) and m.blocks.upsample6.scale_factor == 4
    assert m.final_conv is m.conv2


def test_initialisation_is_full_net_s_and_fewer_than_seven_dilations_raise():
    import torch
    from cdnet_amd.models.FullNet import FCN_pooling, FullNet
    torch.manual_seed(3)
    a = FCN_pooling(3, 3)
    torch.manual_seed(3)
    b = FullNet(3, 3)
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka
    with pytest.raises(IndexError):
        FCN_pooling(3, 3, n_layers=4, dilations=(1, 2, 4))


def test_strict_load_of_the_golden_weights(golden):
    import _fcn_pooling_ref as pr
    from cdnet_amd.models.FullNet import FCN_pooling
    g = golden('fcn_pooling')
    m = FCN_pooling(**pr.GOLDEN)
    assert sum(p.numel() for p in m.parameters()) == 30016
    res = m.load_state_dict(pr.golden_state(g), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert [getattr(m.blocks, 'trans%d' % i).conv.out_channels for i in range(1, 8)] == [20, 18, 17, 16, 16, 16, 16]
    assert [c.dilation[0] for c in m.blocks.block5.modules() if c.__class__.__name__ == 'Conv2d'] == list(pr.GOLDEN_DILATIONS[4])


def test_cpu_training_and_odd_size_forwards_are_refused():
    import torch
    import _fcn_pooling_ref as pr
    from cdnet_amd.models.FullNet import FCN_pooling
    m = FCN_pooling(**pr.GOLDEN).eval()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m(torch.zeros(1, 3, 32, 32))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m.forward_packed(torch.zeros(1, 32, 32, 16))
    for h, w in ((24, 32), (32, 40), (8, 8)):
        with pytest.raises(ValueError, match='multiples of 16'):
            m.forward_packed(torch.zeros(1, h, w, 16))
    m.train()
    with pytest.raises(RuntimeError, match='inference only'):
        m.forward_packed(torch.zeros(1, 32, 32, 16))


X, Y, I = 0x10000, 0x20000, 0x30000                # never dereferenced: every case below is refused before any HIP call
BIG = 1 << 20


def _pool_fwd(x=X, xs=16, y=Y, ys=24, yoff=8, idx=I, istr=16, N=1, H=8, W=8, C=12, f32=1):
    return 'cdnet_maxpool2_forward', (x, xs, y, ys, yoff, idx, istr, N, H, W, C, f32, None)


def _pool_bwd(dy=Y, dys=24, dyoff=8, idx=I, istr=16, dx=X, dxs=16, N=1, H=8, W=8, C=12):
    return 'cdnet_maxpool2_backward', (dy, dys, dyoff, idx, istr, dx, dxs, N, H, W, C, None)


def _up_fwd(x=X, xs=16, y=Y, ys=24, yoff=8, N=1, Hs=2, Ws=3, C=12, f32=1):
    return 'cdnet_upsample4_bilinear_forward', (x, xs, y, ys, yoff, N, Hs, Ws, C, f32, None)


def _up_bwd(dy=Y, dys=24, dyoff=8, dx=X, dxs=16, N=1, Hs=2, Ws=3, C=12):
    return 'cdnet_upsample4_bilinear_backward', (dy, dys, dyoff, dx, dxs, N, Hs, Ws, C, None)


BAD = {
    'pool fwd null x': _pool_fwd(x=None), 'pool fwd null y': _pool_fwd(y=None), 'pool fwd odd H': _pool_fwd(H=7), 'pool fwd odd W': _pool_fwd(W=9),
    'pool fwd N 0': _pool_fwd(N=0), 'pool fwd C 0': _pool_fwd(C=0), 'pool fwd x stride < C': _pool_fwd(xs=8),
    'pool fwd slice past stride': _pool_fwd(yoff=16), 'pool fwd negative offset': _pool_fwd(yoff=-4), 'pool fwd idx stride < C': _pool_fwd(istr=8),
    'pool fwd in place': _pool_fwd(y=X), 'pool fwd too large': _pool_fwd(N=BIG, H=BIG, W=BIG), 'pool fwd items': _pool_fwd(N=4, H=1 << 15, W=1 << 15, C=129, xs=136, ys=136, yoff=0, istr=136),
    'pool bwd null dy': _pool_bwd(dy=None), 'pool bwd null idx': _pool_bwd(idx=None), 'pool bwd null dx': _pool_bwd(dx=None),
    'pool bwd odd H': _pool_bwd(H=6, W=5), 'pool bwd dx stride < C': _pool_bwd(dxs=8), 'pool bwd slice past stride': _pool_bwd(dys=16),
    'pool bwd idx stride < C': _pool_bwd(istr=4), 'pool bwd in place': _pool_bwd(dx=Y), 'pool bwd too large': _pool_bwd(N=BIG, H=BIG, W=BIG),
    'up fwd null x': _up_fwd(x=None), 'up fwd null y': _up_fwd(y=None), 'up fwd Hs 0': _up_fwd(Hs=0), 'up fwd x stride < C': _up_fwd(xs=11),
    'up fwd slice past stride': _up_fwd(ys=19), 'up fwd Ws beyond 8192': _up_fwd(Ws=8193), 'up fwd in place': _up_fwd(y=X),
    'up fwd too large': _up_fwd(N=BIG, Hs=8192, Ws=8192),
    'up bwd null dy': _up_bwd(dy=None), 'up bwd null dx': _up_bwd(dx=None), 'up bwd W 0': _up_bwd(Ws=0), 'up bwd dx stride < C': _up_bwd(dxs=8),
    'up bwd slice past stride': _up_bwd(dyoff=13), 'up bwd Hs beyond 8192': _up_bwd(Hs=10000), 'up bwd in place': _up_bwd(dx=Y),
    'up bwd too large': _up_bwd(N=BIG, Hs=8192, Ws=8192),
}


@pytest.mark.parametrize('case', sorted(BAD))
def test_rejected_arguments(case):
    from cdnet_amd import _lib
    lib = _lib.load()
    name, args = BAD[case]
    rc = getattr(lib, name)(*args)
    assert rc == 1, case                                       # CDNET_E_ARG
    assert name.encode() in lib.cdnet_last_error(), lib.cdnet_last_error()


def test_a_null_index_pointer_is_not_an_argument_error_by_itself():
    """inference passes idx = NULL; the check that refuses this call is the odd size, and its text says so"""
    from cdnet_amd import _lib
    lib = _lib.load()
    name, args = _pool_fwd(idx=None, istr=0, H=6, W=7)
    assert getattr(lib, name)(*args) == 1 and b'must be even' in lib.cdnet_last_error()
