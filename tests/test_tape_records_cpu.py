"""The declared shape of what a training forward leaves for backward (no GPU): ConvLayer, FuseNode, Src and the two tape records have
fixed fields with the defaults the tape walk relies on, and a misspelt name raises instead of silently selecting another backward path."""
import pytest
import torch


def _objects():
    from cdnet_amd import runtime
    from cdnet_amd.engine import Src
    bn = torch.nn.BatchNorm2d(32)
    layer = runtime.ConvLayer('c', 'conv3', torch.zeros((32, 16, 3, 3)), None, bn)
    src = Src(torch.zeros((1, 4, 4, 16), dtype=torch.bfloat16))
    node = runtime.FuseNode('fuse.0')
    out = torch.zeros((1, 4, 4, 32), dtype=torch.float16)
    crec = runtime.ConvRecord(layer, [src], out, 4, 4, True)
    frec = runtime.FuseRecord(node, [src], out, True, 4, 4, 32, 0)
    return layer, src, node, crec, frec


def test_declared_defaults():
    from cdnet_amd import runtime
    layer, src, node, crec, frec = _objects()
    assert layer.needs_input_grad is True and layer.bias_grad_from is None and layer.fold_eval is True and layer.rec is None
    for name in ('wpe', 'wps', 'ru_wr', 'ru_pack'):
        assert getattr(layer, name) is None and getattr(layer, name + '_version') is None, name
    assert layer in runtime.LAYERS                       # (the weak set of live layers still takes a slotted layer)
    assert src.grad_to is None and src.is_input is False
    assert node.name == 'fuse.0'
    assert crec.layer is layer and crec.srcs[0] is src and (crec.H, crec.W) == (4, 4) and crec.relu is True
    assert crec.res is None and crec.res_grad_to is None and crec.fused_res_of is None and crec.deferred is None
    assert frec.node is node and frec.terms[0] is src and frec.relu is True and (frec.H, frec.W, frec.C, frec.coff) == (4, 4, 32, 0)
    bare = runtime.ConvLayer('r', 'conv1', torch.zeros((32, 16, 1, 1)), torch.zeros((32,)), None)
    assert bare.scale is None and bare.save_invstd is None and bare.needs_input_grad is True


def test_sources_take_their_flags_at_construction():
    from cdnet_amd.engine import Src
    x = torch.zeros((1, 4, 4, 16), dtype=torch.bfloat16)
    s = Src(x, grad_to=(x, 1), is_input=True)
    assert s.grad_to[0] is x and s.grad_to[1] == 1 and s.is_input is True


@pytest.mark.parametrize('which', range(5))
def test_a_misspelt_name_raises(which):
    obj = _objects()[which]
    for name in ('need_input_grad', 'grad_too'):
        with pytest.raises(AttributeError):
            setattr(obj, name, None)
    assert not hasattr(obj, '__dict__')
