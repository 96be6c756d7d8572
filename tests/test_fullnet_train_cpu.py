"""FullNet training without a GPU: the new argument structs' sizes, every refused argument of the training entries (found before any HIP
call: the pointers below are never dereferenced) and the trainer a FullNet gets."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

E_ARG = 1


def test_struct_sizes():
    from cdnet_amd import _lib
    lib = _lib.load()
    for name, cls in (('cdnet_dilated_bwd_data_args', _lib.DilatedBwdDataArgs), ('cdnet_dilated_wgrad_args', _lib.DilatedWgradArgs),
                      ('cdnet_slice_bn_fwd_args', _lib.SliceBnFwdArgs), ('cdnet_slice_bn_bwd_args', _lib.SliceBnBwdArgs)):
        assert lib.cdnet_abi_sizeof(name.encode()) == C.sizeof(cls) > 0, name
    # the inference struct stays as it was
    assert C.sizeof(_lib.DilatedConvArgs) == lib.cdnet_abi_sizeof(b'cdnet_dilated_conv_args') == 96


def test_workspace_sizes():
    from cdnet_amd import _lib
    lib = _lib.load()
    assert lib.cdnet_dilated_wgrad_workspace_bytes(2, 9, 37, 168, 24, 9) % (9 * 32 * 192 * 4) == 0
    assert lib.cdnet_dilated_wgrad_workspace_bytes(2, 9, 37, 168, 24, 9) >= 9 * 32 * 192 * 4
    assert lib.cdnet_dilated_wgrad_workspace_bytes(2, 9, 37, 168, 24, 3) == 0
    assert lib.cdnet_dilated_wgrad_workspace_bytes(0, 9, 37, 168, 24, 9) == 0
    assert lib.cdnet_slice_bn_workspace_floats(666, 24) >= 2 * 24 + 2 * 24
    assert lib.cdnet_slice_bn_workspace_floats(0, 24) == 0 and lib.cdnet_slice_bn_workspace_floats(666, 0) == 0


def _fill(a, base, kw):
    for k, v in dict(base, **kw).items():
        setattr(a, k, v)
    return a


BWD_DATA = dict(g=0x10000, w=0x20000, dx=0x30000, N=1, H=8, W=8, Cout=24, g_cstride=24, Cin=40, dx_cstride=48, dx_coff=0, taps=9, dilation=1,
                accumulate=1, f32=1)
BAD_BWD_DATA = {
    'null g': dict(g=None), 'null w': dict(w=None), 'null dx': dict(dx=None), 'taps 3': dict(taps=3), 'taps 0': dict(taps=0),
    'dilation 0': dict(dilation=0), 'N 0': dict(N=0), 'H 0': dict(H=0), 'W -1': dict(W=-1), 'Cin 0': dict(Cin=0), 'Cout 0': dict(Cout=0),
    'g stride < Cout': dict(Cout=32), 'g stride not 8': dict(g_cstride=28), 'dx stride < Cin': dict(dx_cstride=32),
    'dx slice past stride': dict(dx_coff=16), 'negative dx_coff': dict(dx_coff=-8),
    'accumulate onto the source': dict(dx=0x10000, g_cstride=48), 'in place strides differ': dict(dx=0x10000, dx_coff=24, Cin=8),
    'in place overlap': dict(dx=0x10000, g_cstride=48, dx_coff=8, Cin=8),
}


@pytest.mark.parametrize('case', sorted(BAD_BWD_DATA))
def test_backward_data_refusals(case):
    from cdnet_amd import _lib
    lib = _lib.load()
    rc = lib.cdnet_dilated_conv_backward_data(C.byref(_fill(_lib.DilatedBwdDataArgs(), BWD_DATA, BAD_BWD_DATA[case])), None)
    assert rc == E_ARG, case
    assert b'cdnet_dilated_conv_backward_data' in lib.cdnet_last_error()


WGRAD = dict(x=0x10000, g=0x20000, dw=0x30000, ws=0x40000, ws_bytes=1 << 40, N=1, H=8, W=8, Cin=40, x_cstride=48, Cout=24, g_cstride=24, taps=9,
             dilation=2)
BAD_WGRAD = {
    'null x': dict(x=None), 'null g': dict(g=None), 'null dw': dict(dw=None), 'null ws': dict(ws=None), 'taps 4': dict(taps=4),
    'dilation 0': dict(dilation=0), 'N 0': dict(N=0), 'H 0': dict(H=0), 'W 0': dict(W=0), 'Cin 0': dict(Cin=0), 'Cout -1': dict(Cout=-1),
    'x stride < Cin': dict(Cin=56), 'x stride not 8': dict(x_cstride=44), 'g stride < Cout': dict(Cout=25), 'g stride not 8': dict(g_cstride=28),
    'short workspace': dict(ws_bytes=1024),
}


@pytest.mark.parametrize('case', sorted(BAD_WGRAD))
def test_weight_gradient_refusals(case):
    from cdnet_amd import _lib
    lib = _lib.load()
    rc = lib.cdnet_dilated_conv_backward_weight(C.byref(_fill(_lib.DilatedWgradArgs(), WGRAD, BAD_WGRAD[case])), None)
    assert rc == E_ARG, case
    assert b'cdnet_dilated_conv_backward_weight' in lib.cdnet_last_error()


BN_FWD = dict(z=0x10000, out=0x20000, gamma=0x30000, beta=0x31000, running_mean=0x32000, running_var=0x33000, mean=0x34000, invstd=0x35000,
              ws=0x40000, ws_floats=1 << 30, P=64, C=24, z_cstride=24, out_cstride=48, out_coff=8, eps=1e-5, momentum=0.1, p_drop=0.1, layer=3, key=5)
BAD_BN_FWD = {
    'null z': dict(z=None), 'null out': dict(out=None), 'null gamma': dict(gamma=None), 'null beta': dict(beta=None), 'null mean': dict(mean=None),
    'null invstd': dict(invstd=None), 'null ws': dict(ws=None), 'one running statistic': dict(running_var=None), 'P 0': dict(P=0), 'C 0': dict(C=0),
    'z stride < C': dict(z_cstride=16), 'slice past stride': dict(out_coff=32), 'negative out_coff': dict(out_coff=-1), 'out is z': dict(out=0x10000),
    'p 1': dict(p_drop=1.0), 'p negative': dict(p_drop=-0.1), 'layer negative': dict(layer=-1), 'short workspace': dict(ws_floats=16),
}


@pytest.mark.parametrize('case', sorted(BAD_BN_FWD))
def test_bn_forward_refusals(case):
    from cdnet_amd import _lib
    lib = _lib.load()
    rc = lib.cdnet_slice_bn_train_forward(C.byref(_fill(_lib.SliceBnFwdArgs(), BN_FWD, BAD_BN_FWD[case])), None)
    assert rc == E_ARG, case
    assert b'cdnet_slice_bn_train_forward' in lib.cdnet_last_error()


BN_BWD = dict(dy=0x10000, z=0x20000, mean=0x30000, invstd=0x31000, gamma=0x32000, dgamma=0x33000, dbeta=0x34000, g=0x50000, ws=0x40000,
              ws_floats=1 << 30, P=64, C=24, z_cstride=24, dy_cstride=48, dy_coff=8, g_cstride=24, slope=0.01, p_drop=0.1, layer=3, key=5)
BAD_BN_BWD = {
    'null dy': dict(dy=None), 'null z': dict(z=None), 'null mean': dict(mean=None), 'null invstd': dict(invstd=None), 'null gamma': dict(gamma=None),
    'null dgamma': dict(dgamma=None), 'null dbeta': dict(dbeta=None), 'null g': dict(g=None), 'null ws': dict(ws=None), 'P 0': dict(P=0),
    'C 0': dict(C=0), 'z stride < C': dict(z_cstride=16), 'g stride < C': dict(g_cstride=16), 'slice past stride': dict(dy_coff=32),
    'negative dy_coff': dict(dy_coff=-1), 'g is dy': dict(g=0x10000), 'g is z': dict(g=0x20000), 'p 1': dict(p_drop=1.0),
    'layer negative': dict(layer=-1), 'short workspace': dict(ws_floats=16),
}


@pytest.mark.parametrize('case', sorted(BAD_BN_BWD))
def test_bn_backward_refusals(case):
    from cdnet_amd import _lib
    lib = _lib.load()
    rc = lib.cdnet_slice_bn_train_backward(C.byref(_fill(_lib.SliceBnBwdArgs(), BN_BWD, BAD_BN_BWD[case])), None)
    assert rc == E_ARG, case
    assert b'cdnet_slice_bn_train_backward' in lib.cdnet_last_error()


def test_null_args_pack_and_mask_refusals():
    from cdnet_amd import _lib
    lib = _lib.load()
    for fn in ('cdnet_dilated_conv_backward_data', 'cdnet_dilated_conv_backward_weight', 'cdnet_slice_bn_train_forward',
               'cdnet_slice_bn_train_backward'):
        assert getattr(lib, fn)(None, None) == E_ARG, fn
    assert lib.cdnet_dilated_pack_weights_bwd(None, 0x1000, 3, 24, 9, 1, None) == E_ARG
    assert lib.cdnet_dilated_pack_weights_bwd(0x1000, None, 3, 24, 9, 1, None) == E_ARG
    assert lib.cdnet_dilated_pack_weights_bwd(0x1000, 0x2000, 3, 0, 9, 1, None) == E_ARG
    assert lib.cdnet_dilated_pack_weights_bwd(0x1000, 0x2000, 3, 24, 3, 1, None) == E_ARG
    assert b'cdnet_dilated_pack_weights_bwd' in lib.cdnet_last_error()
    assert lib.cdnet_dropout_mask(1, 0, 16, 0.1, None, None) == E_ARG
    assert lib.cdnet_dropout_mask(1, 0, 0, 0.1, 0x1000, None) == E_ARG
    assert lib.cdnet_dropout_mask(1, 0, 16, 1.0, 0x1000, None) == E_ARG
    assert lib.cdnet_dropout_mask(1, -1, 16, 0.1, 0x1000, None) == E_ARG
    assert b'cdnet_dropout_mask' in lib.cdnet_last_error()


def test_trainer_class_of_a_fullnet():
    import _fullnet_ref as fr
    from cdnet_amd import trainer, utils
    from cdnet_amd.models.FullNet import FullNet
    assert utils.trainer_class(FullNet(**fr.SMALL)) is trainer.FullNetTrainer
    assert issubclass(trainer.FullNetTrainer, trainer.UNetTrainer)


def test_forward_in_training_mode_without_a_tape_still_raises():
    import torch
    import _fullnet_ref as fr
    from cdnet_amd import runtime
    from cdnet_amd.models.FullNet import FullNet
    assert runtime.TAPE is None
    with pytest.raises(RuntimeError, match='inference only'):
        FullNet(**fr.SMALL).train().forward_packed(torch.zeros(1, 8, 8, 16))
