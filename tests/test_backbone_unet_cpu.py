"""Host-side checks of the backbone U-Net `UNet_vgg16` (cdnet_amd/models/model_unet.py): the factory and the entries know the name, the
state_dict is the reference's (tests/golden/backbone_unet.npz, written by tests/golden/make_golden_backbone_unet.py from the reference
class), the 16-channel classifier's C entries check their arguments before any HIP call, and the CPU mirror of the GPU tests
(tests/_backbone_unet_ref.py) reproduces the reference's eval logits."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


class _Opt:
    def __init__(self, name):
        self.model = {'modelName': name, 'out_c': 3, 'in_c': 3}


def _model():
    from cdnet_amd import utils
    return utils.chooseModel(_Opt('UNet_vgg16'))


def test_choose_model_returns_the_new_class_with_the_reference_state_dict(golden):
    from cdnet_amd.models.model_unet import Unet
    z = golden('backbone_unet')
    m = _model()
    assert type(m) is Unet and m.final_conv.out_channels == 3 and m.final_conv.in_channels == 16
    assert list(m.state_dict().keys()) == [str(k) for k in z['keys']]
    assert sum(p.numel() for p in m.parameters()) == int(z['n_params'][0])
    assert Unet.UNUSED_PREFIXES == ('child0.', 'child_conv1.')
    assert not hasattr(m, 'mask_conv')                   # pipeline.mask_channels reads final_conv


def test_names_still_refused_and_other_backbones():
    from cdnet_amd import utils
    from cdnet_amd.models.model_unet import Unet
    for name in ('UNet_resnet50', 'UNet_resnet101'):
        with pytest.raises(NotImplementedError):
            utils.chooseModel(_Opt(name))
    with pytest.raises(NotImplementedError, match='ResNet'):
        Unet(backbone_name='resnet50')


def test_entries_know_the_name():
    from cdnet_amd import test, trainer, utils
    test.check_model_name('UNet_vgg16')
    assert utils.trainer_class(_model()) is trainer.BackboneUNetTrainer


def test_cpu_tensor_is_refused():
    import torch
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        _model()(torch.zeros((1, 3, 32, 32)))


FAKE = C.c_void_p(4096)          # (never dereferenced: every call below fails its argument checks first)


def test_c16_entries_reject_bad_arguments_without_a_gpu():
    from cdnet_amd import _lib, runtime
    lib = _lib.load()
    err = lambda: lib.cdnet_last_error().decode()

    def feat(raw=4096, res=None):
        f = runtime.HeadFeat()
        f.raw, f.res, f.scale, f.shift, f.relu, f.f16 = raw, res, None, None, 0, 0
        return f
    ok = feat()
    need = lib.cdnet_final_conv1x1_c16_backward_workspace_floats()
    assert need > 0

    def fwd(f=ok, w=FAKE, b=FAKE, K=3, out=FAKE):
        return lib.cdnet_final_conv1x1_c16(None if f is None else C.byref(f), w, b, K, 1, 4, 4, out, None)

    def bwd(f=ok, w=FAKE, dl=FAKE, K=3, df=FAKE, ws=FAKE, n=need, dw=FAKE, db=FAKE):
        return lib.cdnet_final_conv1x1_c16_backward(None if f is None else C.byref(f), w, dl, K, 1, 4, 4, df, ws, n, dw, db, None)
    for kw in (dict(f=None), dict(f=feat(raw=None)), dict(w=None), dict(b=None), dict(out=None)):
        assert fwd(**kw) == 1 and 'null pointer' in err(), kw
    for kw in (dict(f=None), dict(f=feat(raw=None)), dict(w=None), dict(dl=None), dict(df=None), dict(ws=None), dict(dw=None), dict(db=None)):
        assert bwd(**kw) == 1 and 'null pointer' in err(), kw
    for K in (0, 21):
        assert fwd(K=K) == 1 and 'K=%d' % K in err()
        assert bwd(K=K) == 1 and 'K=%d' % K in err()
    assert fwd(f=feat(res=4096)) == 1 and 'res must be NULL' in err()
    assert bwd(f=feat(res=4096)) == 1 and 'res must be NULL' in err()
    assert fwd(f=feat(raw=4096 + 8)) == 1 and '16-byte aligned' in err()
    assert bwd(n=need - 1) == 2 and 'workspace' in err()                 # CDNET_E_WORKSPACE


@pytest.mark.parametrize('case', ['', '_ragged'])
def test_mirror_reproduces_the_reference_eval_logits(golden, case):
    """fp32 on the CPU, within 1e-3 of the output scale (the golden is stored as float16: 2^-11 = 4.9e-4 of a value's binade)"""
    import torch
    import _backbone_unet_ref as br
    from cdnet_amd import synth
    z = golden('backbone_unet')
    cfg = [int(v) for v in z['x' + case + '_cfg']]
    want = z['y_eval' + case].astype(np.float32)
    ref = br.det_model().eval()
    with torch.no_grad():
        got = ref(torch.from_numpy(synth.det_input(tuple(cfg[:4]), cfg[4]))).numpy()
    assert got.shape == want.shape
    scale = np.abs(want).max()
    assert np.abs(got - want).max() <= 1e-3 * scale, (np.abs(got - want).max(), scale)
