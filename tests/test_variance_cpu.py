"""The instance variance term (--alpha 1) without a GPU: the two entries exist, their argument checks answer before any HIP call, and the
training entry accepts alpha 0 and 1 only."""
import ctypes as C
import os
import re
import types

import pytest
from conftest import ROOT

NAMES = ('cdnet_variance_loss_workspace_bytes', 'cdnet_variance_loss')


def _lib():
    from cdnet_amd.csrc import build
    build.build()
    from cdnet_amd import _lib
    return _lib, _lib.load()


def test_entries_are_declared_exported_and_bound():
    _l, lib = _lib()
    txt = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'cdnet_hip.h')).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r'\b%s\s*\(' % n, txt), n + ' is not declared'
        assert hasattr(lib, n), 'missing export ' + n
    assert _l.SIGNATURES[NAMES[0]][0] is C.c_size_t and len(_l.SIGNATURES[NAMES[0]][1]) == 4
    assert _l.SIGNATURES[NAMES[1]][0] is C.c_int and len(_l.SIGNATURES[NAMES[1]][1]) == 16
    assert lib.cdnet_abi_version() == 5


def test_workspace_size():
    _, lib = _lib()
    f = lib.cdnet_variance_loss_workspace_bytes
    assert f(0, 3, 8, 8) == 0
    assert f(1, 4, 8, 8) == 0 and f(1, 1, 8, 8) == 0            # K outside {2, 3}
    # the forest (4 bytes a pixel) and K sums + a count of 8 bytes for each of the ceil(H/2) * ceil(W/2) possible instances
    assert f(2, 3, 7, 9) >= 2 * (7 * 9 * 4 + 4 * 5 * 4 * 8)
    assert f(16, 3, 256, 256) % 4 == 0


def test_argument_validation_without_gpu():
    _, lib = _lib()
    B, K, H, W = 1, 3, 8, 8
    need = lib.cdnet_variance_loss_workspace_bytes(B, K, H, W)
    assert need > 0
    logits, label, out = (C.c_float * (B * K * H * W))(), (C.c_uint8 * (B * H * W))(), (C.c_float * 1)()
    ws = (C.c_double * (need // 8 + 1))()                         # host memory: no check may touch it

    def call(logits=logits, label=label, K=K, ws=ws, ws_bytes=need, out=out, H=H):
        p = lambda a: None if a is None else C.cast(a, C.c_void_p)
        return lib.cdnet_variance_loss(p(logits), p(label), 1, B, K, H, W, 1.0, p(ws), ws_bytes, p(out), None, None, None, None, None)

    for kw in (dict(logits=None), dict(label=None), dict(ws=None), dict(out=None)):
        assert call(**kw) == 1 and b'null pointer' in lib.cdnet_last_error(), kw
    assert call(K=4) == 1 and b'K=4' in lib.cdnet_last_error()
    assert call(K=1) == 1
    assert call(H=0) == 1 and b'bad size' in lib.cdnet_last_error()
    assert call(ws_bytes=need - 1) == 2 and b'workspace' in lib.cdnet_last_error()


def test_check_branches_accepts_alpha_0_and_1_only():
    from cdnet_amd import train_util_dam
    from cdnet_amd.options import Options
    model = types.SimpleNamespace(VARIANT='rev1')
    for alpha in (0, 1, 0.0, 1.0):
        opt = Options(isTrain=True)
        opt.train['alpha'] = alpha
        train_util_dam._check_branches(opt, model)
    for alpha in (2, 0.5):
        opt = Options(isTrain=True)
        opt.train['alpha'] = alpha
        with pytest.raises(ValueError, match=re.escape(repr(alpha))):
            train_util_dam._check_branches(opt, model)
    opt.train['alpha'] = 2
    with pytest.raises(ValueError, match='out of scope'):
        train_util_dam._check_branches(opt, model)
