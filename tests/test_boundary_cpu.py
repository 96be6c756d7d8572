"""The boundary / focal term (--boundary-loss 1|2|3) without a GPU: the entries exist, their argument checks answer before any HIP call, the
option reaches opt.model and the training entry accepts 0..3 only."""
import ctypes as C
import os
import re

import pytest
from conftest import ROOT

NAMES = ('cdnet_boundary_loss_workspace_bytes', 'cdnet_boundary_loss', 'cdnet_boundary_loss_scratch_bytes')


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
    assert _l.SIGNATURES[NAMES[0]][0] is C.c_size_t and len(_l.SIGNATURES[NAMES[0]][1]) == 5
    assert _l.SIGNATURES[NAMES[1]][0] is C.c_int and len(_l.SIGNATURES[NAMES[1]][1]) == 14
    assert _l.SIGNATURES[NAMES[2]] == (C.c_int, [])
    assert lib.cdnet_abi_version() == 5
    assert 'boundary.hip' in __import__('cdnet_amd.csrc.build', fromlist=['SOURCES']).SOURCES


def test_workspace_size():
    _, lib = _lib()
    f = lib.cdnet_boundary_loss_workspace_bytes
    for kind in (1, 2, 3):
        assert f(kind, 2, 3, 40, 72) > 0 and f(kind, 2, 3, 40, 72) % 8 == 0
        assert f(kind, 1, 3, 1, 1) > 0                              # any H, W >= 1
        assert f(kind, 2, 2, 40, 72) == 0 and f(kind, 2, 4, 40, 72) == 0 and f(kind, 2, 1, 40, 72) == 0      # K != 3
        assert f(kind, 0, 3, 40, 72) == 0 and f(kind, 2, 3, 0, 72) == 0 and f(kind, 2, 3, 40, -1) == 0
    assert f(0, 2, 3, 40, 72) == 0 and f(4, 2, 3, 40, 72) == 0 and f(-1, 2, 3, 40, 72) == 0
    # kind 1: four sums per class and 32 x 32 tile, one double each; kinds 2 and 3 share one kernel
    assert f(1, 2, 3, 40, 72) == 2 * 2 * 3 * 12 * 8
    assert f(2, 2, 3, 40, 72) == f(3, 2, 3, 40, 72)


def test_argument_validation_without_gpu():
    _, lib = _lib()
    B, K, H, W = 1, 3, 8, 8
    need = lib.cdnet_boundary_loss_workspace_bytes(1, B, K, H, W)
    assert need > 0
    logits, label, out = (C.c_float * (B * K * H * W))(), (C.c_uint8 * (B * H * W))(), (C.c_float * 1)()
    ws = (C.c_double * (need // 8 + 1))()                         # host memory: no check may touch it

    def call(logits=logits, label=label, kind=1, K=K, ws=ws, ws_bytes=need, out=out, H=H):
        p = lambda a: None if a is None else C.cast(a, C.c_void_p)
        return lib.cdnet_boundary_loss(p(logits), p(label), kind, B, K, H, W, 1.0, p(ws), ws_bytes, p(out), None, None, None)

    E_ARG = 1
    for kw in (dict(logits=None), dict(label=None), dict(ws=None), dict(out=None)):
        assert call(**kw) == E_ARG and b'null pointer' in lib.cdnet_last_error(), kw
    for kind in (0, 4, -1):
        assert call(kind=kind) == E_ARG and b'kind=%d' % kind in lib.cdnet_last_error()
    assert call(K=4) == E_ARG and b'K=4' in lib.cdnet_last_error()
    assert call(K=2) == E_ARG
    assert call(H=0) == E_ARG and b'bad size' in lib.cdnet_last_error()
    for kind in (1, 2, 3):
        n = lib.cdnet_boundary_loss_workspace_bytes(kind, B, K, H, W)
        assert call(kind=kind, ws_bytes=n - 1) == E_ARG and b'workspace' in lib.cdnet_last_error()


def test_option_reaches_the_model_dict():
    from cdnet_amd.options import Options
    opt = Options(isTrain=True)
    assert opt.model['boundary_loss'] == 0
    opt.parse(['--boundary-loss', '2'])
    assert opt.model['boundary_loss'] == 2


def test_get_optimizer_accepts_0_to_3_only():
    """the range check comes first, so it is reached with no model and no device"""
    from cdnet_amd import utils
    from cdnet_amd.options import Options
    for bad in (4, -1, 7):
        opt = Options(isTrain=True)
        opt.model['boundary_loss'] = bad
        with pytest.raises(ValueError, match=re.escape('boundary_loss = %r' % bad)):
            utils.get_optimizer(opt, None)
