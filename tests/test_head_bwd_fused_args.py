"""cdnet_dam_head_backward_fused refuses everything but its one case before any HIP call (no GPU needed)."""
import ctypes as C

import numpy as np


def test_fused_head_backward_argument_validation_without_gpu():
    from cdnet_amd import _lib, runtime
    lib = _lib.load()
    buf = np.zeros(64, np.float32)
    q = buf.ctypes.data                                   # (host memory: never dereferenced, every call below is refused)

    def feat(**kw):
        f = runtime.HeadFeat()
        f.raw, f.f16 = q, 2
        for k, v in kw.items():
            setattr(f, k, v)
        return f

    names = ['hw', 'dmask', 'dpoint', 'ddir', 'df1', 'df2', 'dz3', 'ws', 'dhw']

    def call(f1=None, f2=None, f3=None, N=1, H=8, W=8, ws_floats=None, **kw):
        f = [C.byref(x) if x is not None else None for x in (f1 or feat(), f2 or feat(), f3 or feat())]
        p = {n: kw.get(n, q) for n in names}
        wsf = lib.cdnet_dam_head_backward_fused_workspace_floats() if ws_floats is None else ws_floats
        return lib.cdnet_dam_head_backward_fused(f[0], f[1], f[2], p['hw'], p['dmask'], p['dpoint'], p['ddir'], N, H, W, p['df1'], p['df2'],
                                                 p['dz3'], p['ws'], wsf, p['dhw'], None)

    assert lib.cdnet_dam_head_backward_fused_blocks() == 1024          # the two-kernel path's grid: the partition of every sum
    assert lib.cdnet_dam_head_backward_fused_workspace_floats() >= lib.cdnet_dam_head_backward_fused_blocks() * 855
    for n in names:
        assert call(**{n: None}) == 1 and b'null pointer' in lib.cdnet_last_error(), n
    assert lib.cdnet_dam_head_backward_fused(None, None, None, q, q, q, q, 1, 8, 8, q, q, q, q, 1 << 22, q, None) == 1
    assert b'null pointer' in lib.cdnet_last_error()
    # anything but a plain stored fp32 feature: 16-bit storage, a pending BatchNorm, a ReLU, a residual branch
    for bad in (dict(f16=0), dict(f16=1), dict(scale=q, shift=q), dict(relu=1), dict(res=q), dict(raw=None)):
        for k in range(3):
            fs = [feat(), feat(), feat()]
            fs[k] = feat(**bad)
            assert call(*fs) == 1 and b'plain stored fp32' in lib.cdnet_last_error(), (bad, k)
    assert call(N=0) == 1 and call(H=0) == 1
    assert call(N=64, H=1024, W=1024) == 1 and b'32-bit' in lib.cdnet_last_error()
    assert call(ws_floats=16) != 0 and b'workspace' in lib.cdnet_last_error()
