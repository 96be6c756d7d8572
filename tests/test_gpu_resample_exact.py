"""The four resampling entries of csrc/resample.hip per element, and the existing dilated / BatchNorm entries at the map sizes FCN_pooling
produces behind its pools.

Layout of every case: N = 2, C in {1, 12, 129}.  The compact side has stride round8(C) (its padding channels hold a sentinel), the slice
side a stride of round8(C) + 24 with the slice at offset 8 (16-byte aligned: the vector kernels) or 3 (the scalar kernels), every other
channel a sentinel; sentinels must survive, inputs must stay unchanged.

  pool forward     small integers (ties in most windows; one case all zeros: every window tied) - the output bit-equal to F.max_pool2d, the
                   index byte equal to numpy's first maximum of the window in raster order;
  pool backward    bit-equal to 'dy at the indexed position, 0 elsewhere' for random indices, and to the autograd of F.max_pool2d for the
                   forward's own indices on a tie-free input;
  upsample forward against F.interpolate(scale_factor=4, mode='bilinear', align_corners=True) in fp64: fp32 |err| <= 2^-20 max|x| (4 weights,
                   each a correctly rounded quotient, a rounded 1 - lambda, 4 products, 3 sums: below 16 units of 2^-24); bf16 <= 2^-8 max|x|
                   (the output rounding added);
  upsample backward against fp64 autograd: per element |err| <= 2^-16 B, B = the fp64 backward of |dy| = sum w |dy| (at most 121 terms of
                   at most 2 roundings each: 256 x 2^-24);
  dilated entries  tests/test_gpu_dilated_conv.py's and tests/test_gpu_fullnet_train_kernels.py's own checks, with their bars, on maps of
                   2 x 3 and 1 x 1 at dilations 1, 13 and 21, and the BatchNorm over P = 4 and P = 12 values per channel."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

N = 2
CS = [1, 12, 129]
COFFS = [8, 3]
SENT = -512.0                  # bf16-exact
IDX_SENT = 0xEE


def _r8(c):
    return (c + 7) // 8 * 8


def _dt(prec):
    import torch
    return torch.float32 if prec == 'fp32' else torch.bfloat16


def _compact(vals, dt):
    """[N,H,W,C] cpu values -> device tensor of stride round8(C), sentinel in the padding"""
    import torch
    n, h, w, c = vals.shape
    t = torch.full((n, h, w, _r8(c)), SENT)
    t[..., :c] = vals
    return t.to(dt).cuda()


def _slice(vals, coff, dt, shape=None):
    """a slice tensor of stride round8(C) + 24: `vals` at [coff, coff + C) (or nothing: an output), sentinel elsewhere"""
    import torch
    n, h, w, c = shape or vals.shape
    t = torch.full((n, h, w, _r8(c) + 24), SENT)
    if vals is not None:
        t[..., coff:coff + c] = vals
    return t.to(dt).cuda()


def _raw(t):
    import torch
    return t.cpu().contiguous().view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _untouched_outside(t, before, lo, hi):
    import torch
    a, b = _raw(t), _raw(before)
    assert torch.equal(a[..., :lo], b[..., :lo]) and torch.equal(a[..., hi:], b[..., hi:]), 'channels outside [%d, %d) changed' % (lo, hi)


def _pool_forward(x, C, coff, prec, want_idx=True):
    """x [N,H,W,C] cpu -> (y slice tensor, idx or None, the compact input as given to the kernel)"""
    import torch
    from cdnet_amd import _lib
    dt = _dt(prec)
    n, h, w, _ = x.shape
    xd = _compact(x, dt)
    y = _slice(None, coff, dt, (n, h // 2, w // 2, C))
    idx = torch.full((n, h // 2, w // 2, _r8(C)), IDX_SENT, dtype=torch.uint8, device='cuda') if want_idx else None
    x0, y0 = xd.clone(), y.clone()
    _lib.call('cdnet_maxpool2_forward', _lib.ptr(xd), xd.shape[3], _lib.ptr(y), y.shape[3], coff, _lib.ptr(idx), _r8(C), n, h, w, C,
              int(prec == 'fp32'), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(_raw(xd), _raw(x0)), 'the input changed'
    _untouched_outside(y, y0, coff, coff + C)
    if want_idx:
        assert bool((idx[..., C:] == IDX_SENT).all()), 'index padding bytes written'
    return y, idx


def _windows(x):
    """numpy [N,H,W,C] -> [N,H/2,W/2,C,4] in raster order"""
    n, h, w, c = x.shape
    return x.reshape(n, h // 2, 2, w // 2, 2, c).transpose(0, 1, 3, 5, 2, 4).reshape(n, h // 2, w // 2, c, 4)


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@pytest.mark.parametrize('coff', COFFS)
@pytest.mark.parametrize('C', CS)
@pytest.mark.parametrize('hw', [(2, 2), (6, 10), (32, 48), 'tied'], ids=str)
def test_pool_forward(hw, C, coff, prec):
    import torch
    import torch.nn.functional as F
    tied = hw == 'tied'
    h, w = (6, 10) if tied else hw
    g = torch.Generator().manual_seed(1000 + 7 * h + C + coff)
    x = torch.zeros((N, h, w, C)) if tied else torch.randint(-3, 4, (N, h, w, C), generator=g).float()
    y, idx = _pool_forward(x, C, coff, prec)
    want = F.max_pool2d(x.permute(0, 3, 1, 2).to(_dt(prec)).float(), 2, 2).permute(0, 2, 3, 1).to(_dt(prec))
    assert torch.equal(_raw(y[..., coff:coff + C]), _raw(want)), 'not bit-equal to F.max_pool2d'
    first = _windows(x.numpy()).argmax(4)                                        # numpy: the first maximum
    assert np.array_equal(idx[..., :C].cpu().numpy(), first.astype(np.uint8))
    if tied:
        assert not bool(idx[..., :C].any())
    else:
        assert len(np.unique(first)) == 4 or h * w * C < 64
    # inference: no index output, the same values
    y2, none = _pool_forward(x, C, coff, prec, want_idx=False)
    assert none is None and torch.equal(_raw(y2), _raw(y))


@pytest.mark.parametrize('coff', COFFS)
@pytest.mark.parametrize('C', CS)
@pytest.mark.parametrize('hw', [(2, 2), (6, 10), (32, 48)], ids=str)
def test_pool_backward(hw, C, coff):
    import torch
    import torch.nn.functional as F
    from cdnet_amd import _lib
    h, w = hw
    g = torch.Generator().manual_seed(2000 + 7 * h + C + coff)

    def backward(dy, idx):
        dyd = _slice(dy, coff, torch.float32)
        dx = torch.full((N, h, w, _r8(C)), SENT, device='cuda')
        dy0, idx0 = dyd.clone(), idx.clone()
        _lib.call('cdnet_maxpool2_backward', _lib.ptr(dyd), dyd.shape[3], coff, _lib.ptr(idx), idx.shape[3], _lib.ptr(dx), dx.shape[3], N, h, w, C,
                  _lib.stream_ptr())
        torch.cuda.synchronize()
        assert torch.equal(_raw(dyd), _raw(dy0)) and torch.equal(idx, idx0)
        assert bool((dx[..., C:] == SENT).all()), 'padding channels of dx written'
        return dx[..., :C].cpu()

    # random indices (ties or not, whatever the forward would have chosen): dy at the indexed position, 0 elsewhere
    dy = torch.randn((N, h // 2, w // 2, C), generator=g)
    k = torch.randint(0, 4, (N, h // 2, w // 2, C), generator=g).to(torch.uint8)
    idx = torch.full((N, h // 2, w // 2, _r8(C)), IDX_SENT, dtype=torch.uint8)
    idx[..., :C] = k
    got = backward(dy, idx.cuda())
    want = torch.zeros((N, h // 2, 2, w // 2, 2, C))
    for pos in range(4):
        want[:, :, pos // 2, :, pos % 2, :] = torch.where(k == pos, dy, torch.zeros(()))
    assert torch.equal(_raw(got), _raw(want.reshape(N, h, w, C)))

    # the forward's own indices on a tie-free input: the autograd of F.max_pool2d, bit for bit
    x = (torch.randperm(N * h * w * C, generator=g).float() - 1000.0).view(N, h, w, C)            # all values distinct, fp32-exact
    _, fidx = _pool_forward(x, C, coff, 'fp32')
    got = backward(dy, fidx)
    xn = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    F.max_pool2d(xn, 2, 2).backward(dy.permute(0, 3, 1, 2))
    assert torch.equal(_raw(got), _raw(xn.grad.permute(0, 2, 3, 1)))


UP_SIZES = [(1, 1), (1, 3), (2, 3), (5, 7), (16, 12)]


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@pytest.mark.parametrize('coff', COFFS)
@pytest.mark.parametrize('C', CS)
@pytest.mark.parametrize('hw', UP_SIZES, ids=str)
def test_upsample_forward(hw, C, coff, prec):
    import torch
    import torch.nn.functional as F
    from cdnet_amd import _lib
    hs, ws = hw
    dt = _dt(prec)
    g = torch.Generator().manual_seed(3000 + 7 * hs + C + coff)
    x = torch.randn((N, hs, ws, C), generator=g).to(dt).float()
    xd = _compact(x, dt)
    y = _slice(None, coff, dt, (N, 4 * hs, 4 * ws, C))
    x0, y0 = xd.clone(), y.clone()
    _lib.call('cdnet_upsample4_bilinear_forward', _lib.ptr(xd), xd.shape[3], _lib.ptr(y), y.shape[3], coff, N, hs, ws, C, int(prec == 'fp32'),
              _lib.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(_raw(xd), _raw(x0)), 'the input changed'
    _untouched_outside(y, y0, coff, coff + C)
    want = F.interpolate(x.permute(0, 3, 1, 2).double(), scale_factor=4, mode='bilinear', align_corners=True).permute(0, 2, 3, 1)
    got = y[..., coff:coff + C].cpu().double()
    err = float((got - want).abs().max())
    bar = (2.0 ** -20 if prec == 'fp32' else 2.0 ** -8) * float(x.abs().max())
    print('upsample forward %s %dx%d C %d coff %d: max err %.3g, bar %.3g, ratio %.3f' % (prec, hs, ws, C, coff, err, bar, err / bar))
    assert err <= bar
    # the corners are copies (align_corners=True), and a size of 1 copies along its axis
    src = x.to(dt)
    assert torch.equal(_raw(y[:, 0, 0, coff:coff + C]), _raw(src[:, 0, 0])) and torch.equal(_raw(y[:, -1, -1, coff:coff + C]), _raw(src[:, -1, -1]))
    if hs == 1:
        assert torch.equal(_raw(y[:, 3, 0, coff:coff + C]), _raw(src[:, 0, 0]))


@pytest.mark.parametrize('coff', COFFS)
@pytest.mark.parametrize('C', CS)
@pytest.mark.parametrize('hw', UP_SIZES, ids=str)
def test_upsample_backward(hw, C, coff):
    import torch
    import torch.nn.functional as F
    from cdnet_amd import _lib
    hs, ws = hw
    g = torch.Generator().manual_seed(4000 + 7 * hs + C + coff)
    dy = torch.randn((N, 4 * hs, 4 * ws, C), generator=g)
    dyd = _slice(dy, coff, torch.float32)
    dx = torch.full((N, hs, ws, _r8(C)), SENT, device='cuda')
    dy0 = dyd.clone()
    _lib.call('cdnet_upsample4_bilinear_backward', _lib.ptr(dyd), dyd.shape[3], coff, _lib.ptr(dx), dx.shape[3], N, hs, ws, C, _lib.stream_ptr())
    again = torch.full_like(dx, SENT)
    _lib.call('cdnet_upsample4_bilinear_backward', _lib.ptr(dyd), dyd.shape[3], coff, _lib.ptr(again), dx.shape[3], N, hs, ws, C, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(_raw(dyd), _raw(dy0)) and bool((dx[..., C:] == SENT).all())
    assert torch.equal(_raw(dx), _raw(again)), 'two runs differ'

    def ref(d):
        x = torch.zeros((N, C, hs, ws), dtype=torch.float64, requires_grad=True)
        F.interpolate(x, scale_factor=4, mode='bilinear', align_corners=True).backward(d.permute(0, 3, 1, 2).double())
        return x.grad.permute(0, 2, 3, 1)
    want, B = ref(dy), ref(dy.abs())
    err = (dx[..., :C].cpu().double() - want).abs()
    assert bool((B > 0).all())
    ratio = float((err / (2.0 ** -16 * B)).max())
    print('upsample backward %dx%d C %d coff %d: max err %.3g, worst err / bar %.4f' % (hs, ws, C, coff, float(err.max()), ratio))
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------------
# the existing entries at FCN_pooling's small maps: the checks of the two existing test modules, called on other shapes
SMALL_MAPS = [(2, 2, 3), (2, 1, 1)]
# (Cout, Cin, taps, d): a dense layer of the golden and of the default network at each dilation, a default transition
TRAIN_CASES = [(24, 40, 9, 1), (24, 129, 9, 13), (8, 40, 9, 21), (24, 256, 9, 21), (143, 286, 1, 1)]
_ID = lambda c: '%dto%d-t%d-d%d' % c


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@pytest.mark.parametrize('case', [(40, 24, 9, 1, 'slice'), (129, 24, 9, 13, 'inplace'), (256, 24, 9, 21, 'inplace'), (40, 8, 9, 21, 'affine'),
                                  (286, 143, 1, 1, 'slice'), (143, 3, 9, 1, 'nchw')], ids=lambda c: '%d-%d-t%d-d%d-%s' % c)
@pytest.mark.parametrize('shape', SMALL_MAPS, ids=lambda s: '%dx%dx%d' % s)
def test_dilated_forward_on_small_maps(shape, case, prec):
    import test_gpu_dilated_conv as dc
    dc._run(prec, shape, *case, seed=500 + sum(case[:4]))


@pytest.fixture
def small_map(request, monkeypatch):
    import test_gpu_fullnet_train_kernels as tk
    n, h, w = request.param
    for name, v in (('N', n), ('H', h), ('W', w), ('CASES', TRAIN_CASES), ('WGRAD_CASES', TRAIN_CASES)):
        monkeypatch.setattr(tk, name, v)
    return tk


_maps = pytest.mark.parametrize('small_map', SMALL_MAPS, ids=lambda s: '%dx%dx%d' % s, indirect=True)


@_maps
@pytest.mark.parametrize('accumulate', [0, 1], ids=['store', 'accumulate'])
@pytest.mark.parametrize('case', TRAIN_CASES, ids=_ID)
def test_backward_data_on_small_maps(small_map, case, accumulate):
    small_map.test_backward_data(case, accumulate)


@_maps
@pytest.mark.parametrize('kind', ['integers', 'random'])
@pytest.mark.parametrize('case', TRAIN_CASES, ids=_ID)
def test_weight_gradient_on_small_maps(small_map, case, kind):
    small_map.test_weight_gradient(case, kind)


@pytest.mark.parametrize('small_map', [(2, 2, 1), (2, 2, 3)], ids=['P4', 'P12'], indirect=True)
@pytest.mark.parametrize('p', [0.0, 0.1])
@pytest.mark.parametrize('Cc', [8, 24, 143])
def test_slice_bn_on_few_values(small_map, Cc, p):
    assert small_map.N * small_map.H * small_map.W in (4, 12)
    small_map.test_slice_bn_forward_and_backward(Cc, p)
