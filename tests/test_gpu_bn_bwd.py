"""BatchNorm-backward kernels (bn_bwd.hip) path by path against CPU autograd, with the tolerances of _bn_cases.py: the flat kernels
(every gradient source same-size and un-shifted) for 1 - 3 sources with and without residual in every storage format, the ReLU modes
0 and 2, the 16-bit window kernel with flat sources, channel counts where 256 is no multiple of the threads per pixel, a layer
without BatchNorm, and the split entries (stats / finalize / apply) bit for bit against cdnet_bn_backward.

Shape: N = 2, 13 x 21 pixels, 32 channels = 546 pixels: three workgroups, a ragged last one, clamped tail loads; odd height and
width leave a last window row / column without a pooled gradient."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bn_cases as bc  # noqa: E402

pytestmark = pytest.mark.gpu
SIZE = (13, 21)


@pytest.mark.parametrize('with_res', [False, True])
@pytest.mark.parametrize('ngin', [1, 2, 3])
@pytest.mark.parametrize('fmt', ['f16', 'bf16', 'f32'])
def test_flat(fmt, ngin, with_res):
    """with a residual the sums pass stores dz and the apply pass reads it as its only source"""
    bc.bn_case(fmt, False, with_res, False, seed=21 + ngin, plain=ngin, size=SIZE)


@pytest.mark.parametrize('fmt', ['f16', 'bf16'])
def test_flat_mask_from_stored_output(fmt):
    """relu = 2: `res` is the stored output of the unit (HRNet's fused residual sums)"""
    bc.bn_case(fmt, False, True, False, seed=31, outmask=True, size=SIZE)


@pytest.mark.parametrize('fmt', ['f16', 'f32'])
def test_flat_masked_source(fmt):
    """relu = 0 with one plain source: what trainer._bn_backward_masked issues"""
    bc.bn_case(fmt, False, False, False, seed=32, plain=1, relu=0, size=SIZE)


@pytest.mark.parametrize('pool_first', [True, False])
@pytest.mark.parametrize('nflat', [1, 2])
def test_window_16bit(nflat, pool_first):
    bc.bn_case('f16', True, False, False, seed=33 + nflat, skip=nflat, size=SIZE, pool_first=pool_first)


@pytest.mark.parametrize('flat', [True, False])
@pytest.mark.parametrize('fmt', ['f16', 'f32'])
def test_48_channels(fmt, flat):
    """HRNet's widths: 6 (16-bit) / 12 (fp32 flat) threads per pixel, the last threads of a workgroup sit the loop out; not flat: the
    source comes through F.pad offsets as a channel slice (generic kernels)"""
    bc.bn_case(fmt, False, False, False, seed=36, plain=1 if flat else 0, Cc=48, size=SIZE)


@pytest.mark.parametrize('fmt', ['f16', 'f32'])
def test_layer_without_batchnorm(fmt):
    """mean / scale NULL: the apply pass alone, dRaw = the summed sources behind the ReLU mask"""
    bc.bn_case(fmt, False, False, False, seed=37, plain=2, bn=False, size=SIZE)


def test_split_entries_match_the_fused_call():
    """cdnet_bn_backward_stats + _apply, and cdnet_bn_backward_finalize + _apply over the partial rows that _stats left, run the same
    kernels in the same grid as cdnet_bn_backward on the plain 16-bit case: equal bits"""
    import torch
    from cdnet_amd import _lib
    c = bc.build('f16', False, False, False, seed=38, plain=1, size=SIZE)
    draw0, _, dgamma0, dbeta0 = bc.run(c)
    bc.check(c, draw0, None, dgamma0, dbeta0)
    N, H, W, Cc = c.shape
    nb = bc.grid_rows(N * H * W, Cc)
    ws = torch.zeros((nb * 2 * Cc,), dtype=torch.float32, device='cuda')

    def apply(ktab):
        draw = torch.zeros_like(draw0)
        _lib.call('cdnet_bn_backward_apply', C.byref(c.A), _lib.ptr(ktab), _lib.ptr(draw), _lib.stream_ptr())
        return draw

    ktab = torch.zeros((7, Cc), dtype=torch.float32, device='cuda')
    dgamma, dbeta = torch.zeros(Cc, device='cuda'), torch.zeros(Cc, device='cuda')
    _lib.call('cdnet_bn_backward_stats', C.byref(c.A), _lib.ptr(c.gamma), _lib.ptr(dgamma), _lib.ptr(dbeta), _lib.ptr(ws), ws.numel(),
              _lib.ptr(ktab), _lib.stream_ptr())
    draw = apply(ktab)
    assert torch.equal(dgamma, dgamma0) and torch.equal(dbeta, dbeta0) and torch.equal(draw, draw0)
    sc, sh, mu, iv = c.keep[2:6]
    assert torch.equal(ktab[:4], torch.stack([sc, sh, mu, iv]))

    ktab2 = torch.zeros_like(ktab)
    dgamma2, dbeta2 = torch.zeros(Cc, device='cuda'), torch.zeros(Cc, device='cuda')
    _lib.call('cdnet_bn_backward_finalize', C.byref(c.A), _lib.ptr(c.gamma), _lib.ptr(dgamma2), _lib.ptr(dbeta2), _lib.ptr(ws), nb,
              _lib.ptr(ktab2), _lib.stream_ptr())
    draw2 = apply(ktab2)
    assert torch.equal(ktab2[4:], ktab[4:]) and not ktab2[:4].any()
    assert torch.equal(dgamma2, dgamma0) and torch.equal(dbeta2, dbeta0) and torch.equal(draw2, draw0)
