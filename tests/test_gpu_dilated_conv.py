"""cdnet_dilated_conv_forward (csrc/dilated.hip) per element against an fp64 conv2d, in both precisions.

Bounds are the project's own.  fp32 mode (tests/test_gpu_fp32.py): |got - want| <= 4e-5 (|x| conv |w|) |scale| + 1e-6.  bf16 mode
(tests/test_gpu_conv.py, same data scale: randn inputs, weights randn 1.5 / sqrt(K)): operands rounded to bf16 before the reference, then
|got - want| <= 2^-7 |want| + 2e-3.

Shapes: 2 x 40 x 36 (ragged against the 32-pixel strips and the 16 / 8-row groups, two images, more than one workgroup; at d = 21 taps lie
both inside and outside) and 1 x 13 x 13 with d = 16 (only the centre tap is ever inside).  Variants: 'plain' no epilogue, 'leaky',
'affine' leaky + scale / shift with negative scales, 'slice' a channel slice of a wider tensor whose other channels hold a sentinel,
'inplace' input and output in one tensor whose channels >= Cin start as NaN, 'nanpad' NaN in the input's channels [Cin, in_cstride),
'nchw' the fp32 [N][Cout][H][W] store of the final convolution."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

A, B = (2, 40, 36), (1, 13, 13)
CASES = [
    (A, 3, 24, 9, 1, 'affine'), (A, 3, 24, 9, 21, 'plain'), (A, 24, 24, 9, 1, 'inplace'), (A, 24, 24, 9, 21, 'inplace'),
    (A, 24, 24, 9, 2, 'leaky'), (A, 24, 24, 9, 7, 'affine'),
    (A, 168, 24, 9, 1, 'plain'), (A, 168, 24, 9, 1, 'leaky'), (A, 168, 24, 9, 1, 'affine'), (A, 168, 24, 9, 1, 'slice'),
    (A, 168, 24, 9, 1, 'inplace'), (A, 168, 24, 9, 1, 'nanpad'),
    (A, 168, 24, 9, 21, 'plain'), (A, 168, 24, 9, 21, 'leaky'), (A, 168, 24, 9, 21, 'affine'), (A, 168, 24, 9, 21, 'slice'),
    (A, 168, 24, 9, 21, 'inplace'), (A, 168, 24, 9, 21, 'nanpad'), (A, 168, 24, 9, 7, 'inplace'),
    (A, 129, 24, 9, 1, 'nanpad'), (A, 129, 24, 9, 21, 'inplace'), (A, 129, 24, 9, 2, 'affine'), (A, 129, 24, 9, 7, 'slice'),
    (A, 31, 8, 9, 1, 'inplace'), (A, 31, 8, 9, 21, 'nanpad'), (A, 31, 8, 9, 7, 'affine'), (A, 31, 8, 9, 2, 'slice'),
    (A, 286, 143, 1, 1, 'affine'), (A, 286, 143, 1, 1, 'slice'), (A, 286, 143, 1, 1, 'nanpad'),
    (A, 258, 129, 1, 1, 'affine'), (A, 258, 129, 1, 1, 'nanpad'),
    (A, 143, 3, 9, 1, 'plain'), (A, 143, 3, 9, 1, 'nchw'), (A, 143, 3, 9, 21, 'nanpad'),
    (B, 24, 24, 9, 16, 'affine'), (B, 168, 24, 9, 16, 'inplace'), (B, 129, 24, 9, 16, 'nanpad'), (B, 3, 24, 9, 1, 'leaky'),
    (B, 143, 3, 9, 16, 'nchw'), (B, 286, 143, 1, 1, 'slice'),
]
SENTINEL = 777.0            # bf16-exact


def _r8(c):
    return (c + 7) // 8 * 8


def _run(prec, shape, Cin, Cout, taps, d, variant, seed):
    import torch
    import torch.nn.functional as F
    from cdnet_amd import _lib
    f32 = prec == 'fp32'
    dt = torch.float32 if f32 else torch.bfloat16
    N, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((N, H, W, Cin), generator=g)
    w = torch.randn((Cout, Cin, 3, 3) if taps == 9 else (Cout, Cin, 1, 1), generator=g) * (1.5 / np.sqrt(Cin * taps))
    leaky = variant not in ('plain', 'nchw')
    affine = variant not in ('plain', 'leaky', 'nchw')
    scale = (0.5 + torch.rand(Cout, generator=g)) * torch.where(torch.arange(Cout) % 3 == 1, -1.0, 1.0)
    shift = 0.3 * torch.randn(Cout, generator=g)
    if not f32:
        x, w = x.bfloat16().float(), w.bfloat16().float()

    # the tensors the kernel sees
    if variant == 'inplace':
        cs = _r8(Cin + Cout + 3)
        buf = torch.full((N, H, W, cs), float('nan'))
        buf[..., :Cin] = x
        src = dst = buf.to(dt).cuda()
        ics = ocs = cs
        coff = Cin
    else:
        ics = _r8(Cin) + (8 if variant == 'nanpad' else 0)
        xin = torch.full((N, H, W, ics), float('nan') if variant == 'nanpad' else 0.0)
        xin[..., :Cin] = x
        src = xin.to(dt).cuda()
        if variant == 'nchw':
            dst, ocs, coff = torch.full((N, Cout, H, W), SENTINEL, dtype=torch.float32).cuda(), 0, 0
        elif variant == 'slice':
            ocs, coff = Cout + 13, 5
            dst = torch.full((N, H, W, ocs), SENTINEL, dtype=dt).cuda()
        else:
            ocs, coff = Cout, 0
            dst = torch.full((N, H, W, ocs), SENTINEL, dtype=dt).cuda()
    before = dst.clone()

    lib = _lib.load()
    wd = w.cuda().contiguous()
    wp = torch.empty(lib.cdnet_dilated_packed_weight_elems(Cin, Cout, taps, int(f32)), dtype=torch.bfloat16, device='cuda')
    _lib.call('cdnet_dilated_pack_weights', _lib.ptr(wd), _lib.ptr(wp), Cin, Cout, taps, int(f32), _lib.stream_ptr())
    sc, sh = scale.cuda(), shift.cuda()
    a = _lib.DilatedConvArgs()
    a.in_, a.w, a.out = src.data_ptr(), wp.data_ptr(), dst.data_ptr()
    a.scale, a.shift = (sc.data_ptr(), sh.data_ptr()) if affine else (None, None)
    a.N, a.H, a.W, a.Cin, a.in_cstride, a.Cout, a.out_cstride, a.out_coff = N, H, W, Cin, ics, Cout, ocs, coff
    a.taps, a.dilation, a.leaky, a.slope, a.f32, a.out_nchw = taps, d, int(leaky), 0.01, int(f32), int(variant == 'nchw')
    _lib.call('cdnet_dilated_conv_forward', C.byref(a), _lib.stream_ptr())
    torch.cuda.synchronize()

    # fp64 reference and the bound's |x| conv |w|
    pad, dil = (d, d) if taps == 9 else (0, 1)
    xn, wn = x.permute(0, 3, 1, 2).double(), w.double()
    if taps == 9 and d > 64:                   # (no tap but the centre one can be inside; conv2d would pad the image by d)
        assert d >= max(H, W)
        wn, pad, dil = wn[:, :, 1:2, 1:2], 0, 1
    want = F.conv2d(xn, wn, padding=pad, dilation=dil)
    mag = F.conv2d(xn.abs(), wn.abs(), padding=pad, dilation=dil)
    if leaky:
        want = F.leaky_relu(want, 0.01)
    if affine:
        want = want * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
        mag = mag * scale.double().abs().view(1, -1, 1, 1)

    out = dst.cpu()
    if variant == 'nchw':
        got = out.double()
    else:
        got = out[..., coff:coff + Cout].double().permute(0, 3, 1, 2)
        # nothing but the Cout channels of the slice was written
        raw = (lambda t: t.cpu().contiguous().view(torch.int32 if f32 else torch.int16))
        rb, ra = raw(before), raw(dst)
        assert torch.equal(rb[..., :coff], ra[..., :coff]), 'channels below out_coff changed'
        assert torch.equal(rb[..., coff + Cout:], ra[..., coff + Cout:]), 'channels above the slice changed'
    assert bool(torch.isfinite(got).all()), 'non-finite output (masking of channels >= Cin or of pixels outside the image)'
    err = (got - want).abs()
    tol = 4e-5 * mag + 1e-6 if f32 else want.abs() * 2 ** -7 + 2e-3
    bad = err > tol
    i = int(err.flatten().argmax())
    print('%s %s Cin %d Cout %d taps %d d %d %s: max err %.3g (tol there %.3g), worst err / tol %.3f'
          % (prec, shape, Cin, Cout, taps, d, variant, float(err.flatten()[i]), float(tol.flatten()[i]), float((err / tol).max())))
    assert not bool(bad.any()), '%d of %d elements out of tolerance, max err %g' % (int(bad.sum()), bad.numel(), float(err.max()))


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@pytest.mark.parametrize('case', CASES, ids=lambda c: '%dx%dx%d-%d-%d-t%d-d%d-%s' % (c[0] + c[1:]))
def test_dilated_conv(case, prec):
    _run(prec, *case, seed=CASES.index(case))


def test_large_dilation_reads_nothing_outside():
    """d far beyond H and W (and beyond what 32-bit pixel arithmetic of y + d * W would survive): the result is the centre tap's 1x1"""
    _run('fp32', B, 24, 24, 9, 1 << 30, 'affine', seed=99)
    _run('bf16', B, 24, 24, 9, 1 << 30, 'inplace', seed=98)
