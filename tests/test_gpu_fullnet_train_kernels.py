"""The FullNet training entries (csrc/dilated.hip, csrc/dilated_train.hip) per element against fp64, fp32 precision mode.

Shapes: N = 2, H = 9, W = 37 - ragged against the 32-pixel strips and the row groups, two images, more than one workgroup; at d = 21 > H
only the centre tap's row is ever inside.  Bounds:
  backward-data    the project's fp32 rule (tests/test_gpu_dilated_conv.py): 4e-5 (|g| conv |w|) + 1e-6, plus 2^-23 |prior + want| for the
                   one fp32 addition when accumulating;
  weight gradient  integers |v| <= 4: every product and every partial sum is an integer below 2^24, so fp32 is exact and the result equals
                   fp64 bit for bit; random inputs: 4e-5 sum |g| |x| + 1e-6 per element (the same rule, the sum over the pixels);
  BatchNorm        1e-5 relative to each tensor's largest magnitude: the statistics are fp32 sums of at most 11 terms per thread and 8 per
                   tile under an fp64 tree (666 terms in all, ~1e-6 relative at worst), every other step a handful of fp32 roundings.
                   The slice sits at offset 40 of a stride of 168; 143 channels do not fit behind 40 and sit at offset 5 (odd) instead.
At d = 21 the rows of taps above and below the centre reach no pixel (H = 9); the centre row's outer taps still do (W = 37 > 21)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, H, W = 2, 9, 37
# (Cout -> Cin, taps, d)
CASES = [(24, 3, 9, 1), (24, 168, 9, 3), (8, 40, 9, 21), (143, 286, 1, 1), (96, 24, 9, 2), (3, 143, 9, 1)]
WGRAD_CASES = CASES + [(24, 129, 9, 2)]
DX_STRIDE = 288
SENTINEL = 777.0
_ID = lambda c: '%dto%d-t%d-d%d' % c


def _r8(c):
    return (c + 7) // 8 * 8


@pytest.fixture(autouse=True)
def fp32_mode():
    import cdnet_amd
    before = cdnet_amd.get_precision()
    cdnet_amd.set_precision('fp32')
    yield
    cdnet_amd.set_precision(before)


def _conv_args(taps, d):
    return dict(padding=d, dilation=d) if taps == 9 else dict(padding=0, dilation=1)


@pytest.mark.parametrize('accumulate', [0, 1], ids=['store', 'accumulate'])
@pytest.mark.parametrize('case', CASES, ids=_ID)
def test_backward_data(case, accumulate):
    import torch
    import torch.nn.functional as F
    from cdnet_amd import _lib
    Cout, Cin, taps, d = case
    gen = torch.Generator().manual_seed(100 + CASES.index(case))
    k = 3 if taps == 9 else 1
    g = torch.randn((N, H, W, Cout), generator=gen)
    w = torch.randn((Cout, Cin, k, k), generator=gen) * (1.5 / np.sqrt(Cout * taps))
    gs = _r8(Cout) + 8
    gbuf = torch.full((N, H, W, gs), float('nan'))                  # NaN behind the Cout channels: selected away, never multiplied
    gbuf[..., :Cout] = g
    coff = 1 if Cin + 1 <= DX_STRIDE else 0
    prior = torch.randn((N, H, W, DX_STRIDE), generator=gen)
    prior[..., :coff] = SENTINEL
    prior[..., coff + Cin:] = SENTINEL
    lib = _lib.load()
    wd, gd, dx = w.cuda().contiguous(), gbuf.cuda(), prior.cuda()
    wp = torch.empty(lib.cdnet_dilated_packed_weight_elems(Cout, Cin, taps, 1), dtype=torch.bfloat16, device='cuda')
    _lib.call('cdnet_dilated_pack_weights_bwd', _lib.ptr(wd), _lib.ptr(wp), Cin, Cout, taps, 1, _lib.stream_ptr())
    a = _lib.DilatedBwdDataArgs()
    a.g, a.w, a.dx = gd.data_ptr(), wp.data_ptr(), dx.data_ptr()
    a.N, a.H, a.W, a.Cout, a.g_cstride, a.Cin, a.dx_cstride, a.dx_coff = N, H, W, Cout, gs, Cin, DX_STRIDE, coff
    a.taps, a.dilation, a.accumulate, a.f32 = taps, d, accumulate, 1
    _lib.call('cdnet_dilated_conv_backward_data', C.byref(a), _lib.stream_ptr())
    torch.cuda.synchronize()
    out = dx.cpu()

    gn, wn = g.permute(0, 3, 1, 2).double(), w.double()
    want = F.conv_transpose2d(gn, wn, **_conv_args(taps, d))         # the adjoint of conv2d(x, w): dx of include/cdnet_hip.h's formula
    mag = F.conv_transpose2d(gn.abs(), wn.abs(), **_conv_args(taps, d))
    assert want.shape == (N, Cin, H, W)
    tol = 4e-5 * mag + 1e-6
    if accumulate:
        p = prior[..., coff:coff + Cin].permute(0, 3, 1, 2).double()
        want = want + p
        tol = tol + 2.0 ** -23 * want.abs()
    got = out[..., coff:coff + Cin].permute(0, 3, 1, 2).double()
    raw = lambda t: t.contiguous().view(torch.int32)
    assert torch.equal(raw(out[..., :coff]), raw(prior[..., :coff])), 'channels below dx_coff changed'
    assert torch.equal(raw(out[..., coff + Cin:]), raw(prior[..., coff + Cin:])), 'channels above the slice changed'
    assert bool(torch.isfinite(got).all())
    err = (got - want).abs()
    print('backward-data %s acc %d: max err %.3g, worst err / tol %.3f' % (_ID(case), accumulate, float(err.max()), float((err / tol).max())))
    assert not bool((err > tol).any()), '%d elements out of tolerance, max err %g' % (int((err > tol).sum()), float(err.max()))


@pytest.mark.parametrize('f32', [0, 1], ids=['bf16', 'fp32'])
@pytest.mark.parametrize('case', [(24, 40, 9), (143, 286, 1), (3, 24, 9)], ids=lambda c: '%dto%d-t%d' % c)
def test_backward_pack_is_forward_pack_of_swapped_mirrored_weights(case, f32):
    """cdnet_dilated_pack_weights_bwd(w) == cdnet_dilated_pack_weights(w'), w'[ci][co][tap] = w[co][ci][taps - 1 - tap], bit for bit over the
    whole buffer (the two entries' index expressions; the zero padding of the ragged tiles on both sides included).  The buffers start
    from different fills, so an element that either entry leaves unwritten differs."""
    import torch
    from cdnet_amd import _lib
    Cout, Cin, taps = case
    k = 3 if taps == 9 else 1
    w = torch.randn((Cout, Cin, k, k), generator=torch.Generator().manual_seed(400 + Cout)).cuda()
    wt = w.permute(1, 0, 2, 3).flip(2, 3).contiguous()
    n = _lib.load().cdnet_dilated_packed_weight_elems(Cout, Cin, taps, f32)       # GEMM-K over Cout, GEMM-N over Cin
    assert n > 0
    bwd = torch.full((n,), 0x1111, dtype=torch.int16, device='cuda')
    fwd = torch.full((n,), 0x2222, dtype=torch.int16, device='cuda')
    _lib.call('cdnet_dilated_pack_weights_bwd', _lib.ptr(w), _lib.ptr(bwd), Cin, Cout, taps, f32, _lib.stream_ptr())
    _lib.call('cdnet_dilated_pack_weights', _lib.ptr(wt), _lib.ptr(fwd), Cout, Cin, taps, f32, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(bwd, fwd), '%d of %d packed elements differ' % (int((bwd != fwd).sum()), n)
    assert bool((bwd == 0).any()) and bool((bwd != 0).any())           # ragged tiles: the padding is there, and so are the weights


def _wgrad(x, g, Cin, Cout, taps, d, xs, gs, dw=None):
    """x [N,H,W,xs], g [N,H,W,gs] device tensors -> dW [Cout,Cin,k,k] from the device"""
    import torch
    from cdnet_amd import _lib
    lib = _lib.load()
    k = 3 if taps == 9 else 1
    need = lib.cdnet_dilated_wgrad_workspace_bytes(N, H, W, Cin, Cout, taps)
    assert need > 0
    ws = torch.full((need // 4,), float('nan'), device='cuda')       # the slabs are stored, not accumulated: NaN must not survive
    if dw is None:
        dw = torch.full((Cout, Cin, k, k), float('nan'), device='cuda')
    a = _lib.DilatedWgradArgs()
    a.x, a.g, a.dw, a.ws, a.ws_bytes = x.data_ptr(), g.data_ptr(), dw.data_ptr(), ws.data_ptr(), need
    a.N, a.H, a.W, a.Cin, a.x_cstride, a.Cout, a.g_cstride, a.taps, a.dilation = N, H, W, Cin, xs, Cout, gs, taps, d
    _lib.call('cdnet_dilated_conv_backward_weight', C.byref(a), _lib.stream_ptr())
    torch.cuda.synchronize()
    return dw


def _wgrad_want(x, g, taps, d):
    """fp64 dW and sum |g| |x| of NHWC fp64 CPU tensors, straight from include/cdnet_hip.h's formula"""
    import torch
    import torch.nn.functional as F
    Cin, Cout = x.shape[3], g.shape[3]
    k = 3 if taps == 9 else 1
    want = torch.zeros((Cout, Cin, k, k), dtype=torch.float64)
    mag = torch.zeros_like(want)
    for ky in range(k):
        for kx in range(k):
            oy, ox = ((ky - 1) * d, (kx - 1) * d) if taps == 9 else (0, 0)
            # xs[n, y, x] = x[n, y + oy, x + ox], zero outside
            xs = torch.zeros_like(x)
            y0, y1, x0, x1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
            if y0 < y1 and x0 < x1:
                xs[:, y0:y1, x0:x1] = x[:, y0 + oy:y1 + oy, x0 + ox:x1 + ox]
            want[:, :, ky, kx] = torch.einsum('nyxo,nyxi->oi', g, xs)
            mag[:, :, ky, kx] = torch.einsum('nyxo,nyxi->oi', g.abs(), xs.abs())
    return want, mag


@pytest.mark.parametrize('kind', ['integers', 'random'])
@pytest.mark.parametrize('case', WGRAD_CASES, ids=_ID)
def test_weight_gradient(case, kind):
    import torch
    Cout, Cin, taps, d = case
    gen = torch.Generator().manual_seed(200 + WGRAD_CASES.index(case))
    if kind == 'integers':
        x = torch.randint(-4, 5, (N, H, W, Cin), generator=gen).float()
        g = torch.randint(-4, 5, (N, H, W, Cout), generator=gen).float()
    else:
        x, g = torch.randn((N, H, W, Cin), generator=gen), torch.randn((N, H, W, Cout), generator=gen)
    xs, gs = 288 if Cin <= 288 else _r8(Cin), _r8(Cout)
    xb = torch.full((N, H, W, xs), float('nan'))                    # NaN in every channel of x behind Cin (padding and other layers' channels)
    xb[..., :Cin] = x
    gb = torch.full((N, H, W, gs), float('nan'))
    gb[..., :Cout] = g
    xd, gd = xb.cuda(), gb.cuda()
    got = _wgrad(xd, gd, Cin, Cout, taps, d, xs, gs)
    again = _wgrad(xd, gd, Cin, Cout, taps, d, xs, gs)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), 'two runs differ'
    got = got.cpu().double()
    assert bool(torch.isfinite(got).all()), 'NaN from the padding channels reached dW'
    want, mag = _wgrad_want(x.double(), g.double(), taps, d)
    if d > H and taps == 9:
        off = got.clone()
        off[:, :, 1, :] = 0                                        # at d = 21 > H = 9 only the centre row of taps reaches a pixel ...
        assert not bool(off.any())
        assert bool(got[:, :, 1, 1].any()) and bool(want[:, :, 1, 1].any())
        if d >= W:
            assert not bool(got[:, :, 1, 0].any()) and not bool(got[:, :, 1, 2].any())       # ... and of it the centre tap alone
    err = (got - want).abs()
    if kind == 'integers':
        print('weight gradient %s integers: max |dW| %g, max err %g' % (_ID(case), float(want.abs().max()), float(err.max())))
        assert float(want.abs().max()) < 2 ** 24
        assert torch.equal(got, want), 'max err %g' % float(err.max())
    else:
        tol = 4e-5 * mag + 1e-6
        print('weight gradient %s random: max err %.3g, worst err / tol %.3f' % (_ID(case), float(err.max()), float((err / tol).max())))
        assert not bool((err > tol).any()), '%d elements out of tolerance, max err %g' % (int((err > tol).sum()), float(err.max()))


def _mask(key, layer, count, p):
    import torch
    from cdnet_amd import _lib
    m = torch.empty((count,), dtype=torch.uint8, device='cuda')
    _lib.call('cdnet_dropout_mask', key, layer, count, p, _lib.ptr(m), _lib.stream_ptr())
    return m


@pytest.mark.parametrize('p', [0.0, 0.1])
@pytest.mark.parametrize('Cc', [8, 24, 143])
def test_slice_bn_forward_and_backward(Cc, p):
    import torch
    from cdnet_amd import _lib
    lib = _lib.load()
    P, stride, coff, key, layer = N * H * W, 168, 40 if Cc + 40 <= 168 else 5, 0x1234567800000007, 11
    gen = torch.Generator().manual_seed(300 + Cc)
    zs = _r8(Cc)
    z = torch.randn((P, Cc), generator=gen) * (0.5 + torch.rand(Cc, generator=gen)) + 0.3 * torch.randn(Cc, generator=gen)
    z = torch.where(z > 0, z, 0.01 * z)
    gamma = 0.5 + torch.rand(Cc, generator=gen)
    gamma[1], gamma[2] = -gamma[1], 0.0
    beta = 0.1 * torch.randn(Cc, generator=gen)
    rm, rv = 0.1 * torch.randn(Cc, generator=gen), 0.5 + torch.rand(Cc, generator=gen)
    dy = torch.randn((P, stride), generator=gen)
    zb = torch.full((P, zs), float('nan'))
    zb[:, :Cc] = z
    out0 = torch.full((P, stride), SENTINEL)
    ws = torch.empty((lib.cdnet_slice_bn_workspace_floats(P, Cc),), device='cuda')
    zd, out, gd, bd, rmd, rvd = zb.cuda(), out0.cuda(), gamma.cuda(), beta.cuda(), rm.cuda(), rv.cuda()
    mean, invstd = torch.empty(Cc, device='cuda'), torch.empty(Cc, device='cuda')
    a = _lib.SliceBnFwdArgs()
    a.z, a.out, a.gamma, a.beta, a.running_mean, a.running_var = (t.data_ptr() for t in (zd, out, gd, bd, rmd, rvd))
    a.mean, a.invstd, a.ws, a.ws_floats = mean.data_ptr(), invstd.data_ptr(), ws.data_ptr(), ws.numel()
    a.P, a.C, a.z_cstride, a.out_cstride, a.out_coff = P, Cc, zs, stride, coff
    a.eps, a.momentum, a.p_drop, a.layer, a.key = 1e-5, 0.1, p, layer, key
    _lib.call('cdnet_slice_bn_train_forward', C.byref(a), _lib.stream_ptr())
    dyd = dy.cuda()
    g = torch.full((P, zs), SENTINEL, device='cuda')
    dgamma, dbeta = torch.empty(Cc, device='cuda'), torch.empty(Cc, device='cuda')
    b = _lib.SliceBnBwdArgs()
    b.dy, b.z, b.mean, b.invstd, b.gamma = dyd.data_ptr(), zd.data_ptr(), mean.data_ptr(), invstd.data_ptr(), gd.data_ptr()
    b.dgamma, b.dbeta, b.g, b.ws, b.ws_floats = dgamma.data_ptr(), dbeta.data_ptr(), g.data_ptr(), ws.data_ptr(), ws.numel()
    b.P, b.C, b.z_cstride, b.dy_cstride, b.dy_coff, b.g_cstride = P, Cc, zs, stride, coff, zs
    b.slope, b.p_drop, b.layer, b.key = 0.01, p, layer, key
    _lib.call('cdnet_slice_bn_train_backward', C.byref(b), _lib.stream_ptr())
    m = _mask(key, layer, P * Cc, p).cpu().view(P, Cc).double() if p > 0 else torch.ones((P, Cc), dtype=torch.float64)
    torch.cuda.synchronize()

    z64 = z.double()
    mu, var = z64.mean(0), z64.var(0, unbiased=False)
    istd = 1.0 / torch.sqrt(var + 1e-5)
    xhat = (z64 - mu) * istd
    keep = m / (1.0 - p)
    y = (xhat * gamma.double() + beta.double()) * keep
    dyh = dy[:, coff:coff + Cc].double() * keep
    dbeta_w, dgamma_w = dyh.sum(0), (dyh * xhat).sum(0)
    dz = gamma.double() * istd * (dyh - dbeta_w / P - xhat * dgamma_w / P)
    g_w = dz * torch.where(z64 > 0, 1.0, 0.01)
    pairs = {
        'mean': (mean, mu), 'invstd': (invstd, istd), 'running_mean': (rmd, 0.9 * rm.double() + 0.1 * mu),
        'running_var': (rvd, 0.9 * rv.double() + 0.1 * var * P / (P - 1)), 'y': (out[:, coff:coff + Cc], y),
        'dgamma': (dgamma, dgamma_w), 'dbeta': (dbeta, dbeta_w), 'g': (g[:, :Cc], g_w),
    }
    for name, (got, want) in pairs.items():
        err = float((got.cpu().double() - want).abs().max()) / float(want.abs().max())
        print('slice bn C %d p %g %s: relative error %.3g' % (Cc, p, name, err))
        assert err <= 1e-5, (name, err)
    o = out.cpu()
    raw = lambda t: t.contiguous().view(torch.int32)
    assert torch.equal(raw(o[:, :coff]), raw(out0[:, :coff])) and torch.equal(raw(o[:, coff + Cc:]), raw(out0[:, coff + Cc:]))
    assert torch.equal(raw(g.cpu()[:, Cc:]), raw(torch.full((P, zs - Cc), SENTINEL)))
    if p > 0:
        # the mask of cdnet_dropout_mask is the one the forward applied (no y is zero by itself: gamma = 0 has beta != 0)
        assert torch.equal(o[:, coff:coff + Cc] == 0, m == 0)


def test_dropout_mask_statistics():
    import torch
    n, key = 1 << 20, 0x00000007000000a1
    for p in (0.1, 0.5):
        kept = float(_mask(key, 3, n, p).double().mean())
        assert abs(kept - (1 - p)) <= 5 * np.sqrt(p * (1 - p) / n), (p, kept)
    assert bool(_mask(key, 3, n, 0.0).all())
    a, b, c = _mask(key, 3, n, 0.1), _mask(key, 4, n, 0.1), _mask(key + 1, 3, n, 0.1)
    assert torch.equal(a, _mask(key, 3, n, 0.1))
    # another layer / another step: independent masks agree on ~ (0.9^2 + 0.1^2) of the elements, not on all of them
    for other in (b, c):
        agree = float((a == other).double().mean())
        assert abs(agree - 0.82) < 0.01, agree
    # independent of the launch geometry: a prefix of a longer mask is the shorter mask
    assert torch.equal(_mask(key, 3, 1000, 0.1), a[:1000])
