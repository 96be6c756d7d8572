"""conv1x1_f32_stream_kernel (csrc/conv32.hip): the halo-free streaming form of the fp32-mode 1x1 convolution over one dense source,
against conv_f32_kernel (cdnet_conv_args.debug bit 256 keeps a launch on it) and against an fp64 conv2d.  The two kernels issue the
same MFMA sequence per accumulator, the same source transform and the same epilogue, so their outputs agree bit for bit; both lie within
the fp32-MFMA bound of 5e-5 of the output scale (2^-16 per product).

Shapes: (2, 16, 16) full 16 x 16 tiles (the old kernel's fast epilogue); (1, 24, 20) ragged tiles, the pixel count a multiple of 32;
(3, 5, 7) = 105 pixels, three full blocks of 32 and a tail block of 9.  Channels: 32 / 64 (two and four chunks; one block of 32 or 64 output
channels), and beside them the residual units' own edge shapes: 16 input channels (one chunk), 16 output channels (half a channel block: lanes
without a channel), 64 output channels in two blocks of 32."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

OLD = 256          # cdnet_conv_args.debug: conv_f32_kernel also where the streaming kernel applies

SHAPES = [(2, 16, 16), (1, 24, 20), (3, 5, 7)]
CHANS = [(32, 32, 32), (32, 64, 64), (64, 32, 32), (64, 64, 64),          # (Cin, Cout, BN)
         (16, 64, 64), (64, 16, 32), (32, 64, 32)]
VARIANTS = ['plain', 'xf', 'fold', 'eres', 'slice']


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().float().cuda()


def _case(shape, chans, variant):
    """(launch(debug) -> NHWC output on the device, fp64 NHWC reference)"""
    import torch
    import torch.nn.functional as F
    from cdnet_amd import _lib, engine
    N, H, W = shape
    Cin, Cout, BN = chans
    g = torch.Generator().manual_seed(1000 * Cin + 10 * Cout + H + VARIANTS.index(variant))
    x = torch.randn((N, Cin, H, W), generator=g)
    w = torch.randn((Cout, Cin, 1, 1), generator=g) * (1.5 / Cin ** 0.5)
    cfg = (16, 16, BN)
    wp = engine.pack_weights(w.cuda(), cfg, 0, split=True)
    t, src = x.double(), engine.Src(_nhwc(x))
    if variant == 'xf':                                            # BatchNorm scale / shift + ReLU pending on the source
        sc, sh = torch.rand((Cin,), generator=g) + 0.5, torch.randn((Cin,), generator=g) * 0.3
        t = F.relu(x.double() * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1))
        src = engine.Src(_nhwc(x), sc.cuda(), sh.cuda(), relu=True)
    want = F.conv2d(t, w.double())
    kw = {}
    if variant == 'fold':                                          # bias + folded BatchNorm + ReLU in the epilogue
        bias, osc, osh = torch.randn((Cout,), generator=g) * 0.1, torch.rand((Cout,), generator=g) + 0.5, torch.randn((Cout,), generator=g) * 0.2
        want = F.relu((want + bias.double().view(1, -1, 1, 1)) * osc.double().view(1, -1, 1, 1) + osh.double().view(1, -1, 1, 1))
        kw = dict(bias=bias.cuda(), oscale=osc.cuda(), oshift=osh.cuda(), orelu=True)
    if variant == 'eres':                                          # the residual unit's forward: relu(bn2(other branch) + conv_1x1(x) + bias)
        bias = torch.randn((Cout,), generator=g) * 0.1
        e = torch.randn((N, Cout, H, W), generator=g)
        esc, esh = torch.rand((Cout,), generator=g) + 0.5, torch.randn((Cout,), generator=g) * 0.3
        want = F.relu(e.double() * esc.double().view(1, -1, 1, 1) + esh.double().view(1, -1, 1, 1) + want + bias.double().view(1, -1, 1, 1))
        kw = dict(bias=bias.cuda(), eres=engine.Src(_nhwc(e), esc.cuda(), esh.cuda(), relu=True))
    ref = want.permute(0, 2, 3, 1).contiguous()

    def launch(debug):
        if variant == 'slice':                                     # channels [coff, coff + Cout) of a wider tensor, the rest untouched
            cs, coff = Cout + 48, 16
            out = torch.full((N, H, W, cs), 7.0, dtype=torch.float32, device='cuda')
            a = engine.ConvArgs()
            src.fill(a.src[0])
            a.nsrc, a.w = 1, wp.data_ptr()
            a.out, a.Cout, a.out_cstride, a.out_coff = out.data_ptr(), Cout, cs, coff
            a.N, a.H, a.W, a.taps, a.npar, a.ostride, a.nchunk = N, H, W, 1, 1, 1, Cin // 16
            a.tile, a.CK, a.BN, a.f32, a.debug = cfg[0], cfg[1], cfg[2], 1, debug
            _lib.call('cdnet_conv_forward', C.byref(a), _lib.stream_ptr())
            torch.cuda.synchronize()
            assert bool((out[..., :coff] == 7.0).all()) and bool((out[..., coff + Cout:] == 7.0).all()), 'bytes outside the slice changed'
            return out[..., coff:coff + Cout].clone()
        out = torch.full((N, H, W, Cout), 7.0, dtype=torch.float32, device='cuda')
        got, _ = engine.conv_forward([src], wp, Cout, cfg, taps=1, out=out, H=H, W=W, debug_or=debug, **kw)
        torch.cuda.synchronize()
        return got.clone()

    return launch, ref


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('chans', CHANS)
@pytest.mark.parametrize('shape', SHAPES)
def test_conv1x1_stream_matches_conv_f32_and_fp64(shape, chans, variant):
    import torch
    launch, ref = _case(shape, chans, variant)
    old, new = launch(OLD), launch(0)
    scale = float(ref.abs().max())
    for name, got in (('conv_f32_kernel', old), ('conv1x1_f32_stream_kernel', new)):
        err = float((got.double().cpu() - ref).abs().max()) / scale
        assert err < 5e-5, (name, err)
    assert torch.equal(old, new), 'conv1x1_f32_stream_kernel differs from conv_f32_kernel'


@pytest.mark.parametrize('shape', SHAPES)
def test_conv1x1_stream_declines_a_source_with_residual(shape):
    """relu(x * scale + shift + res) as the source is not the streaming kernel's: the launch stays on conv_f32_kernel, with or without bit 256"""
    import torch
    import torch.nn.functional as F
    from cdnet_amd import engine
    N, H, W = shape
    Cin, Cout, cfg = 64, 64, (16, 16, 64)
    g = torch.Generator().manual_seed(77 + H)
    x, r = torch.randn((N, Cin, H, W), generator=g), torch.randn((N, Cin, H, W), generator=g)
    sc, sh = torch.rand((Cin,), generator=g) + 0.5, torch.randn((Cin,), generator=g) * 0.3
    w = torch.randn((Cout, Cin, 1, 1), generator=g) * (1.5 / Cin ** 0.5)
    wp = engine.pack_weights(w.cuda(), cfg, 0, split=True)
    src = engine.Src(_nhwc(x), sc.cuda(), sh.cuda(), relu=True, res=_nhwc(r))
    want = F.conv2d(F.relu(x.double() * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1) + r.double()), w.double())
    ref = want.permute(0, 2, 3, 1).contiguous()
    outs = []
    for debug in (OLD, 0):
        got, _ = engine.conv_forward([src], wp, Cout, cfg, taps=1, H=H, W=W, debug_or=debug)
        torch.cuda.synchronize()
        outs.append(got.clone())
        assert float((got.double().cpu() - ref).abs().max()) / float(ref.abs().max()) < 5e-5
    assert torch.equal(outs[0], outs[1])
