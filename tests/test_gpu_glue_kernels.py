"""Kernel-level tests of the streaming "glue" kernels of HRNet training (csrc/model.hip: cdnet_fuse_sum, cdnet_upsample_bilinear_backward,
cdnet_s2d_to_nhwc, cdnet_grad_sum, each with its _f32 twin) and of the UNet bias gradient (csrc/head_bwd.hip: cdnet_bias_grad[_f32]) through
the C ABI, against fp64 references built on the CPU.  Inputs, references and the derivation of every bound: tests/_glue_cases.py.

Exact-input cases (small integers, dyadic scales and weights) demand equality; real-input cases a per-element bound counted from the
roundings.  Outputs are allocated filled with a sentinel, with the channels outside an output slice and one guard row after the end
checked; N = 2 and low-resolution terms of another Hs * Ws than the output show a wrong batch stride.  Every launcher caps its grid,
so one case per kernel is large enough for the grid-stride loop to take a second trip (more than 4096 * 256 vectors; 512 workgroups
for the bias gradient); those are exact-input cases."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _glue_cases as gc  # noqa: E402

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------
# cdnet_fuse_sum / cdnet_fuse_sum_f32
# ------------------------------------------------------------------------------------------------------
def fuse_terms(nterm, H, W, f32):
    """1..4 terms (each count is its own fuse_sum16_kernel<NT>): same-size terms, x2 / x4 / x8, one with Hs == H but Ws == W / 2, one
    1 x 1; bf16 and fp16 storage (fp32 for the f32 entry), each with and without scale / shift"""
    a, b = ('f32', 'f32') if f32 else ('bf16', 'f16')
    return {1: [(H // 2, W // 2, a, False)],
            2: [(H, W, a, False), (H // 4, W // 4, b, True)],
            3: [(H, W, b, False), (H, W // 2, a, True), (H // 8, W // 8, b, False)],
            4: [(H // 2, W // 2, a, True), (H, W, b, True), (1, 1, a, False), (H // 4, W // 4, b, False)]}[nterm]


@pytest.mark.parametrize('sliced', [False, True])
@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('Cc', [8, 48, 144])
@pytest.mark.parametrize('nterm', [1, 2, 3, 4])
@pytest.mark.parametrize('f32', [False, True])
def test_fuse_sum_exact(f32, nterm, Cc, relu, sliced):
    H, W = (16, 32) if nterm == 4 else (16, 24)            # the 1 x 1 term needs a power-of-two width for dyadic weights
    got, ref, _ = gc.fuse_case(f32, 2, H, W, Cc, fuse_terms(nterm, H, W, f32), relu, sliced, True, seed=100 + nterm)
    gc.assert_exact(got, ref, f32, 'fuse_sum')


@pytest.mark.parametrize('sliced', [False, True])
@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('Cc', [8, 48, 144])
@pytest.mark.parametrize('nterm', [1, 2, 3, 4])
@pytest.mark.parametrize('f32', [False, True])
def test_fuse_sum_real(f32, nterm, Cc, relu, sliced):
    got, ref, e = gc.fuse_case(f32, 2, 16, 24, Cc, fuse_terms(nterm, 16, 24, f32), relu, sliced, False, seed=200 + nterm)
    gc.assert_close(got, ref, e, f32, 'fuse_sum')


@pytest.mark.parametrize('f32', [False, True])
def test_fuse_sum_same_size_term_with_affine_alone(f32):
    """one same-size term with its BatchNorm affine and ReLU: trainer's `_plain` (fuse_sum16_kernel<1> without interpolation)"""
    s = 'f32' if f32 else 'f16'
    got, ref, _ = gc.fuse_case(f32, 2, 16, 24, 48, [(16, 24, s, True)], 1, False, True, seed=7)
    gc.assert_exact(got, ref, f32, 'fuse_sum one term')


@pytest.mark.parametrize('shape', [(12, 7, [(12, 7, 0, False), (5, 3, 1, True), (1, 1, 0, True)]),       # 5 -> 12 rows, 3 -> 7 columns
                                   (6, 7, [(1, 3, 1, False), (6, 7, 0, True)]),                          # 1 -> 6 rows
                                   (12, 7, [(5, 7, 0, False), (12, 3, 1, True), (5, 3, 0, False), (12, 7, 1, False)])])
@pytest.mark.parametrize('f32', [False, True])
def test_fuse_sum_ragged_ratios(f32, shape):
    H, W, spec = shape
    st = ('f32', 'f32') if f32 else ('bf16', 'f16')
    terms = [(hs, ws, st[k], aff) for hs, ws, k, aff in spec]
    for Cc, relu, sliced in ((8, 0, True), (48, 1, False)):
        got, ref, e = gc.fuse_case(f32, 2, H, W, Cc, terms, relu, sliced, False, seed=300 + H)
        gc.assert_close(got, ref, e, f32, 'fuse_sum ragged C=%d' % Cc)


@pytest.mark.parametrize('f32', [False, True])
def test_fuse_sum_grid_stride(f32):
    """384 x 384 x 64: 1 179 648 vectors against the launcher's 4096 * 256"""
    a, b = ('f32', 'f32') if f32 else ('bf16', 'f16')
    got, ref, _ = gc.fuse_case(f32, 1, 384, 384, 64, [(192, 192, a, True), (384, 384, b, False)], 1, False, True, seed=9)
    gc.assert_exact(got, ref, f32, 'fuse_sum grid stride')


def _fuse_refusal(entry_f32, mutate, N=2, H=16, W=24, Cc=16, out_cstride=0, out_coff=0):
    import torch
    from cdnet_amd import _lib
    from cdnet_amd.runtime import FuseTerm
    dt = torch.float32 if entry_f32 else torch.bfloat16
    x = torch.ones((2 * 32 * 32 * 32,), dtype=dt, device='cuda')
    sc = torch.ones((32,), dtype=torch.float32, device='cuda')
    arr = (FuseTerm * 1)()
    arr[0].x, arr[0].Hs, arr[0].Ws, arr[0].f16 = x.data_ptr(), 8, 12, 2 if entry_f32 else 0
    mutate(arr[0], sc)
    out = gc.sentinel_buffer(2 * 16 * 24, 32, 0, dt)
    with pytest.raises(_lib.CdnetHipError):
        _lib.call('cdnet_fuse_sum_f32' if entry_f32 else 'cdnet_fuse_sum', C.byref(arr), 1, N, H, W, Cc, 0, _lib.ptr(out), out_cstride, out_coff,
                  _lib.stream_ptr())
    torch.cuda.synchronize()
    assert gc.untouched(out)


def test_fuse_sum_refusals():
    def nothing(t, sc):
        pass

    def sixteen_bit(t, sc):
        t.f16 = 1

    def fp32_term(t, sc):
        t.f16 = 2

    def scale_only(t, sc):
        t.scale = sc.data_ptr()

    def taller(t, sc):
        t.Hs = 17
    _fuse_refusal(True, sixteen_bit)                       # a 16-bit term passed to the f32 entry
    _fuse_refusal(False, fp32_term)                        # and the reverse
    _fuse_refusal(False, scale_only)                       # scale without shift
    _fuse_refusal(True, scale_only)
    _fuse_refusal(False, taller)                           # Hs > H
    _fuse_refusal(False, nothing, Cc=12)
    _fuse_refusal(True, nothing, Cc=12)
    _fuse_refusal(False, nothing, Cc=16, out_cstride=32, out_coff=24)          # out_coff + C > out_cstride
    # 2^31 output vectors or more: the 16-bit kernels index in 32 bits (by argument only; nothing of that size exists)
    _fuse_refusal(False, nothing, N=1 << 15, H=1 << 10, W=1 << 10, Cc=8)


# ------------------------------------------------------------------------------------------------------
# cdnet_upsample_bilinear_backward / _f32
# ------------------------------------------------------------------------------------------------------
EXACT_UP = [(8, 12, 16, 24), (4, 6, 16, 24), (2, 3, 16, 24), (4, 6, 16, 12), (16, 12, 16, 24), (1, 1, 8, 16)]
RAGGED_UP = [(8, 5, 57, 6), (7, 10, 8, 37), (4, 6, 5, 13), (5, 5, 6, 11), (1, 1, 5, 3)]


@pytest.mark.parametrize('sliced', [False, True])
@pytest.mark.parametrize('Cc', [8, 48])
@pytest.mark.parametrize('shape', EXACT_UP)
@pytest.mark.parametrize('f32', [False, True])
def test_upsample_backward_exact(f32, shape, Cc, sliced):
    """ratios 2 / 4 / 8, another ratio per axis, Hs == H with Ws < W, a 1 x 1 source"""
    Hs, Ws, H, W = shape
    got, ref, _ = gc.upsample_bwd_case(f32, 2, Hs, Ws, H, W, Cc, sliced, True, seed=400 + Hs)
    gc.assert_exact(got.double(), ref.double(), f32, 'upsample_bwd %s' % (shape,))


@pytest.mark.parametrize('shape', RAGGED_UP + [(4, 6, 16, 24)])
@pytest.mark.parametrize('f32', [False, True])
def test_upsample_backward_real_and_ragged(f32, shape):
    """ratios that are no integers: the window of candidate rows [(ys - 1) r, (ys + 2) r) with r = ceil(H / Hs) of the first version of
    this kernel missed contributing rows or whole source rows at these shapes (fp32 entry, worst |error| 6.7 at (8, 5, 57, 6), 5.7 at
    (7, 10, 8, 37), 2.0 at (4, 6, 5, 13), 4.3 at (5, 5, 6, 11): 8 000 to 18 000 times the bound)"""
    Hs, Ws, H, W = shape
    for Cc, sliced in ((8, True), (48, False)):
        got, ref, e = gc.upsample_bwd_case(f32, 2, Hs, Ws, H, W, Cc, sliced, False, seed=500 + H)
        gc.assert_close(got.double(), ref, e, f32, 'upsample_bwd %s C=%d' % (shape, Cc))


def test_upsample_backward_grid_stride():
    """4 x 96 x 96 x 256 / 8 = 1 179 648 threads' worth of work; the fp32 CPU reference is exact on these inputs"""
    import torch
    got, ref, _ = gc.upsample_bwd_case(False, 4, 96, 96, 192, 192, 256, False, True, seed=11, ref_dtype=torch.float32)
    want = ref.to(torch.bfloat16).float()
    assert torch.equal(got, want), '%d elements differ' % int((got != want).sum())


def test_upsample_backward_refusals():
    import torch
    from cdnet_amd import _lib
    d = torch.ones((2 * 16 * 24 * 16,), dtype=torch.bfloat16, device='cuda')
    for (Cc, cs, co, Hs, Ws) in ((12, 0, 0, 4, 6), (8, 16, 16, 4, 6), (8, 0, 0, 17, 6), (8, 0, 0, 4, 25)):
        din = gc.sentinel_buffer(2 * 17 * 25, 16, 0, torch.bfloat16)
        with pytest.raises(_lib.CdnetHipError):
            _lib.call('cdnet_upsample_bilinear_backward', _lib.ptr(d), 2, 16, 24, Cc, cs, co, Hs, Ws, _lib.ptr(din), _lib.stream_ptr())
        torch.cuda.synchronize()
        assert gc.untouched(din)


# ------------------------------------------------------------------------------------------------------
# cdnet_s2d_to_nhwc / _f32: a pure permutation, compared as integers
# ------------------------------------------------------------------------------------------------------
def _s2d(f32, N, H2, W2, Cc):
    import torch
    from cdnet_amd import _lib
    it = torch.int32 if f32 else torch.int16
    g = torch.Generator().manual_seed(H2 * 131 + Cc)
    x = torch.randint(-30000, 30000, (N, H2, W2, 2, 2, Cc), generator=g, dtype=it)          # [n][y2][x2][(a, b, c)]
    want = x.permute(0, 1, 3, 2, 4, 5).reshape(N * 2 * H2 * 2 * W2, Cc)
    out = torch.full((N * 2 * H2 * 2 * W2 + 2 * W2, Cc), 4096, dtype=it, device='cuda')
    xd = x.cuda()
    _lib.call('cdnet_s2d_to_nhwc_f32' if f32 else 'cdnet_s2d_to_nhwc', _lib.ptr(xd), N, H2, W2, Cc, _lib.ptr(out), _lib.stream_ptr())
    torch.cuda.synchronize()
    o = out.cpu()
    assert (o[want.shape[0]:] == 4096).all(), 'wrote past the end'
    assert torch.equal(o[:want.shape[0]], want)


@pytest.mark.parametrize('size', [(3, 5), (8, 8)])
@pytest.mark.parametrize('Cc', [8, 48])
def test_s2d_to_nhwc_bf16(Cc, size):
    _s2d(False, 2, size[0], size[1], Cc)


@pytest.mark.parametrize('size', [(3, 5), (8, 8)])
@pytest.mark.parametrize('Cc', [4, 12, 48])
def test_s2d_to_nhwc_f32(Cc, size):
    _s2d(True, 2, size[0], size[1], Cc)


@pytest.mark.parametrize('f32', [False, True])
def test_s2d_to_nhwc_grid_stride(f32):
    """192 x 192 x 4 x 8 vectors = 1 179 648"""
    _s2d(f32, 1, 192, 192, 32 if f32 else 64)


def test_s2d_to_nhwc_refusals():
    import torch
    from cdnet_amd import _lib
    x = torch.zeros((4096,), dtype=torch.float32, device='cuda')
    for name, Cc in (('cdnet_s2d_to_nhwc', 12), ('cdnet_s2d_to_nhwc_f32', 6)):
        out = gc.sentinel_buffer(64, 16, 0, torch.float32)
        with pytest.raises(_lib.CdnetHipError):
            _lib.call(name, _lib.ptr(x), 1, 2, 2, Cc, _lib.ptr(out), _lib.stream_ptr())
        torch.cuda.synchronize()
        assert gc.untouched(out)


# ------------------------------------------------------------------------------------------------------
# cdnet_grad_sum / _f32
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('nterm', [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize('f32', [False, True])
def test_grad_sum(f32, nterm, masked):
    """real inputs, equality with the same fp32 chain on the CPU; terms of their own, with cstride = 0 and as slices of wider tensors;
    the mask holds exact zeros and -0.0"""
    import torch
    for Cc in (8, 48, 144):
        for npix in (1, 37, 4099):
            got, want = gc.grad_sum_case(f32, npix, Cc, nterm, masked, seed=600 + nterm)
            assert torch.equal(got, want), 'grad_sum C=%d npix=%d: %d elements differ' % (Cc, npix, int((got != want).sum()))


@pytest.mark.parametrize('f32', [False, True])
def test_grad_sum_grid_stride(f32):
    """131 101 pixels x 64 channels = 1 048 808 vectors"""
    import torch
    got, want = gc.grad_sum_case(f32, 131101, 64, 2, True, seed=13, exact=True)
    assert torch.equal(got, want), '%d elements differ' % int((got != want).sum())


def test_grad_sum_refusals():
    import torch
    from cdnet_amd import _lib
    g = torch.ones((37 * 32,), dtype=torch.bfloat16, device='cuda')
    for nterm, Cc, cs, co in ((0, 16, 0, 0), (7, 16, 0, 0), (1, 12, 0, 0), (1, 16, 24, 16)):
        arr = (gc.GradTerm * 7)()
        for k in range(7):
            arr[k].g, arr[k].cstride, arr[k].coff = g.data_ptr(), cs, co
        out = gc.sentinel_buffer(37, 16, 0, torch.bfloat16)
        with pytest.raises(_lib.CdnetHipError):
            _lib.call('cdnet_grad_sum', C.byref(arr), nterm, None, 37, Cc, _lib.ptr(out), _lib.stream_ptr())
        torch.cuda.synchronize()
        assert gc.untouched(out)


# ------------------------------------------------------------------------------------------------------
# cdnet_bias_grad / _f32
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Cc', [8, 16, 48, 80, 144, 2048])
@pytest.mark.parametrize('f32', [False, True])
def test_bias_grad_exact(f32, Cc):
    """integer inputs, every partial sum below 2^24: equality with the int64 column sum.  48 / 80 / 144 channels: 256 is no multiple of
    the threads per pixel, the left-over threads of a workgroup sit out"""
    import torch
    for npix in (1, 7, 1000):
        g = torch.randint(-8, 9, (npix, Cc), generator=torch.Generator().manual_seed(npix + Cc))
        db = gc.bias_grad_run(f32, g.to(torch.float32 if f32 else torch.bfloat16), Cc)
        assert torch.equal(db.long(), g.sum(0)), 'bias_grad C=%d npix=%d' % (Cc, npix)


@pytest.mark.parametrize('f32', [False, True])
def test_bias_grad_beyond_the_block_cap(f32):
    """C = 8: 256 pixels per workgroup and trip, 8 trips per workgroup wanted -> 513 workgroups, capped at 512: threads stride, and the
    last pixel count is odd"""
    import torch
    npix = 1_048_583
    assert -(-npix // (256 * 8)) > 512
    g = torch.randint(-8, 9, (npix, 8), generator=torch.Generator().manual_seed(3))
    db = gc.bias_grad_run(f32, g.to(torch.float32 if f32 else torch.bfloat16), 8)
    assert torch.equal(db.long(), g.sum(0))


@pytest.mark.parametrize('f32', [False, True])
def test_bias_grad_real(f32):
    """|db - ref| <= depth * 2^-24 * sum_p |g[p, c]| with depth from gc.bias_depth (its docstring derives it): here C = 80, 4099 pixels:
    ppb = 25, nb = 21 workgroups, 8 pixels per thread + 26 per-thread sums + 1 per lane + 6 butterfly steps = 41"""
    import torch
    npix, Cc = 4099, 80
    assert gc.bias_depth(npix, Cc) == 41
    g = torch.randn((npix, Cc), generator=torch.Generator().manual_seed(5)).to(torch.float32 if f32 else torch.bfloat16)
    db = gc.bias_grad_run(f32, g, Cc).double()
    ref, S = g.double().sum(0), g.double().abs().sum(0)
    bound = gc.bias_depth(npix, Cc) * gc.EPS * S
    err = (db - ref).abs()
    print('bias_grad worst err / bound %.3f' % float((err / bound).max()))
    assert bool((err <= bound).all()), 'worst err / bound %.3f' % float((err / bound).max())


def test_bias_grad_refusals():
    import torch
    from cdnet_amd import _lib
    for Cc, short in ((12, 0), (2056, 0), (16, 1)):
        g = torch.ones((7, Cc), dtype=torch.bfloat16)
        with pytest.raises(_lib.CdnetHipError):
            gc.bias_grad_run(False, g, Cc, workspace_floats=512 * Cc - short)
        assert gc.untouched(gc.bias_grad_run.last_db), 'a refused call wrote db'
