"""The 16-channel classifier (csrc/classifier16.hip: cdnet_final_conv1x1_c16 and its backward) per element against fp64 on the same
inputs, after those inputs were rounded to their storage format.

Bars (T = the sum of the absolute values of the terms of the dot product or sum in question; derived, not tuned):
  logits   |err| <= 1e-5 * (sum_c |w_kc| (|raw_c scale_c| + |shift_c|) + |b_k|): 1 + 16 + 2 = 19 fp32 roundings, 1.1e-6, times a margin of 8
  df       fp32 storage: 1e-5 * T (at most 20 fused multiply-adds, 20 * 2^-24 = 1.2e-6); 16-bit storage: 2^-8 * T - one bf16 rounding to
           nearest is at most u / (1 + u) = 0.9961 u relative with u = 2^-8, the fp32 sum before it adds at most 1.2e-6 = 0.0003 u
  dw, db   1e-4 * T.  The kernel's sums: every thread adds one term per trip of its grid-stride loop - a chain of ceil(pixels / (1024 * 64)),
           2 at 260 x 260 and 1 at the other shapes here (16 for 16 tiles of 256 x 256) - then a 4-level butterfly over the wave's 16 pixel
           slots, 2 levels over the four waves, and in reduce_partials_kernel a chain of at most 1024 / 64 = 16 partial rows per lane with
           a 6-level butterfly: 2 + 4 + 2 + 16 + 6 = 30 additions at most here, 30 * 2^-24 = 1.8e-6, a margin of 56 under 1e-4 (44
           additions, a margin of 38, at the training size).  The feature itself carries one rounding of |raw scale| + |shift|, which
           is at most a few times |F| on these inputs: far inside the same margin.

Shapes, the smallest at which each mechanism can fail: one pixel; less than one workgroup with odd sizes; several workgroups with a tail;
and 260 x 260 = 67 600 pixels, just past 1024 workgroups x 64 pixels = 65 536, the only size here at which the backward's grid-stride loop
takes a second trip (the 1024 is read back from the workspace size the library reports, the 64 is C16_PPB of the kernel)."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (2, 5, 7), (3, 33, 65), (1, 260, 260)]
FORMS = ['bf16', 'fp16_affine_relu', 'fp32_affine_relu', 'fp32']
KS = (1, 3, 17, 20)
PPB, ROW_MOST = 64, 20 * 16 + 20           # pixels per workgroup of the backward; floats of its widest partial row


@functools.lru_cache(maxsize=None)
def _inputs(shape, form):
    """storage-rounded inputs on the CPU (shared by the K's of a case, never modified) and their fp64 views"""
    import torch
    N, H, W = shape
    g = torch.Generator().manual_seed(1000 * SHAPES.index(shape) + FORMS.index(form))
    raw = torch.randn((N, H, W, 16), generator=g)
    dt = {'bf16': torch.bfloat16, 'fp16_affine_relu': torch.float16}.get(form, torch.float32)
    raw = raw.to(dt)
    affine = form.endswith('affine_relu')
    scale = (torch.rand((16,), generator=g) + 0.5) if affine else None
    shift = (torch.randn((16,), generator=g) * 0.2) if affine else None
    w = torch.randn((20, 16), generator=g)
    b = torch.randn((20,), generator=g)
    dl = torch.randn((N, 20, H, W), generator=g)
    r64 = raw.double()
    if affine:
        pre = r64 * scale.double() + shift.double()
        F = pre.clamp_min(0)
        mag = (r64 * scale.double()).abs() + shift.double().abs()
    else:
        F, mag = r64, r64.abs()
    return dict(raw=raw, scale=scale, shift=shift, relu=affine, w=w, b=b, dl=dl, F=F, mag=mag)


def _device_feat(d):
    from cdnet_amd import runtime
    src = runtime.Src(d['raw'].cuda(), None if d['scale'] is None else d['scale'].cuda(), None if d['shift'] is None else d['shift'].cuda(),
                      relu=d['relu'])
    return src, runtime.head_feat16(src)


def test_shape_past_the_workgroup_cap_is_in_the_list():
    from cdnet_amd import _lib
    cap = _lib.load().cdnet_final_conv1x1_c16_backward_workspace_floats() // ROW_MOST - 1
    assert cap == 1024
    n = [s[0] * s[1] * s[2] for s in SHAPES]
    assert max(n) > cap * PPB and max(n) <= 2 * cap * PPB and sorted(n)[-2] <= cap * PPB


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_forward_vs_fp64(shape, form):
    import torch
    from cdnet_amd import _lib
    d = _inputs(shape, form)
    N, H, W = shape
    src, hf = _device_feat(d)
    for K in KS:
        w, b = d['w'][:K].contiguous(), d['b'][:K].contiguous()
        out = torch.full((N, K, H, W), float('nan'), dtype=torch.float32, device='cuda')
        wd, bd = w.cuda(), b.cuda()
        _lib.call('cdnet_final_conv1x1_c16', C.byref(hf), _lib.ptr(wd), _lib.ptr(bd), K, N, H, W, _lib.ptr(out), _lib.stream_ptr())
        want = torch.einsum('nhwc,kc->nkhw', d['F'], w.double()) + b.double().view(1, K, 1, 1)
        S = torch.einsum('nhwc,kc->nkhw', d['mag'], w.double().abs()) + b.double().abs().view(1, K, 1, 1)
        err = (out.cpu().double() - want).abs()
        ratio = float((err / (1e-5 * S)).max())
        print('forward %s %s K=%d: worst error %.3g of its bar' % (shape, form, K, ratio))
        assert bool(torch.isfinite(out).all()) and ratio <= 1.0, (shape, form, K, ratio)


def _backward(d, hf, K, shape, tail=4096, sentinel=-12345.0):
    import torch
    from cdnet_amd import _lib
    N, H, W = shape
    need = _lib.load().cdnet_final_conv1x1_c16_backward_workspace_floats()
    ws = torch.full((need + tail,), sentinel, dtype=torch.float32, device='cuda')
    f32 = d['raw'].dtype == torch.float32
    df = torch.full((N, H, W, 16), float('nan'), dtype=torch.float32 if f32 else torch.bfloat16, device='cuda')
    dw = torch.full((K, 16), float('nan'), dtype=torch.float32, device='cuda')
    db = torch.full((K,), float('nan'), dtype=torch.float32, device='cuda')
    wd, dld = d['w'][:K].contiguous().cuda(), d['dl'][:, :K].contiguous().cuda()
    _lib.call('cdnet_final_conv1x1_c16_backward', C.byref(hf), _lib.ptr(wd), _lib.ptr(dld), K, N, H, W, _lib.ptr(df), _lib.ptr(ws),
              ws.numel(), _lib.ptr(dw), _lib.ptr(db), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert bool((ws[need:] == sentinel).all()), 'the backward wrote past the workspace size it reports'
    return df.cpu(), dw.cpu(), db.cpu()


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_backward_vs_fp64(shape, form):
    import torch
    d = _inputs(shape, form)
    src, hf = _device_feat(d)
    f32 = d['raw'].dtype == torch.float32
    for K in KS:
        df, dw, db = _backward(d, hf, K, shape)
        df2, dw2, db2 = _backward(d, hf, K, shape)
        for a, b_ in ((df, df2), (dw, dw2), (db, db2)):                       # same bits every run
            assert torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32),
                               b_.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32)), (shape, form, K)
        w, dl = d['w'][:K].double(), d['dl'][:, :K].double()
        want_df = torch.einsum('nkhw,kc->nhwc', dl, w)
        T_df = torch.einsum('nkhw,kc->nhwc', dl.abs(), w.abs())
        want_dw = torch.einsum('nkhw,nhwc->kc', dl, d['F'])
        T_dw = torch.einsum('nkhw,nhwc->kc', dl.abs(), d['F'].abs())
        want_db, T_db = dl.sum((0, 2, 3)), dl.abs().sum((0, 2, 3))
        r_df = float(((df.double() - want_df).abs() / ((1e-5 if f32 else 2.0 ** -8) * T_df)).max())
        e_dw, e_db = (dw.double() - want_dw).abs(), (db.double() - want_db).abs()
        print('backward %s %s K=%d: df %.3g of its bar, dw %.3g, db %.3g' % (shape, form, K, r_df, float((e_dw / (1e-4 * T_dw + 1e-300)).max()),
                                                                             float((e_db / (1e-4 * T_db)).max())))
        assert bool(torch.isfinite(df.float()).all()) and r_df <= 1.0, (shape, form, K, r_df)
        assert bool((e_dw <= 1e-4 * T_dw).all()), (shape, form, K, float((e_dw - 1e-4 * T_dw).max()))
        assert bool((e_db <= 1e-4 * T_db).all()), (shape, form, K)
