"""Inputs, fp64 CPU references and error bounds for tests/test_gpu_glue_kernels.py: the streaming kernels of HRNet training
(cdnet_fuse_sum, cdnet_upsample_bilinear_backward, cdnet_s2d_to_nhwc, cdnet_grad_sum) and the UNet bias gradient (cdnet_bias_grad).

Two kinds of input.

EXACT inputs make fp32 arithmetic independent of its order: values are integers |v| <= 8 (exact in bf16 / fp16 / fp32), scales come
from {0.5, 1, 2}, shifts are multiples of 0.5 and every resolution ratio is a power of two, so `sy`, `fy` and the bilinear weights
are dyadic (multiples of 1 / 16 per axis at ratio 8).  A term is then a multiple of 2^-9 below 2^7 and a sum of four of them below
2^9: 18 bits, every product and partial sum is exact in fp32, and the requirement is EQUALITY with the fp64 reference (rounded once
to bf16, RNE, for the 16-bit entries).  One dropped, duplicated or mis-weighted element fails it.

REAL inputs are seeded normal values (rounded to the storage type); the bound is per element, e = 2^-24 * (k * S + kw * A):

  S   the reference formula evaluated in fp64 on absolute values (|term * scale| + |shift| through the non-negative bilinear
      weights; |dout| through the transposed weights): every fp32 rounding on the way rounds a partial result whose magnitude S bounds.
  k   the number of such roundings on the longest chain.
      fuse_sum, per term: the affine fma, hx * a, + lx * b, hy * (.), the sum of the two rows, acc += : 6 roundings of a quantity
      bounded by the term's share of S, then at most nterm - 1 later roundings of the running sum: (6 + nterm) <= 8 * nterm.
      upsample_bwd: wy * wx, 1 - l, and one fma per candidate with a non-zero weight.  Output row y reads source row ys only if
      ys - 1 < fy < ys + 1, an interval of 2 H / Hs rows, so at most 2 * ceil(H / Hs) + 1 rows (one more for a row that fp32 puts on the
      other side of the boundary) and as many columns by the same rule: k = rows * cols + 2.
  kw  the weight error.  fy = (y + 0.5) * sy - 0.5 in fp32: sy carries one rounding (relative 2^-24, times y + 0.5 <= Hs), the product
      one and the subtraction one, each at most Hs * 2^-24; 1 - ly one more: |d wy| <= 4 * Hs * 2^-24, in both axes 4 * (Hs + Ws).
      (A fy that crosses an integer moves the tap pair but not the interpolated value: it is continuous in fy.)
  A   what a weight error multiplies.  A perturbed weight moves the result by d * (a - c): bounded by the taps, not by their weighted
      sum (hy ~ 1, ly ~ 0 gives S ~ |a| whatever c is), so S cannot carry this term.  fuse_sum: A = sum over the up-sampled terms of
      max over the pixels of |term| per (n, c).  upsample_bwd: every candidate takes part: A = rows * cols * max over the pixels of
      |dout| per (n, c).  With the shapes used here kw * A * 2^-24 stays below 1e-3 of a typical element; a missing or mis-weighted
      tap is an error of order 0.1.

The bf16 entries round the fp32 result r once more (RNE).  bf16 keeps 8 significant bits, so the rounding moves r by at most half a
unit in the last place of r's binade, 2^(floor(log2 |r|) - 8): between 2^-9 |r| (top of a binade) and 2^-8 |r| (bottom); a flat
2^-9 * |ref| would refuse correctly rounded results in the lower half of every binade.  With |r| <= |ref| + e:
|got - ref| <= 2^(floor(log2(|ref| + e)) - 8) + e.

grad_sum adds its terms in index order in fp32, masks, and rounds once: the reference is the same chain in torch fp32 on the CPU and
the requirement is equality for real inputs too.  bias_grad: see bias_depth()."""
import ctypes as C

from cdnet_amd._lib import GradTerm                     # cdnet_grad_term (test_gpu_glue_kernels builds tables of it too)

EPS = 2.0 ** -24
SENTINEL = 4096.0                 # exact in bf16; no result here comes near it
F16_CODE = {'bf16': 0, 'f16': 1, 'f32': 2}


def tdtype(store):
    import torch
    return {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32}[store]


def sentinel_buffer(pixels, width, guard_pixels, dtype):
    """[pixels + guard_pixels][width] on the device, every element SENTINEL"""
    import torch
    return torch.full((pixels + guard_pixels, width), SENTINEL, dtype=dtype, device='cuda')


def check_guards(buf, pixels, coff, Cc):
    """channels outside [coff, coff + Cc) and the guard pixels after the end still hold SENTINEL"""
    b = buf.float().cpu()
    assert (b[pixels:] == SENTINEL).all(), 'wrote past the end'
    assert (b[:pixels, :coff] == SENTINEL).all() and (b[:pixels, coff + Cc:] == SENTINEL).all(), 'wrote outside the channel slice'


def untouched(buf):
    return bool((buf.float().cpu() == SENTINEL).all())


def values(shape, gen, exact, store, dtype=None):
    """fp64 (or `dtype`) values that `store` holds exactly"""
    import torch
    dtype = dtype or torch.float64
    if exact:
        return torch.randint(-8, 9, shape, generator=gen, dtype=dtype)
    return torch.randn(shape, generator=gen).to(tdtype(store)).to(dtype)


def nhwc(x, dtype):
    """NCHW fp64 on the CPU -> contiguous NHWC of `dtype` on the device"""
    return x.permute(0, 2, 3, 1).contiguous().to(dtype).cuda()


def nchw(y):
    return y.double().cpu().permute(0, 3, 1, 2).contiguous()


# ------------------------------------------------------------------------------------------------------
# cdnet_fuse_sum
# ------------------------------------------------------------------------------------------------------
def fuse_case(f32, N, H, W, Cc, terms, relu, sliced, exact, seed, guard=True):
    """terms: list of (Hs, Ws, store, affine).  Runs the entry; returns (got, ref, e): NCHW fp64 on the CPU, e the bound for the fp32
    result (see the module docstring)."""
    import torch
    import torch.nn.functional as F
    from cdnet_amd import _lib
    from cdnet_amd.runtime import FuseTerm
    g = torch.Generator().manual_seed(seed)
    arr = (FuseTerm * len(terms))()
    keep, ref, S, A = [], 0.0, 0.0, 0.0
    for k, (Hs, Ws, store, affine) in enumerate(terms):
        v = values((N, Cc, Hs, Ws), g, exact, store)
        xd = nhwc(v, tdtype(store))
        keep.append(xd)
        arr[k].x, arr[k].Hs, arr[k].Ws, arr[k].f16 = xd.data_ptr(), Hs, Ws, F16_CODE[store]
        if affine:
            if exact:
                sc = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (Cc,), generator=g)]
                sh = torch.randint(-4, 5, (Cc,), generator=g).float() * 0.5
            else:
                sc, sh = torch.rand((Cc,), generator=g) + 0.5, torch.randn((Cc,), generator=g) * 0.3
            scd, shd = sc.cuda(), sh.cuda()
            keep += [scd, shd]
            arr[k].scale, arr[k].shift = scd.data_ptr(), shd.data_ptr()
            a = (v * sc.double().view(1, -1, 1, 1)).abs() + sh.double().abs().view(1, -1, 1, 1)
            v = v * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)
        else:
            a = v.abs()
        if (Hs, Ws) != (H, W):
            A = A + a.amax(dim=(2, 3), keepdim=True)
            v = F.interpolate(v, size=(H, W), mode='bilinear', align_corners=False)
            a = F.interpolate(a, size=(H, W), mode='bilinear', align_corners=False)
        ref, S = ref + v, S + a
    if relu:
        ref = F.relu(ref)
    cstride, coff = (Cc + 16, 8) if sliced else (Cc, 0)
    pixels = N * H * W
    out = sentinel_buffer(pixels, cstride, W if guard else 0, torch.float32 if f32 else torch.bfloat16)
    _lib.call('cdnet_fuse_sum_f32' if f32 else 'cdnet_fuse_sum', C.byref(arr), len(terms), N, H, W, Cc, relu, _lib.ptr(out),
              cstride if sliced else 0, coff, _lib.stream_ptr())
    torch.cuda.synchronize()
    if guard:
        check_guards(out, pixels, coff, Cc)
    got = nchw(out[:pixels, coff:coff + Cc].reshape(N, H, W, Cc))
    k = 8 * len(terms)
    ups = [t for t in terms if (t[0], t[1]) != (H, W)]                # only these carry interpolation weights
    kw = 4 * (max(t[0] for t in ups) + max(t[1] for t in ups)) if ups else 0
    return got, ref, EPS * (k * S + kw * A)


def assert_close(got, ref, e, f32, what=''):
    """real inputs: |got - ref| <= e (fp32 entry) or half a bf16 ulp of (|ref| + e), plus e (bf16 entry); prints the worst ratio
    before it asserts"""
    import torch
    bound = e
    if not f32:
        ex = torch.frexp((ref.abs() + e).clamp_min(2.0 ** -120))[1]                 # |ref| + e = m * 2^ex, 0.5 <= m < 1
        bound = torch.ldexp(torch.ones_like(ref), ex - 9) + e
    err = (got - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print('%s worst |err| %.3e, worst err / bound %.3f' % (what, float(err.max()), worst))
    assert bool((err <= bound).all()), '%s: worst err / bound %.3f, worst |err| %.3e' % (what, worst, float(err.max()))


def assert_exact(got, ref, f32, what=''):
    """exact inputs: equality with the fp64 reference (fp32 entry) or with its RNE to bf16 (16-bit entry)"""
    import torch
    want = ref if f32 else ref.float().to(torch.bfloat16).double()
    bad = int((got != want).sum())
    assert bad == 0, '%s: %d of %d elements differ, worst %.3e' % (what, bad, got.numel(), float((got - want).abs().max()))


# ------------------------------------------------------------------------------------------------------
# cdnet_upsample_bilinear_backward
# ------------------------------------------------------------------------------------------------------
def upsample_bwd_reference(d, Hs, Ws):
    """transpose of F.interpolate(bilinear, align_corners=False) by autograd, in the dtype of d (NCHW, CPU)"""
    import torch
    import torch.nn.functional as F
    x = torch.zeros((d.shape[0], d.shape[1], Hs, Ws), dtype=d.dtype, requires_grad=True)
    F.interpolate(x, size=d.shape[2:], mode='bilinear', align_corners=False).backward(d)
    return x.grad


def upsample_bwd_case(f32, N, Hs, Ws, H, W, Cc, sliced, exact, seed, ref_dtype=None):
    """returns (got, ref, e), NCHW on the CPU"""
    import torch
    from cdnet_amd import _lib
    g = torch.Generator().manual_seed(seed)
    cstride, coff = (Cc + 8, 8) if sliced else (Cc, 0)
    store = 'f32' if f32 else 'bf16'
    wide = values((N, cstride, H, W), g, exact, store, ref_dtype)           # the channels outside the slice hold values too: reading them shows
    dd = nhwc(wide, tdtype(store))
    d = wide[:, coff:coff + Cc].contiguous()
    ref = upsample_bwd_reference(d, Hs, Ws)
    pixels = N * Hs * Ws
    din = sentinel_buffer(pixels, Cc, Ws, tdtype(store))
    _lib.call('cdnet_upsample_bilinear_backward_f32' if f32 else 'cdnet_upsample_bilinear_backward', _lib.ptr(dd), N, H, W, Cc,
              cstride if sliced else 0, coff, Hs, Ws, _lib.ptr(din), _lib.stream_ptr())
    torch.cuda.synchronize()
    check_guards(din, pixels, 0, Cc)
    got = din[:pixels].reshape(N, Hs, Ws, Cc).cpu().permute(0, 3, 1, 2).to(ref.dtype)
    if exact:
        return got, ref, None
    S = upsample_bwd_reference(d.abs(), Hs, Ws)
    ncand = (2 * -(-H // Hs) + 1) * (2 * -(-W // Ws) + 1)
    A = ncand * d.abs().amax(dim=(2, 3), keepdim=True)
    return got, ref, EPS * ((ncand + 2) * S + 4 * (Hs + Ws) * A)


# ------------------------------------------------------------------------------------------------------
# cdnet_grad_sum
# ------------------------------------------------------------------------------------------------------
def grad_sum_case(f32, npix, Cc, nterm, masked, seed, exact=False):
    """term k reads: k = 0 a tensor of its own with cstride = 0 (= C); k odd a slice of a wider tensor (cstride = C + 8 * (k + 1),
    coff = 8 * k); other k a tensor of its own with cstride = C given.  Returns (got, want) on the CPU, in the output dtype."""
    import torch
    from cdnet_amd import _lib
    g = torch.Generator().manual_seed(seed)
    dt = torch.float32 if f32 else torch.bfloat16
    arr = (GradTerm * nterm)()
    keep = []
    acc = torch.zeros((npix, Cc), dtype=torch.float32)
    for k in range(nterm):
        cstride, coff = (Cc + 8 * (k + 1), 8 * k) if k % 2 else (Cc, 0)
        t = (torch.randint(-8, 9, (npix, cstride), generator=g).float() if exact else torch.randn((npix, cstride), generator=g)).to(dt)
        td = t.cuda()
        keep.append(td)
        arr[k].g, arr[k].cstride, arr[k].coff = td.data_ptr(), (0 if k == 0 else cstride), coff
        acc = acc + t[:, coff:coff + Cc].float()
    md = None
    if masked:
        m = torch.relu(torch.randn((npix, Cc), generator=g)).to(dt)                # post-ReLU activations: about half exact zeros
        m.view(-1)[::7] = -0.0
        m.view(-1)[3::11] = 0.0
        md = m.cuda()
        acc = torch.where(m.float() > 0, acc, torch.zeros_like(acc))
    want = acc.to(dt)
    out = sentinel_buffer(npix, Cc, 8, dt)
    _lib.call('cdnet_grad_sum_f32' if f32 else 'cdnet_grad_sum', C.byref(arr), nterm, _lib.ptr(md), npix, Cc, _lib.ptr(out), _lib.stream_ptr())
    torch.cuda.synchronize()
    check_guards(out, npix, 0, Cc)
    return out[:npix].cpu(), want


# ------------------------------------------------------------------------------------------------------
# cdnet_bias_grad
# ------------------------------------------------------------------------------------------------------
def bias_blocks(npix, Cc):
    ppb = 256 // (Cc // 8)
    return max(1, min(512, -(-npix // (ppb * 8)))), ppb


def bias_depth(npix, Cc):
    """longest chain of fp32 additions of the scheme head_bwd.hip documents: a thread of the nb <= 512 workgroups adds its
    ceil(npix / (nb * ppb)) pixels one after the other (ppb = 256 / (C / 8) pixels per workgroup and trip), one thread per channel adds
    the workgroup's ceil(256 / (C / 8)) per-thread sums in order, the reduction of the nb partial rows adds ceil(nb / 64) per lane and
    then takes the 6 steps of a 64-lane butterfly.  Each addition rounds a partial sum of the column, bounded by sum_p |g[p, c]|."""
    nb, ppb = bias_blocks(npix, Cc)
    vpp = Cc // 8
    return -(-npix // (nb * ppb)) + -(-256 // vpp) + -(-nb // 64) + 6


def bias_grad_run(f32, g, Cc, workspace_floats=None):
    """g: [npix][C] CPU tensor of the entry's dtype; returns db (CPU fp32) - its buffer has a guard row that is checked"""
    import torch
    from cdnet_amd import _lib
    lib = _lib.load()
    npix = g.shape[0]
    need = lib.cdnet_bias_grad_workspace_floats(Cc)
    ws = torch.full((need,), float('nan'), dtype=torch.float32, device='cuda')
    db = sentinel_buffer(1, Cc, 1, torch.float32)
    gd = g.cuda()
    try:
        _lib.call('cdnet_bias_grad_f32' if f32 else 'cdnet_bias_grad', _lib.ptr(gd), npix, Cc, _lib.ptr(ws),
                  need if workspace_floats is None else workspace_floats, _lib.ptr(db), _lib.stream_ptr())
    finally:
        torch.cuda.synchronize()
        bias_grad_run.last_db = db
    check_guards(db, 1, 0, Cc)
    return db[0].cpu()
