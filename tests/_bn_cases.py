"""One BatchNorm + ReLU (+ residual) (+ max-pool / F.pad consumers) backward case against CPU autograd, shared by
test_gpu_train_kernels.py (16-bit tensors), test_gpu_fp32_kernels.py (fp32 tensors) and test_gpu_bn_bwd.py.

fmt: 'f16' / 'bf16' (raw output and residual stored as fp16 / bf16, gradients and dRaw bf16) or 'f32' (everything fp32).
Tolerances (relative L2): 16-bit dRaw 1e-2, dgamma / dbeta 3e-3, dz 6e-3 (bf16 outputs, bf16-rounded gradients); fp32 1e-5."""
import ctypes as C

TOL = {'16': dict(draw=1e-2, dparam=3e-3, dz=6e-3), 'f32': dict(draw=1e-5, dparam=1e-5, dz=1e-5)}


def rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def nchw(y):
    return y.float().cpu().permute(0, 3, 1, 2).contiguous()


def grid_rows(npix, Cc, chans_per_thread=8, unroll=4):
    """workgroups (= partial rows) of the flat passes over npix pixels"""
    per_block = (256 // (Cc // chans_per_thread)) * unroll
    return max(1, min(512, -(-npix // per_block)))


class Case:
    """inputs on the device (kept alive here), the filled cdnet_bn_bwd_args and the autograd reference"""


def build(fmt, pooled, with_res, two_grads, seed, outmask=False, skip=0, size=(12, 20), pool_first=True, plain=0, Cc=32, relu=1, bn=True):
    """pooled: a 2x2 max-pool consumer; skip: same-size consumers reading a channel slice of a wider gradient; plain: same-size
    consumers with a gradient of their own; (two_grads or not pooled) and no skip / plain: one more consumer - through F.pad offsets
    and a channel slice, or (outmask) plain.  outmask: relu = 2, `res` is the stored post-ReLU output and the mask is read from it.
    relu = 0: the source went through the ReLU already (trainer._bn_backward_masked).  bn = False: a layer without BatchNorm."""
    import torch
    import torch.nn.functional as F
    from cdnet_amd import trainer
    f32 = fmt == 'f32'
    raw_dt = {'f16': torch.float16, 'bf16': torch.bfloat16, 'f32': torch.float32}[fmt]
    act_dt = torch.float32 if f32 else torch.bfloat16
    stored = (lambda x: x) if f32 else (lambda x: x.to(raw_dt).float())          # values a stored tensor can hold
    bf = (lambda x: x) if f32 else (lambda x: x.to(torch.bfloat16).float())
    nhwc = lambda x, dt=act_dt: x.permute(0, 2, 3, 1).contiguous().to(dt).cuda()
    g = torch.Generator().manual_seed(seed)
    N, (H, W) = 2, size
    raw = stored(torch.randn((N, Cc, H, W), generator=g)).requires_grad_(True)
    res = stored(torch.randn((N, Cc, H, W), generator=g)).requires_grad_(True) if with_res else None
    gamma = (torch.rand((Cc,), generator=g) + 0.5).requires_grad_(True)
    gamma.data[::4] *= -1
    beta = (torch.randn((Cc,), generator=g) * 0.2).requires_grad_(True)
    mean = raw.detach().mean((0, 2, 3))
    var = raw.detach().var((0, 2, 3), unbiased=False)
    y = F.batch_norm(raw, None, None, gamma, beta, training=True, eps=1e-5) if bn else raw
    if with_res:
        y = y + res
    a = F.relu(y) if relu else y
    if not f32:
        a = a + (bf(a.detach()) - a.detach())      # consumers see the activation rounded to bf16 (as the conv staging does)
    total = 0
    gins = []
    if pooled:
        p = F.max_pool2d(a, 2)
        gp = bf(torch.randn(p.shape, generator=g))
        total = total + (p * gp).sum()
        gins.append(trainer._G(nhwc(gp), p.shape[2], p.shape[3], pooled=1))
    for _ in range(skip):
        # a same-size consumer that reads the activation as a channel slice of a wider tensor (the decoder's torch.cat with the skip)
        gwide = bf(torch.randn((N, Cc + 16, H, W), generator=g))
        total = total + (a * gwide[:, 16:16 + Cc]).sum()
        gins.append(trainer._G(nhwc(gwide), H, W, coff=16, cstride=Cc + 16))
    for _ in range(plain):
        gown = bf(torch.randn((N, Cc, H, W), generator=g))
        total = total + (a * gown).sum()
        gins.append(trainer._G(nhwc(gown), H, W))
    if not pool_first:
        gins = gins[1:] + gins[:1]
    if (two_grads or not pooled) and not skip and not plain:
        if outmask:
            gfull = bf(torch.randn((N, Cc, H, W), generator=g))
            total = total + (a * gfull).sum()
            gins.append(trainer._G(nhwc(gfull), H, W))
        else:
            # consumer that read the tensor through F.pad offsets (1, 2) and as a channel slice of a wider gradient
            ap = F.pad(a, (2, 1, 1, 0))
            gfull = bf(torch.randn((N, Cc + 16, H + 1, W + 3), generator=g))
            total = total + (ap * gfull[:, 8:8 + Cc]).sum()
            gins.append(trainer._G(nhwc(gfull), H + 1, W + 3, oy=1, ox=2, coff=8, cstride=Cc + 16))
    total.backward()
    invstd = 1.0 / torch.sqrt(var + 1e-5)
    scale = (gamma.detach() * invstd)
    shift = beta.detach() - mean * scale
    c = Case()
    c.fmt, c.f32, c.with_res, c.bn, c.shape, c.act_dt = fmt, f32, with_res, bn, (N, H, W, Cc), act_dt
    c.raw_grad, c.res_grad, c.gamma_grad, c.beta_grad = raw.grad, (res.grad if with_res else None), gamma.grad, beta.grad
    A = c.A = trainer.BnBwdArgs()
    raw_d = nhwc(raw.detach(), raw_dt)
    res_d = None
    if with_res:
        # relu = 2: `res` is the stored post-ReLU output of the unit (the fused residual epilogue), the mask is read from it
        res_d = nhwc(a.detach()) if outmask else nhwc(res.detach(), raw_dt)
    A.raw, A.res = raw_d.data_ptr(), (res_d.data_ptr() if with_res else None)
    dev = lambda t: t.detach().float().cuda().contiguous()
    sc, sh, mu, iv, c.gamma = dev(scale), dev(shift), dev(mean), dev(invstd), dev(gamma)
    if bn:
        A.scale, A.shift, A.mean, A.invstd = sc.data_ptr(), sh.data_ptr(), mu.data_ptr(), iv.data_ptr()
    A.ngin = len(gins)
    for k, gi in enumerate(gins):
        A.gin[k].g = gi.t.data_ptr()
        A.gin[k].Hg, A.gin[k].Wg, A.gin[k].oy, A.gin[k].ox = gi.Hg, gi.Wg, gi.oy, gi.ox
        A.gin[k].pooled, A.gin[k].coff, A.gin[k].cstride = gi.pooled, gi.coff, gi.cstride or Cc
    A.f16 = {'bf16': 0, 'f16': 1, 'f32': 2}[fmt]
    A.relu, A.N, A.H, A.W, A.C = (2 if outmask else relu), N, H, W, Cc
    c.keep = [raw_d, res_d, sc, sh, mu, iv, gins]
    return c


def run(c):
    """cdnet_bn_backward on the case: (draw, dz or None, dgamma, dbeta) on the device"""
    import torch
    from cdnet_amd import _lib
    N, H, W, Cc = c.shape
    ws = torch.empty((_lib.load().cdnet_bn_backward_workspace_floats(Cc),), dtype=torch.float32, device='cuda')
    dgamma, dbeta = torch.zeros(Cc, device='cuda'), torch.zeros(Cc, device='cuda')
    draw = torch.empty((N, H, W, Cc), dtype=c.act_dt, device='cuda')
    dz = torch.empty((N, H, W, Cc), dtype=c.act_dt, device='cuda') if c.with_res else None
    _lib.call('cdnet_bn_backward', C.byref(c.A), _lib.ptr(c.gamma) if c.bn else None, _lib.ptr(dgamma) if c.bn else None,
              _lib.ptr(dbeta) if c.bn else None, _lib.ptr(ws), ws.numel(), _lib.ptr(draw), _lib.ptr(dz) if c.with_res else None,
              _lib.stream_ptr())
    torch.cuda.synchronize()
    return draw, dz, dgamma, dbeta


def check(c, draw, dz, dgamma, dbeta):
    tol = TOL['f32' if c.f32 else '16']
    assert rel(nchw(draw), c.raw_grad) < tol['draw'], ('draw', rel(nchw(draw), c.raw_grad))
    if c.bn:
        assert rel(dgamma.cpu(), c.gamma_grad) < tol['dparam'] and rel(dbeta.cpu(), c.beta_grad) < tol['dparam'], \
            ('dgamma, dbeta', rel(dgamma.cpu(), c.gamma_grad), rel(dbeta.cpu(), c.beta_grad))
    if c.with_res:
        assert rel(nchw(dz), c.res_grad) < tol['dz'], ('dz', rel(nchw(dz), c.res_grad))


def bn_case(fmt, pooled, with_res, two_grads, seed, **kw):
    c = build(fmt, pooled, with_res, two_grads, seed, **kw)
    check(c, *run(c))
