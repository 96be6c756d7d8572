"""cdnet_dam_head_backward_fused (fp32 training step): the DAM head's backward and its weight gradients in one launch, the third
feature's gradient leaving behind its residual unit's ReLU for that unit's BatchNorm backward - against fp64 autograd (streaming-kernel
tolerance 1e-5, as test_head_forward_backward_fp32 and tests/_bn_cases.py), bit for bit against the two-kernel path on
the same inputs, and through Trainer.backward.

Shapes (N, H, W): (1, 8, 8) one 64-pixel group - every other workgroup must contribute zeros; (3, 7, 9) 189 pixels, a ragged last group
that is no multiple of 4; (2, 24, 20); (2, 192, 192) 73 728 pixels: the 32-pixel chains of the first 256 workgroups get a third pixel, so the
loop over pixel groups, a partly filled group and the exchange of the scalar sums between the two halves of a workgroup all run."""
import ctypes as C
import functools

import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8, 8), (3, 7, 9), (2, 24, 20), (2, 192, 192)]


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().float().cuda()


def _nchw(y):
    return y.float().cpu().permute(0, 3, 1, 2).contiguous()


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


@functools.lru_cache(maxsize=None)
def _reference(shape):
    """inputs (fp32 values) and the fp64 autograd gradients of  head(f1, f2, relu(batch_norm(raw, gamma, beta) + res)); computed once per
    shape and shared (nobody writes to it)"""
    import torch
    import torch.nn.functional as F
    from oracle import models as om
    torch.manual_seed(3)
    ref = om.Unet().double()
    N, H, W = shape
    g = torch.Generator().manual_seed(17 + N * H * W)
    leaf = lambda *s: torch.randn(s, generator=g).double().requires_grad_(True)
    f1, f2, raw, res = leaf(N, 64, H, W), leaf(N, 64, H, W), leaf(N, 64, H, W), leaf(N, 64, H, W)
    gamma = torch.rand((64,), generator=g) + 0.5
    gamma[::4] *= -1
    gamma = gamma.double().requires_grad_(True)
    beta = (torch.randn((64,), generator=g) * 0.2).double().requires_grad_(True)
    f3 = F.relu(F.batch_norm(raw, None, None, gamma, beta, training=True, eps=1e-5) + res)
    f3.retain_grad()
    # model_unet_rev1.py:258-263
    x_point = ref.point_conv(f3)
    x_dir = ref.direction_conv(ref.directionAtt(f2, x_point))
    x_mask = ref.mask_conv(ref.maskAtt(f1, x_dir))
    gm, gp, gd = [torch.randn(t.shape, generator=g).double() for t in (x_mask, x_point, x_dir)]
    ((x_mask * gm).sum() + (x_point * gp).sum() + (x_dir * gd).sum()).backward()
    ps = [ref.point_conv.weight, ref.direction_conv.weight, ref.mask_conv.weight, ref.point_conv.bias, ref.direction_conv.bias,
          ref.mask_conv.bias, ref.directionAtt.Conv1x1.weight, ref.maskAtt.Conv1x1.weight]
    mean = raw.detach().mean((0, 2, 3))
    invstd = 1.0 / torch.sqrt(raw.detach().var((0, 2, 3), unbiased=False) + 1e-5)
    scale = gamma.detach() * invstd
    return dict(shape=shape, f1=f1.detach(), f2=f2.detach(), f3=f3.detach(), raw=raw.detach(), gamma=gamma.detach(), mean=mean, invstd=invstd,
                scale=scale, shift=beta.detach() - mean * scale, gm=gm, gp=gp, gd=gd,
                hw=torch.cat([p.detach().reshape(-1) for p in ps]), dhw=torch.cat([p.grad.reshape(-1) for p in ps]),
                df1=f1.grad, df2=f2.grad, df3=f3.grad, dres=res.grad, draw=raw.grad, dgamma=gamma.grad, dbeta=beta.grad)


def _device_inputs(R):
    import torch
    from cdnet_amd import engine, runtime
    dev = lambda t: t.detach().float().cuda().contiguous()
    d = dict(feats=[engine.Src(_nhwc(R[k])) for k in ('f1', 'f2', 'f3')], raw=_nhwc(R['raw']), hw=dev(R['hw']))
    d['hf'] = [runtime.head_feat(s) for s in d['feats']]
    for k in ('gm', 'gp', 'gd', 'mean', 'invstd', 'scale', 'shift', 'gamma'):
        d[k] = dev(R[k])
    return d


def _fused(R, d):
    """one call of the new entry: dF1, dF2, dz3, the 855 head gradients"""
    import torch
    from cdnet_amd import _lib
    lib = _lib.load()
    N, H, W = R['shape']
    out = [torch.full((N, H, W, 64), 7.0, dtype=torch.float32, device='cuda') for _ in range(3)]
    ws = torch.full((lib.cdnet_dam_head_backward_fused_workspace_floats(),), float('nan'), dtype=torch.float32, device='cuda')   # (a workgroup without pixels must write zeros)
    dhw = torch.zeros((855,), device='cuda')
    hf = d['hf']
    _lib.call('cdnet_dam_head_backward_fused', C.byref(hf[0]), C.byref(hf[1]), C.byref(hf[2]), _lib.ptr(d['hw']), _lib.ptr(d['gm']),
              _lib.ptr(d['gp']), _lib.ptr(d['gd']), N, H, W, _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]), _lib.ptr(ws), ws.numel(),
              _lib.ptr(dhw), _lib.stream_ptr())
    torch.cuda.synchronize()
    return out[0], out[1], out[2], dhw


def _bn_args(R, d, dz, relu):
    from cdnet_amd import trainer
    N, H, W = R['shape']
    A = trainer.BnBwdArgs()
    A.raw = d['raw'].data_ptr()
    A.scale, A.shift, A.mean, A.invstd = d['scale'].data_ptr(), d['shift'].data_ptr(), d['mean'].data_ptr(), d['invstd'].data_ptr()
    A.ngin = 1
    A.gin[0].g, A.gin[0].Hg, A.gin[0].Wg, A.gin[0].cstride = dz.data_ptr(), H, W, 64
    A.f16, A.relu, A.N, A.H, A.W, A.C = 2, relu, N, H, W, 64
    return A


@pytest.mark.parametrize('shape', SHAPES)
def test_fused_head_backward_against_fp64_autograd(shape):
    """feature gradients, dz3 (= the residual branch's gradient, exactly 0 where f3 <= 0), the 855 head gradients; then the unit's
    BatchNorm backward over dz3 as a relu = 0 source - cdnet_bn_backward (what the trainer runs), and the second pass alone through
    cdnet_bn_backward_finalize + cdnet_bn_backward_apply(relu = 0): draw, dgamma, dbeta - all to 1e-5 of fp64 autograd"""
    import torch
    from cdnet_amd import _lib
    R = _reference(shape)
    d = _device_inputs(R)
    df1, df2, dz3, dhw = _fused(R, d)
    rels = dict(df1=_rel(_nchw(df1), R['df1']), df2=_rel(_nchw(df2), R['df2']), dz3=_rel(_nchw(dz3), R['dres']), dhw=_rel(dhw.cpu(), R['dhw']))
    print(shape, rels)
    assert all(v < 1e-5 for v in rels.values()), rels
    assert bool((dz3[d['feats'][2].x <= 0] == 0).all())
    N, H, W = shape
    dgamma, dbeta = torch.zeros(64, device='cuda'), torch.zeros(64, device='cuda')
    draw = torch.empty((N, H, W, 64), dtype=torch.float32, device='cuda')
    ws = torch.empty((_lib.load().cdnet_bn_backward_workspace_floats(64),), dtype=torch.float32, device='cuda')
    _lib.call('cdnet_bn_backward', C.byref(_bn_args(R, d, dz3, 0)), _lib.ptr(d['gamma']), _lib.ptr(dgamma), _lib.ptr(dbeta), _lib.ptr(ws), ws.numel(),
              _lib.ptr(draw), None, _lib.stream_ptr())
    torch.cuda.synchronize()
    rels = dict(draw=_rel(_nchw(draw), R['draw']), dgamma=_rel(dgamma.cpu(), R['dgamma']), dbeta=_rel(dbeta.cpu(), R['dbeta']))
    print(shape, rels)
    assert all(v < 1e-5 for v in rels.values()), rels
    # the two passes as separate calls: one partial row [2][64] (sum dz, sum dz * xhat) made here in float64
    xh = (d['raw'].double() - d['mean'].double()) * d['invstd'].double()
    part = torch.stack([dz3.double().sum((0, 1, 2)), (dz3.double() * xh).sum((0, 1, 2))]).float().reshape(1, 2, 64).contiguous()
    ktab = torch.zeros((7, 64), device='cuda')
    dgamma2, dbeta2 = torch.zeros(64, device='cuda'), torch.zeros(64, device='cuda')
    draw2 = torch.empty_like(draw)
    _lib.call('cdnet_bn_backward_finalize', C.byref(_bn_args(R, d, dz3, 1)), _lib.ptr(d['gamma']), _lib.ptr(dgamma2), _lib.ptr(dbeta2), _lib.ptr(part),
              1, _lib.ptr(ktab), _lib.stream_ptr())
    _lib.call('cdnet_bn_backward_apply', C.byref(_bn_args(R, d, dz3, 0)), _lib.ptr(ktab), _lib.ptr(draw2), _lib.stream_ptr())
    torch.cuda.synchronize()
    rels = dict(draw=_rel(_nchw(draw2), R['draw']), dgamma=_rel(dgamma2.cpu(), R['dgamma']), dbeta=_rel(dbeta2.cpu(), R['dbeta']))
    print(shape, rels)
    assert all(v < 1e-5 for v in rels.values()), rels


@pytest.mark.parametrize('shape', SHAPES)
def test_fused_head_backward_is_bit_identical_to_the_two_kernel_path(shape):
    """dF1, dF2, dz3 against dF1, dF2 and [f3 > 0] * dF3 of cdnet_dam_head_backward on the same inputs, and the 855 head gradients: every
    sum is taken in the two-kernel path's order and the library is built without floating-point contraction, so all bits agree (an
    indexing error in either shows here).  Then the unit's BatchNorm backward: cdnet_bn_backward over dz3 as a relu = 0 source against
    the relu = 2 form over dF3 with the mask read from f3 - the same draw, dgamma and dbeta, bit for bit"""
    import torch
    from cdnet_amd import _lib
    R = _reference(shape)
    d = _device_inputs(R)
    df1, df2, dz3, dhw = _fused(R, d)
    N, H, W = shape
    old = [torch.empty((N, H, W, 64), dtype=torch.float32, device='cuda') for _ in range(3)]
    ws = torch.empty((_lib.load().cdnet_dam_head_backward_workspace_floats(N, H, W),), device='cuda')
    dhw_old = torch.zeros((855,), device='cuda')
    hf = d['hf']
    _lib.call('cdnet_dam_head_backward', C.byref(hf[0]), C.byref(hf[1]), C.byref(hf[2]), _lib.ptr(d['hw']), _lib.ptr(d['gm']), _lib.ptr(d['gp']),
              _lib.ptr(d['gd']), N, H, W, _lib.ptr(old[0]), _lib.ptr(old[1]), _lib.ptr(old[2]), _lib.ptr(ws), ws.numel(), _lib.ptr(dhw_old),
              _lib.stream_ptr())
    torch.cuda.synchronize()
    f3 = d['feats'][2].x
    assert torch.equal(df1, old[0]) and torch.equal(df2, old[1])
    assert torch.equal(dz3, torch.where(f3 > 0, old[2], torch.zeros_like(old[2])))
    assert torch.equal(dhw[832:], dhw_old[832:]), float((dhw[832:] - dhw_old[832:]).abs().max())
    assert torch.equal(dhw, dhw_old), float((dhw - dhw_old).abs().max())
    res = []
    for g, relu in ((dz3, 0), (old[2], 2)):
        A = _bn_args(R, d, g, relu)
        dzo = None
        if relu == 2:
            A.res = f3.data_ptr()
            dzo = torch.empty_like(g)
        dgamma, dbeta = torch.zeros(64, device='cuda'), torch.zeros(64, device='cuda')
        draw = torch.empty((N, H, W, 64), dtype=torch.float32, device='cuda')
        wsb = torch.empty((_lib.load().cdnet_bn_backward_workspace_floats(64),), dtype=torch.float32, device='cuda')
        _lib.call('cdnet_bn_backward', C.byref(A), _lib.ptr(d['gamma']), _lib.ptr(dgamma), _lib.ptr(dbeta), _lib.ptr(wsb), wsb.numel(),
                  _lib.ptr(draw), _lib.ptr(dzo), _lib.stream_ptr())
        torch.cuda.synchronize()
        res.append((draw, dgamma, dbeta))
    for x, y in zip(*res):
        assert torch.equal(x, y)


@pytest.mark.parametrize('shape', [(3, 7, 9), (2, 192, 192)])
def test_fused_head_backward_is_deterministic(shape):
    import torch
    R = _reference(shape)
    d = _device_inputs(R)
    a, b = _fused(R, d), _fused(R, d)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_fused_kernel_needs_no_scratch():
    """the kernel holds 256 VGPRs only just (its scheduling barriers keep the LDS weight reads of several phases apart): a compiler that
    starts spilling shows here, not as a slower step"""
    from cdnet_amd import _lib
    assert _lib.load().cdnet_dam_head_backward_fused_scratch_bytes() == 0


def _first_backward(precision, fuse, monkeypatch):
    import torch
    import cdnet_amd
    from cdnet_amd import trainer
    from test_gpu_train_step import _setup, _hip_grads
    monkeypatch.setattr(trainer, 'HEAD_BWD_FUSE', fuse)
    before = cdnet_amd.get_precision()
    cdnet_amd.set_precision(precision)
    try:
        m, ref, x, t = _setup(B=2, S=64)
        tr, g = _hip_grads(m, x, t)
        return tr, g, tr.flat.G[:tr.flat.n_used].clone()
    finally:
        cdnet_amd.set_precision(before)


def test_trainer_takes_the_fused_entry_in_fp32_mode(monkeypatch):
    """one forward + backward of the small training setup with trainer.HEAD_BWD_FUSE off and on: the fused entry is really taken, and
    every parameter gradient is the same bit for bit"""
    import torch
    tr0, g0, flat0 = _first_backward('fp32', False, monkeypatch)
    tr1, g1, flat1 = _first_backward('fp32', True, monkeypatch)
    assert tr0.head_fused is False and tr1.head_fused is True
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
    assert torch.equal(flat0, flat1)
    assert torch.equal(g1['point_feature.conv_1x1.bias'], g1['point_feature.bn2.bias'])


def test_trainer_bf16_mode_ignores_the_switch(monkeypatch):
    import torch
    tr0, g0, _ = _first_backward('bf16', False, monkeypatch)
    tr1, g1, _ = _first_backward('bf16', True, monkeypatch)
    assert tr0.head_fused is False and tr1.head_fused is False
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
