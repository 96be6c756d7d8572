"""The fp32 head backward without stored dF1 / dF2: cdnet_dam_head_backward_coef leaves a pixel's 16 coefficients, and the sums pass of
the two residual units' bn2 (bn_bwd_flat32_kernel's head-coefficient form, cdnet_bn_bwd_args.hc_*) rebuilds its element of the gradient.
Nothing may change by a bit: the new head form against cdnet_dam_head_backward_fused and the two-kernel path's coefficient rows, the
rebuilt source against the same call with the dense tensor in its slot, the plans that cannot serve such a source refusing it, and two
whole training steps with the switch off and on.

Shapes are chosen for the kernels, not the workload.  Head: 1 x 24 x 20 (480 pixels: less than one chain stride of 32 768) and
2 x 136 x 128 (34 816: crosses that stride, the last 128-pixel group partly out of range).  Sums pass: 1 x 9 x 7 (63 pixels: a ragged
tail inside one workgroup) and 1 x 192 x 192 (36 864: more than 512 workgroups x 64 pixels, so the grid cap holds and the loop makes
more than one trip)."""
import ctypes as C
import functools

import pytest

from _head_coef_ref import K0, W0, rebuild

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _head_case(shape):
    """random fp32 inputs of the head backward and the results of the existing one-pass entry; made once per shape, nobody writes to them"""
    import torch
    from cdnet_amd import _lib, engine, runtime
    N, H, W = shape
    g = torch.Generator(device='cuda').manual_seed(29 + N * H * W)
    rnd = lambda *s: torch.randn(s, device='cuda', generator=g)
    d = dict(shape=shape, feats=[engine.Src(rnd(N, H, W, 64)) for _ in range(3)], gm=rnd(N, 3, H, W), gp=rnd(N, 1, H, W), gd=rnd(N, 9, H, W),
             hw=0.3 * rnd(855))
    d['hf'] = [runtime.head_feat(s) for s in d['feats']]
    lib = _lib.load()
    out = [torch.full((N, H, W, 64), 7.0, device='cuda') for _ in range(3)]
    ws = torch.full((lib.cdnet_dam_head_backward_fused_workspace_floats(),), float('nan'), device='cuda')
    dhw = torch.zeros((855,), device='cuda')
    hf = d['hf']
    _lib.call('cdnet_dam_head_backward_fused', C.byref(hf[0]), C.byref(hf[1]), C.byref(hf[2]), _lib.ptr(d['hw']), _lib.ptr(d['gm']),
              _lib.ptr(d['gp']), _lib.ptr(d['gd']), N, H, W, _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]), _lib.ptr(ws), ws.numel(),
              _lib.ptr(dhw), _lib.stream_ptr())
    torch.cuda.synchronize()
    d.update(df1=out[0], df2=out[1], dz3=out[2], dhw=dhw, ws=ws)
    return d


def _coef_form(d):
    import torch
    from cdnet_amd import _lib
    lib = _lib.load()
    N, H, W = d['shape']
    coef = torch.full((N, H, W, 16), 7.0, device='cuda')
    dz3 = torch.full((N, H, W, 64), 7.0, device='cuda')
    ws = torch.full((lib.cdnet_dam_head_backward_fused_workspace_floats(),), float('nan'), device='cuda')
    dhw = torch.zeros((855,), device='cuda')
    hf = d['hf']
    _lib.call('cdnet_dam_head_backward_coef', C.byref(hf[0]), C.byref(hf[1]), C.byref(hf[2]), _lib.ptr(d['hw']), _lib.ptr(d['gm']),
              _lib.ptr(d['gp']), _lib.ptr(d['gd']), N, H, W, _lib.ptr(coef), _lib.ptr(dz3), _lib.ptr(ws), ws.numel(), _lib.ptr(dhw),
              _lib.stream_ptr())
    torch.cuda.synchronize()
    return coef, dz3, dhw, ws


@pytest.mark.parametrize('shape', [(1, 24, 20), (2, 136, 128)])
def test_coefficient_form_of_the_head_backward(shape):
    """dz3, the 855 head gradients and every partial row and scalar chain in the workspace: the bits of cdnet_dam_head_backward_fused.
    The coefficient rows: the bits of the rows the two-kernel path keeps in its workspace, columns 13..15 zero; and for EVERY element the
    fma chain over them and the weight rows gives dF1 / dF2 of the existing entry bit for bit"""
    import torch
    from cdnet_amd import _lib
    d = _head_case(shape)
    N, H, W = shape
    coef, dz3, dhw, ws = _coef_form(d)
    assert torch.equal(dz3, d['dz3'])
    assert torch.equal(dhw, d['dhw'])
    assert torch.equal(ws.view(torch.int32), d['ws'].view(torch.int32))          # (bits: rows no workgroup writes stay NaN on both sides)
    assert bool((coef[..., 13:] == 0).all())
    old = [torch.empty((N, H, W, 64), device='cuda') for _ in range(3)]
    ws2 = torch.zeros((_lib.load().cdnet_dam_head_backward_workspace_floats(N, H, W),), device='cuda')
    dhw2 = torch.zeros((855,), device='cuda')
    hf = d['hf']
    _lib.call('cdnet_dam_head_backward', C.byref(hf[0]), C.byref(hf[1]), C.byref(hf[2]), _lib.ptr(d['hw']), _lib.ptr(d['gm']), _lib.ptr(d['gp']),
              _lib.ptr(d['gd']), N, H, W, _lib.ptr(old[0]), _lib.ptr(old[1]), _lib.ptr(old[2]), _lib.ptr(ws2), ws2.numel(), _lib.ptr(dhw2),
              _lib.stream_ptr())
    torch.cuda.synchronize()
    rows = ws2[1024 * 855:].reshape(N, H, W, 16)
    assert torch.equal(coef.view(torch.int32), rows.view(torch.int32))
    for nk, want in ((3, d['df1']), (9, d['df2'])):
        w = d['hw'][W0[nk]:W0[nk] + nk * 64].reshape(nk, 64)
        got = rebuild(coef, w, K0[nk], nk)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (nk, float((got - want).abs().max()))


def test_coefficient_form_needs_no_scratch():
    from cdnet_amd import _lib
    assert _lib.load().cdnet_dam_head_backward_coef_scratch_bytes() == 0


# ------------------------------------------------------------------------------------------------------
# the sums pass
# ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bn_case(shape, nk, zero_row):
    """one residual unit's bn2 with three gradient sources: raw output, stored unit output y (the mask), BatchNorm constants, two dense
    sources, and the third one twice - coefficient rows + weight rows, and the dense tensor the reference chain makes of them"""
    import torch
    N, H, W = shape
    g = torch.Generator(device='cuda').manual_seed(41 + N * H * W + nk)
    rnd = lambda *s: torch.randn(s, device='cuda', generator=g)
    d = dict(shape=shape, nk=nk, raw=rnd(N, H, W, 64), y=rnd(N, H, W, 64), g=[rnd(N, H, W, 64), rnd(N, H, W, 64)], coef=rnd(N, H, W, 16),
             w=0.3 * rnd(nk, 64), mean=0.1 * rnd(64), invstd=torch.rand(64, device='cuda', generator=g) + 0.5,
             gamma=(torch.rand(64, device='cuda', generator=g) + 0.5) * torch.where(torch.arange(64, device='cuda') % 4 == 0, -1.0, 1.0))
    if zero_row:
        # a source that is +0 everywhere (zero coefficients times negative weights: every product is -0), beside two sources of -0:
        # the sum of the three keeps the sign the chain's +0 start gives it
        d['coef'] = torch.zeros_like(d['coef'])
        d['w'] = -d['w'].abs() - 0.1
        d['g'] = [-torch.zeros_like(t) for t in d['g']]
    d['scale'] = d['gamma'] * d['invstd']
    d['shift'] = 0.2 * rnd(64) - d['mean'] * d['scale']
    d['dense'] = rebuild(d['coef'], d['w'], K0[nk], nk)
    return d


def _bn_backward(d, slot, coef_source, f16=2, window=False, sentinel=None):
    """cdnet_bn_backward over the case with the third source in `slot`; returns the status and everything the call leaves"""
    import torch
    from cdnet_amd import _lib
    lib = _lib.load()
    N, H, W = d['shape']
    A = _lib.BnBwdArgs()
    A.raw, A.res = d['raw'].data_ptr(), None if window else d['y'].data_ptr()
    A.scale, A.shift, A.mean, A.invstd = d['scale'].data_ptr(), d['shift'].data_ptr(), d['mean'].data_ptr(), d['invstd'].data_ptr()
    dense = list(d['g'])
    dense.insert(slot, d['dense'])
    A.ngin = 3
    for k in range(3):
        A.gin[k].g, A.gin[k].Hg, A.gin[k].Wg, A.gin[k].cstride = dense[k].data_ptr(), H, W, 64
    if coef_source:
        A.gin[slot].g = None
        A.hc_coef, A.hc_w, A.hc_slot, A.hc_k0, A.hc_nk = d['coef'].data_ptr(), d['w'].data_ptr(), slot, K0[d['nk']], d['nk']
    if window:                                           # BatchNorm + ReLU layer whose other consumer is a 2x2 max-pool: the window form
        kp = (slot + 1) % 3
        A.gin[kp].pooled, A.gin[kp].Hg, A.gin[kp].Wg = 1, H // 2, W // 2
    A.f16, A.relu, A.N, A.H, A.W, A.C = f16, 1 if window else 2, N, H, W, 64
    fill = float('nan') if sentinel is None else sentinel
    ws = torch.full((lib.cdnet_bn_backward_workspace_floats(64),), fill, device='cuda')
    dgamma, dbeta = torch.full((64,), fill, device='cuda'), torch.full((64,), fill, device='cuda')
    draw, dz = torch.full((N, H, W, 64), fill, device='cuda'), torch.full((N, H, W, 64), fill, device='cuda')
    rc = lib.cdnet_bn_backward(C.byref(A), _lib.ptr(d['gamma']), _lib.ptr(dgamma), _lib.ptr(dbeta), _lib.ptr(ws), ws.numel(), _lib.ptr(draw),
                               None if window else _lib.ptr(dz), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, dict(ws=ws, dgamma=dgamma, dbeta=dbeta, draw=draw, dz=dz, sums_plan=lib.cdnet_bn_backward_last_sums_plan(),
                    plan=lib.cdnet_bn_backward_last_plan())


def _assert_same_bits(a, b, shape):
    import torch
    N, H, W = shape
    # the plan: flat path, fp32, three sources, residual form, second pass on the stored dz; the workgroups of bn_grid
    nb = min(512, -(-N * H * W // 64))
    assert a['sums_plan'] == b['sums_plan'] == (2 | 1 << 2 | 3 << 3 | 1 << 5 | nb << 10)
    assert a['plan'] == b['plan'] == (2 | 1 << 2 | 1 << 3 | 1 << 8 | 1 << 9 | nb << 10)
    rows = nb * 2 * 64
    bits = lambda t: t.view(torch.int32)
    assert torch.equal(bits(a['ws'][:rows]), bits(b['ws'][:rows]))                          # partial rows
    assert torch.equal(bits(a['ws'][rows:rows + 192]), bits(b['ws'][rows:rows + 192]))      # k1 | k2 | k3
    for k in ('dgamma', 'dbeta', 'dz', 'draw'):
        assert torch.equal(bits(a[k]), bits(b[k])), k
        assert bool(torch.isfinite(a[k]).all()), k                                          # (everything was written)


@pytest.mark.parametrize('shape', [(1, 9, 7), (1, 192, 192)])
@pytest.mark.parametrize('nk', [3, 9])
@pytest.mark.parametrize('slot', [0, 1, 2])
def test_sums_pass_rebuilds_the_source_bit_for_bit(slot, nk, shape):
    """(a) the dense tensor in slot `slot`, (b) the head-coefficient source there: partial rows, dgamma, dbeta, k1 | k2 | k3, the stored
    dz and, after the second pass, dx - equal bits"""
    d = _bn_case(shape, nk, False)
    rc_a, a = _bn_backward(d, slot, False)
    rc_b, b = _bn_backward(d, slot, True)
    assert rc_a == 0 and rc_b == 0
    _assert_same_bits(a, b, shape)


@pytest.mark.parametrize('slot', [0, 2])
def test_zero_coefficients_give_plus_zero(slot):
    """zero coefficients, negative weights, the two dense sources -0: the rebuilt value is +0 (the chain starts from +0), so the sum of
    the three is +0 wherever the mask keeps it - the dz both forms store has no sign bit set"""
    import torch
    d = _bn_case((1, 9, 7), 9, True)
    assert not torch.signbit(d['dense']).any()
    rc_a, a = _bn_backward(d, slot, False)
    rc_b, b = _bn_backward(d, slot, True)
    assert rc_a == 0 and rc_b == 0
    _assert_same_bits(a, b, (1, 9, 7))
    assert not torch.signbit(b['dz']).any() and bool((b['dz'] == 0).all())


@pytest.mark.parametrize('kind', ['bf16', 'fp16', 'window'])
def test_plans_that_cannot_serve_the_source_refuse_it(kind):
    """16-bit tensors (the flat 16-bit kernels) and the window form (a pooled consumer beside it): CDNET_E_ARG before any launch, every
    output still holds its sentinel; the dense source in the same arguments is served (so it is the source that is refused)"""
    import torch
    from cdnet_amd import _lib
    d = _bn_case((1, 8, 8), 3, False)
    kw = dict(f16={'bf16': 0, 'fp16': 1, 'window': 2}[kind], window=kind == 'window', sentinel=-3.0)
    if kind == 'window':
        assert _bn_backward(d, 1, False, **kw)[0] == 0
    rc, o = _bn_backward(d, 1, True, **kw)
    assert rc == 1
    assert b'head-coefficient' in _lib.load().cdnet_last_error()
    for k in ('ws', 'dgamma', 'dbeta', 'draw', 'dz'):
        assert bool((o[k] == -3.0).all()), k


# ------------------------------------------------------------------------------------------------------
# the whole step
# ------------------------------------------------------------------------------------------------------
def _two_steps(on, monkeypatch):
    import torch
    import cdnet_amd
    from cdnet_amd import trainer
    from test_gpu_train_step import _setup
    monkeypatch.setattr(trainer, 'HEAD_COEF_SRC', on)
    before = cdnet_amd.get_precision()
    cdnet_amd.set_precision('fp32')
    try:
        m, ref, x, t = _setup(B=2, S=64)
        dev = torch.device('cuda:0')
        tr = trainer.Trainer(m)
        batch = (x.to(dev), t[0].to(dev), t[1].to(dev), t[2].to(dev), t[3][:, 0].contiguous().to(dev))
        losses = [tr.train_step(*batch).clone() for _ in range(2)]
        torch.cuda.synchronize()
        return tr, losses, tr.flat.P.clone(), {n: p.detach().clone() for n, p in m.named_parameters()}
    finally:
        cdnet_amd.set_precision(before)


def test_two_training_steps_with_the_switch_off_and_on(monkeypatch):
    import torch
    tr0, l0, flat0, p0 = _two_steps(False, monkeypatch)
    tr1, l1, flat1, p1 = _two_steps(True, monkeypatch)
    assert tr0.head_fused is True and tr1.head_fused is True
    assert tr0.head_coef is False and tr1.head_coef is True
    assert 'dF0' in tr0._bufs and 'dF1' in tr0._bufs and 'head_coef' not in tr0._bufs
    assert 'dF0' not in tr1._bufs and 'dF1' not in tr1._bufs and 'head_coef' in tr1._bufs
    for a, b in zip(l0, l1):
        assert torch.equal(a, b)
    assert torch.equal(flat0, flat1)
    for n in p0:
        assert torch.equal(p0[n], p1[n]), n
