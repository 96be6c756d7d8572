"""The non-convolution kernels of csrc/model.hip, each on its own against a plain float64 reference of the same operation
(tests/_model_kernel_refs.py, pinned on the CPU by test_model_kernel_refs_cpu.py).  Every comparison is per element:

  cdnet_bn_finalize_train / cdnet_bn_fold_eval   save_mean, save_invstd 1 fp32 ulp, scale 2 ulp; shift, running_mean, running_var
                                                 4 * 2^-24 * (sum of the absolute terms of their defining expression)
  dam_head_fwd_kernel<1>, <2>, final_conv1x1     |got - want| <= 2^-16 * S per logit, S = the logit expression over absolute values
  input pack, window pack, window stitch         equal bits

Outputs are filled with a sentinel before each call: every element must be written, nothing beyond them.  Each check prints its worst
|err| / bound ("RATIO <kernel> <output> <value>") before it asserts."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _model_kernel_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 8               # sentinel elements behind every output row
E_ARG = 1               # CDNET_E_ARG


def _check(kernel, what, got, want, bound):
    """per element |got - want| <= bound (float64 arrays of one shape)"""
    got, want, bound = R.f64(got), R.f64(want), R.f64(bound)
    assert got.shape == want.shape == bound.shape, (kernel, what, got.shape, want.shape, bound.shape)
    assert np.all(np.isfinite(got)), (kernel, what, 'not finite')
    err = np.abs(got - want)
    ratio = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
    i = int(np.argmax(ratio)) if ratio.size else 0
    print('RATIO %s %s %.4f' % (kernel, what, float(ratio.reshape(-1)[i]) if ratio.size else 0.0))
    assert np.all(err <= bound), (kernel, what, 'worst |err| / bound', float(ratio.reshape(-1)[i]), 'at', np.unravel_index(i, ratio.shape),
                                  'got', float(got.reshape(-1)[i]), 'want', float(want.reshape(-1)[i]))


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _rows(n, C):
    """n output rows of C floats, GUARD sentinels behind each"""
    import torch
    return torch.full((n, C + GUARD), R.SENTINEL, dtype=torch.float32, device='cuda')


def _untouched(t):
    import torch
    return bool(torch.all(t == torch.tensor(R.SENTINEL, dtype=t.dtype, device=t.device)))


def _written(t):
    import torch
    return not bool(torch.any(t == torch.tensor(R.SENTINEL, dtype=t.dtype, device=t.device)))


# ----------------------------------------------------------------------------------------------------------------------------------
# 1. cdnet_bn_finalize_train
# ----------------------------------------------------------------------------------------------------------------------------------
BN_SHAPES = [(1, 1, 2), (3, 5, 4), (256, 64, 8192), (257, 3, 771), (1000, 130, 32000), (2, 7, 1)]


def _finalize(stats, count, c, eps, mom, with_bias=True, with_running=True, with_save=True):
    """one call on the case c (bn_stats_case layout).  Returns the 6 output rows [scale, shift, mean, invstd, rm, rv] (host, with
    their guards) after checking that rows that were not passed stayed untouched"""
    import torch
    from cdnet_amd import _lib
    T, _, Cc = stats.shape
    out = _rows(6, Cc)
    if with_running:
        out[4, :Cc], out[5, :Cc] = _dev(c['rm']), _dev(c['rv'])
    st, g, b, bias = _dev(stats), _dev(c['g']), _dev(c['b']), _dev(c['bias'])
    p = lambda i, on=True: _lib.ptr(out[i]) if on else None
    _lib.call('cdnet_bn_finalize_train', _lib.ptr(st), T, Cc, float(count), _lib.ptr(g), _lib.ptr(b), _lib.ptr(bias) if with_bias else None,
              float(eps), float(mom), p(4, with_running), p(5, with_running), p(0), p(1), p(2, with_save), p(3, with_save), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert _untouched(out[:, Cc:]), 'wrote behind an output row'
    if not with_running:
        assert _untouched(out[4:6])
    if not with_save:
        assert _untouched(out[2:4])
    return out.cpu().numpy()[:, :Cc]


def _check_finalize(got, r, with_running, with_save, tag):
    tol = r['tol']
    _check('bn_finalize_train', 'scale' + tag, got[0], r['scale'], tol['scale'])
    _check('bn_finalize_train', 'shift' + tag, got[1], r['shift'], tol['shift'])
    if with_save:
        _check('bn_finalize_train', 'save_mean' + tag, got[2], r['mean'], tol['mean'])
        _check('bn_finalize_train', 'save_invstd' + tag, got[3], r['invstd'], tol['invstd'])
    if with_running:
        _check('bn_finalize_train', 'running_mean' + tag, got[4], r['running_mean'], tol['running_mean'])
        _check('bn_finalize_train', 'running_var' + tag, got[5], r['running_var'], tol['running_var'])


def _f32(x):
    """the float64 value of the fp32 number a float argument becomes at the ABI"""
    return float(np.float32(x))


@pytest.mark.parametrize('shape', BN_SHAPES)
def test_bn_finalize_train_vs_fp64_over_the_same_stats(shape):
    """every output against the float64 reference over the SAME fp32 statistics; channels of all data regimes mixed in one call
    (well conditioned, mean 100 / std 0.01, constant, q / count - mean^2 slightly negative, negative gamma); T = 1 .. 1000 covers the
    256-thread strided loop and the LDS tree, count == 1 the unbiased-factor guard"""
    T, Cc, count = shape
    c = R.bn_stats_case(T, Cc, count, seed=T + Cc, regime_offset=BN_SHAPES.index(shape))
    eps, mom = _f32(1e-5), _f32(0.1)
    got = _finalize(c['stats'], count, c, eps, mom)
    r = R.ref_bn_finalize(c['stats'], count, c['g'], c['b'], c['bias'], eps, mom, c['rm'], c['rv'])
    _check_finalize(got, r, True, True, '')
    neg = [i for i, reg in enumerate(c['regimes']) if reg == 'negvar']
    if neg:
        # the regime is what it claims: unclamped negative in float64; the clamp gives invstd = 1 / sqrt(eps) and adds 0 to running_var
        st = c['stats'].astype(np.float64)
        m = st[:, 0, neg].sum(0) / count
        assert np.all(st[:, 1, neg].sum(0) / count - m * m < 0) and np.all(r['var'][neg] == 0)
        _check('bn_finalize_train', 'clamped invstd', got[3][neg], np.full(len(neg), 1 / np.sqrt(eps)), R.ulp32(np.full(len(neg), 1 / np.sqrt(eps))))
        _check('bn_finalize_train', 'clamped running_var', got[5][neg], (1 - mom) * c['rv'][neg].astype(np.float64), R.terms_tol((1 - mom) * c['rv'][neg]))
    if count == 1:
        assert np.all(np.isfinite(got))
    # two calls on the same input give equal bits
    again = _finalize(c['stats'], count, c, eps, mom)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))


@pytest.mark.parametrize('shape', [(3, 5, 4), (257, 3, 771), (2, 7, 1)])
def test_bn_finalize_train_switches(shape):
    """conv_bias NULL / given x running statistics NULL / given x saved statistics NULL / given x (momentum, eps) in
    (0.1, 1e-5), (0.37, 1e-3): buffers that are not passed keep their sentinel, the others meet the reference"""
    T, Cc, count = shape
    c = R.bn_stats_case(T, Cc, count, seed=11 * T + Cc, regime_offset=1 + BN_SHAPES.index(shape))
    for with_bias in (False, True):
        for with_running in (False, True):
            for with_save in (False, True):
                for mom, eps in ((0.1, 1e-5), (0.37, 1e-3)):
                    mom, eps = _f32(mom), _f32(eps)
                    got = _finalize(c['stats'], count, c, eps, mom, with_bias, with_running, with_save)
                    r = R.ref_bn_finalize(c['stats'], count, c['g'], c['b'], c['bias'] if with_bias else None, eps, mom,
                                          c['rm'] if with_running else None, c['rv'] if with_running else None)
                    _check_finalize(got, r, with_running, with_save, ' bias=%d run=%d save=%d mom=%.2f' % (with_bias, with_running, with_save, mom))


@pytest.mark.parametrize('count', [2, 4, 32, 771])
def test_bn_finalize_train_is_batchnorm2d_train(count):
    """semantics: data on a 2^-6 grid in uneven tiles of at most 64 pixels (every fp32 tile sum exact, asserted by the builder), the
    kernel against nn.BatchNorm2d(train) in float64 over x + bias: running_mean carries the bias, running_var the unbiased variance
    (factor 2 and 4 / 3 at count 2 and 4), the output is x * scale + shift"""
    import torch
    Cc = 6
    x, stats = R.bn_grid_case(Cc, count, seed=count)
    rng = np.random.default_rng(100 + count)
    c = dict(g=np.float32(rng.uniform(0.5, 1.5, Cc) * rng.choice([-1.0, 1.0], Cc)), b=np.float32(rng.standard_normal(Cc)),
             bias=np.float32(rng.standard_normal(Cc)), rm=np.float32(rng.standard_normal(Cc)), rv=np.float32(rng.uniform(0.5, 2, Cc)))
    eps, mom = _f32(1e-5), _f32(0.1)
    got = _finalize(stats, count, c, eps, mom)
    bn = torch.nn.BatchNorm2d(Cc, eps=eps, momentum=mom).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(c['g']).double()); bn.bias.copy_(torch.from_numpy(c['b']).double())
        bn.running_mean.copy_(torch.from_numpy(c['rm']).double()); bn.running_var.copy_(torch.from_numpy(c['rv']).double())
        y = bn(torch.from_numpy(x).view(1, Cc, count, 1) + torch.from_numpy(c['bias']).double().view(1, Cc, 1, 1))[0, :, :, 0].numpy()
    r = R.ref_bn_finalize(stats, count, c['g'], c['b'], c['bias'], eps, mom, c['rm'], c['rv'])      # (for the bounds)
    tol = r['tol']
    _check('bn_finalize_train', 'running_mean vs BatchNorm2d', got[4], bn.running_mean.numpy(), tol['running_mean'])
    _check('bn_finalize_train', 'running_var vs BatchNorm2d', got[5], bn.running_var.numpy(), tol['running_var'])
    _check('bn_finalize_train', 'save_mean vs data', got[2], x.mean(1), tol['mean'])
    _check('bn_finalize_train', 'save_invstd vs data', got[3], 1 / np.sqrt(x.var(1) + eps), tol['invstd'])
    _check('bn_finalize_train', 'scale vs data', got[0], c['g'] / np.sqrt(x.var(1) + eps), tol['scale'])
    # y = x * scale + shift: the scale's 2 ulp times |x| plus the shift's bound
    _check('bn_finalize_train', 'output vs BatchNorm2d', x * got[0].astype(np.float64)[:, None] + got[1].astype(np.float64)[:, None], y,
           np.abs(x) * tol['scale'][:, None] + tol['shift'][:, None])


# ----------------------------------------------------------------------------------------------------------------------------------
# 2. cdnet_bn_fold_eval
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Cc', [1, 64, 257])
def test_bn_fold_eval_vs_fp64(Cc):
    """C across the 256-thread workgroup, bias NULL / given, running_var entries of 0 and 1e-12 beside ordinary ones, two eps"""
    import torch
    from cdnet_amd import _lib
    rng = np.random.default_rng(Cc)
    g = np.float32(rng.uniform(0.5, 1.5, Cc) * rng.choice([-1.0, 1.0], Cc))
    b, bias, rm = np.float32(rng.standard_normal(Cc)), np.float32(rng.standard_normal(Cc)), np.float32(rng.standard_normal(Cc))
    for first in (0.0, 1e-12, 0.7):
        rv = np.float32(rng.uniform(0.5, 2, Cc))
        rv[0] = first
        if Cc > 1:
            rv[Cc - 1], rv[Cc // 2] = 1e-12, 0.0
        for with_bias in (False, True):
            for eps in (_f32(1e-5), _f32(1e-3)):
                out = _rows(2, Cc)
                d = [_dev(a) for a in (g, b, rm, rv, bias)]
                _lib.call('cdnet_bn_fold_eval', _lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(d[2]), _lib.ptr(d[3]), _lib.ptr(d[4]) if with_bias else None,
                          eps, Cc, _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.stream_ptr())
                torch.cuda.synchronize()
                assert _untouched(out[:, Cc:])
                got = out.cpu().numpy()[:, :Cc]
                r = R.ref_bn_fold(g, b, rm, rv, bias if with_bias else None, eps)
                _check('bn_fold_eval', 'scale', got[0], r['scale'], r['tol']['scale'])
                _check('bn_fold_eval', 'shift', got[1], r['shift'], r['tol']['shift'])


# ----------------------------------------------------------------------------------------------------------------------------------
# 3. / 4. lazily transformed features: the DAM head on the vector units, the plain classifier
# ----------------------------------------------------------------------------------------------------------------------------------
KINDS = {   # storage, affine, residual, relu
    'train16': ('f16', True, True, True),                # fp16 raw * scale + shift + fp16 residual -> ReLU (xf_bnrelu_f16<true>)
    'train16_nores': ('f16', True, False, True),         # the same without residual (xf_bnrelu_f16<false>)
    'addrelu16': ('f16', False, True, True),             # eval-mode residual unit: relu(raw + res) (xf_addrelu_f16)
    'bf16_affine_relu': ('bf16', True, False, True),     # generic loop
    'bf16_res': ('bf16', False, True, False),            # generic loop, no ReLU
    'plain16': ('f16', False, False, False),             # fp16 values as they are: nothing is rounded
    'plainbf': ('bf16', False, False, False),
    'f32_full': ('f32', True, True, True),               # fp32 storage: plain fp32 arithmetic, nothing rounded to 16 bits
}
C_ZERO, C_NEG0, C_ZEROS = 5, 9, 13        # channels with: pre-ReLU value exactly 0; tiny negative (-0 in bf16); raw = res = shift = 0


class _Feat:
    """a 64-channel feature on the device (tensors kept alive here), its cdnet_head_feat and Src"""


def _feature(kind, shape, seed):
    """16-bit kinds hold grid values (raw, shift, residual on 2^-4, scale on 2^-3): raw * scale + shift + res is exact in fp32 and in
    float64 (at most 11 bits), so the stored bf16 feature is the rounding of the exact value and no cancellation can spoil the one-ulp
    check of _feature_values.  Negative scales on every fourth channel; channels C_ZERO, C_NEG0, C_ZEROS as named above."""
    import torch
    from cdnet_amd import engine, runtime
    storage, affine, has_res, relu = KINDS[kind]
    dt = {'f16': torch.float16, 'bf16': torch.bfloat16, 'f32': torch.float32}[storage]
    N, H, W = shape
    g = torch.Generator(device='cuda').manual_seed(seed)
    grid = lambda shp, lo, hi, step: torch.randint(lo, hi + 1, shp, generator=g, device='cuda').float() * step
    f = _Feat()
    if storage == 'f32':
        raw = torch.randn((N, H, W, 64), generator=g, device='cuda')
        res = torch.randn((N, H, W, 64), generator=g, device='cuda')
        scale = torch.rand(64, generator=g, device='cuda') + 0.5
        shift = torch.randn(64, generator=g, device='cuda') * 0.3
    elif not affine and not has_res:
        raw = torch.randn((N, H, W, 64), generator=g, device='cuda').to(dt).float()      # all the bits of the storage type
        res = scale = shift = None
    else:
        # (without the affine the residual sits on 2^-7: raw + res then has up to 11 bits and the rounding to bf16 still matters)
        raw, res = grid((N, H, W, 64), -64, 64, 2.0 ** -4), grid((N, H, W, 64), -64, 64, 2.0 ** (-4 if affine else -7))
        scale, shift = grid((64,), 4, 12, 2.0 ** -3), grid((64,), -16, 16, 2.0 ** -4)
    if affine:
        scale[1::4] *= -1.0
    if affine or has_res:
        raw[..., C_ZEROS] = 0.0
        res[..., C_ZEROS] = 0.0
        if affine:
            shift[C_ZEROS] = 0.0
            scale[C_ZERO], shift[C_ZERO] = 2.0, 0.5
            res[..., C_ZERO] = -(2.0 * raw[..., C_ZERO] + 0.5)
            if not has_res:
                raw[..., C_ZERO], shift[C_ZERO] = 0.0, 0.0
            scale[C_NEG0], shift[C_NEG0] = -(2.0 ** -140), 0.0           # (an fp32 subnormal: the product rounds to -0 in bf16)
            raw[..., C_NEG0] = raw[..., C_NEG0].abs() + 2.0 ** -4
            res[..., C_NEG0] = 0.0
        else:
            res[..., C_ZERO] = -raw[..., C_ZERO]
    f.raw = raw.to(dt).contiguous()
    f.res = res.to(dt).contiguous() if has_res else None
    f.scale, f.shift = (scale.contiguous(), shift.contiguous()) if affine else (None, None)
    assert torch.equal(f.raw.float(), raw) and (f.res is None or torch.equal(f.res.float(), res)), 'the storage type holds the inputs exactly'
    f.src = engine.Src(f.raw, f.scale, f.shift, relu=relu, res=f.res)
    f.hf = runtime.head_feat(f.src)
    f.kind, f.relu, f.storage, f.plain = kind, relu, storage, not (affine or has_res or relu)
    return f


def _feature_values(f, ranges):
    """the feature values the kernels see at the pixels of `ranges`, float64 [P'][64].  Transformed 16-bit features: the bf16 tensor
    cdnet_src_materialize writes (documented bit-identical to the staging transform, pinned to PyTorch by test_gpu_conv.py) - checked
    here, element by element, to lie within one bf16 ulp of the float64 transform.  Plain and fp32-stored features: the float64 values."""
    import torch
    from cdnet_amd import runtime
    cut = lambda t: torch.cat([t.reshape(-1, 64)[a:b] for a, b in ranges]).double().cpu().numpy()
    want = R.ref_transform(cut(f.raw), None if f.scale is None else f.scale.double().cpu().numpy(),
                           None if f.shift is None else f.shift.double().cpu().numpy(), None if f.res is None else cut(f.res), f.relu)
    if f.storage == 'f32' or f.plain:
        return want
    if not hasattr(f, 'stored'):
        f.stored = runtime.materialize(f.src).x
        torch.cuda.synchronize()
    got = cut(f.stored)
    _check('src_materialize', f.kind, got, want, R.ulp_bf16(want))
    if f.relu:
        assert np.all(got[:, [C_ZERO, C_NEG0, C_ZEROS] if f.scale is not None else [C_ZERO, C_ZEROS]] == 0)
    return got


def _head_weights(seed):
    """fp32 block in the CDNET_HEAD_WEIGHT_FLOATS layout: classifier rows U(-1/8, 1/8) (nn.Conv2d's bound for 64 inputs), gates with
    weights of distinct size so that a swapped gate or gate weight moves the logits"""
    rng = np.random.default_rng(seed)
    hw = rng.uniform(-0.125, 0.125, 855)
    hw[845] = 0.7                                                    # directionAtt.Conv1x1
    hw[846:855] = rng.uniform(0.1, 1 / 3, 9) * rng.choice([-1.0, 1.0], 9)      # maskAtt.Conv1x1
    return np.float32(hw)


HEAD_CONFIGS = {
    '1_train_res': ('train16', 'train16', 'train16'),                         # dam_head_fwd_kernel<1>
    '2_one_without_res': ('train16', 'train16_nores', 'train16'),             # <2>, packed path, RES = false
    '3_eval_residual_unit': ('addrelu16', 'addrelu16', 'addrelu16'),          # xf_addrelu_f16
    '4a_bf16_affine_relu': ('bf16_affine_relu', 'bf16_affine_relu', 'bf16_affine_relu'),
    '4b_bf16_res_no_relu': ('bf16_res', 'bf16_res', 'bf16_res'),
    '5_fp16_untransformed': ('plain16', 'plain16', 'plain16'),
    '6_flags_per_feature': ('plainbf', 'train16', 'addrelu16'),
    '7a_fp32_full': ('f32_full', 'f32_full', 'f32_full'),
    '7b_fp32_beside_16bit': ('train16', 'f32_full', 'bf16_affine_relu'),      # all16 == false
}


def _run_head(config, shape, ranges=None):
    import torch
    from cdnet_amd import _lib
    N, H, W = shape
    P = N * H * W
    ranges = ranges or [(0, P)]
    feats = [_feature(kind, shape, seed=31 * k + len(config) + H) for k, kind in enumerate(HEAD_CONFIGS[config])]
    hw = _head_weights(7)
    hw_d = _dev(hw)
    mask = torch.full((N, 3, H, W), R.SENTINEL, device='cuda'); point = torch.full((N, 1, H, W), R.SENTINEL, device='cuda')
    dirn = torch.full((N, 9, H, W), R.SENTINEL, device='cuda')
    _lib.call('cdnet_dam_head_forward', C.byref(feats[0].hf), C.byref(feats[1].hf), C.byref(feats[2].hf), _lib.ptr(hw_d), N, H, W,
              _lib.ptr(mask), _lib.ptr(point), _lib.ptr(dirn), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert _written(mask) and _written(point) and _written(dirn), 'an output element was not written'
    F = [_feature_values(f, ranges) for f in feats]
    (w_mask, w_point, w_dir), (S_mask, S_point, S_dir) = R.ref_head(F[0], F[1], F[2], hw)
    cut = lambda t, K: torch.cat([t.permute(0, 2, 3, 1).reshape(P, K)[a:b] for a, b in ranges]).double().cpu().numpy()
    _check('dam_head_fwd', config + ' point', cut(point, 1)[:, 0], w_point, R.HEAD_EPS * S_point)
    _check('dam_head_fwd', config + ' direction', cut(dirn, 9), w_dir, R.HEAD_EPS * S_dir)
    _check('dam_head_fwd', config + ' mask', cut(mask, 3), w_mask, R.HEAD_EPS * S_mask)


@pytest.mark.parametrize('shape', [(1, 1, 1), (3, 7, 9), (2, 24, 20)])
@pytest.mark.parametrize('config', sorted(HEAD_CONFIGS))
def test_dam_head_over_transformed_features(config, shape):
    """dam_head_fwd_kernel<1> / <2> on every storage / transform branch of the feature loaders, per logit against ref_head over the
    features the kernel sees.  (1, 1, 1): three lanes of the quad group clamped to the last pixel; 189 pixels: a ragged last group"""
    _run_head(config, shape)


def test_dam_head_grid_stride_second_iteration():
    """262 600 pixels > 4096 workgroups x 64: the grid-stride loop of dam_head_fwd_kernel<1> runs twice for the first 456 pixels' worth
    of workgroups.  Reference on the first 4096, the last 4096 and the pixels around 262 144."""
    shape = (1, 520, 505)
    _run_head('1_train_res', shape, R.sample_ranges(520 * 505, 4096 * 64))


def test_dam_head_given_point_needs_plain_features():
    """f3->raw = NULL (point given) with a transformed f1: the argument error, nothing written"""
    import torch
    from cdnet_amd import _lib, runtime
    shape = (1, 4, 4)
    f1, f2 = _feature('train16', shape, 1), _feature('plainbf', shape, 2)
    hw_d = _dev(_head_weights(7))
    outs = [torch.full((1, k, 4, 4), R.SENTINEL, device='cuda') for k in (3, 1, 9)]
    none = runtime.HeadFeat()
    rc = _lib.load().cdnet_dam_head_forward(C.byref(f1.hf), C.byref(f2.hf), C.byref(none), _lib.ptr(hw_d), 1, 4, 4, _lib.ptr(outs[0]),
                                            _lib.ptr(outs[1]), _lib.ptr(outs[2]), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == E_ARG and all(_untouched(t) for t in outs)


def _run_final(kind, shape, Ks, ranges=None):
    import torch
    from cdnet_amd import _lib
    N, H, W = shape
    P = N * H * W
    ranges = ranges or [(0, P)]
    f = _feature(kind, shape, seed=5 + H)
    F = _feature_values(f, ranges)
    rng = np.random.default_rng(H)
    for K in Ks:
        w, b = np.float32(rng.uniform(-0.125, 0.125, (K, 64))), np.float32(rng.uniform(-1, 1, K))
        w_d, b_d = _dev(w), _dev(b)
        out = torch.full((N * K * H * W + GUARD,), R.SENTINEL, device='cuda')
        _lib.call('cdnet_final_conv1x1', C.byref(f.hf), _lib.ptr(w_d), _lib.ptr(b_d), K, N, H, W, _lib.ptr(out), _lib.stream_ptr())
        torch.cuda.synchronize()
        assert _written(out[:N * K * H * W]) and _untouched(out[N * K * H * W:])
        got = out[:N * K * H * W].view(N, K, H, W).permute(0, 2, 3, 1).reshape(P, K)
        want, S = R.ref_conv1x1(F, w, b)
        _check('final_conv1x1', '%s K=%d' % (kind, K), torch.cat([got[a:b_] for a, b_ in ranges]).double().cpu().numpy(), want, R.HEAD_EPS * S)


@pytest.mark.parametrize('shape', [(1, 1, 1), (3, 7, 9), (2, 24, 20)])
@pytest.mark.parametrize('kind', ['plainbf', 'train16_nores', 'bf16_res', 'f32_full'])
def test_final_conv1x1_vs_fp64(kind, shape):
    """the plain UNet's / ablation heads' classifier for K = 1, 3, 17, 32 over plain bf16, fp16 x scale + shift -> ReLU, bf16 + residual
    and fully transformed fp32 features"""
    _run_final(kind, shape, (1, 3, 17, 32))


def test_final_conv1x1_grid_stride_second_iteration():
    """1025 x 1024 pixels > 4096 workgroups x 256: the only size at which final_conv1x1_kernel's loop iterates"""
    _run_final('plainbf', (1, 1025, 1024), (3,), R.sample_ranges(1025 * 1024, 4096 * 256))


@pytest.mark.parametrize('K', [0, 33])
def test_final_conv1x1_refuses_K_outside_1_32(K):
    import torch
    from cdnet_amd import _lib
    f = _feature('plainbf', (1, 2, 2), 3)
    w_d, b_d = _dev(np.zeros((33, 64))), _dev(np.zeros(33))
    out = torch.full((33 * 4,), R.SENTINEL, device='cuda')
    rc = _lib.load().cdnet_final_conv1x1(C.byref(f.hf), _lib.ptr(w_d), _lib.ptr(b_d), K, 1, 2, 2, _lib.ptr(out), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == E_ARG and _untouched(out)


# ----------------------------------------------------------------------------------------------------------------------------------
# 5. packing and stitching: equal bits
# ----------------------------------------------------------------------------------------------------------------------------------
SPECIALS = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -0.0, 3.3895313892515355e38, -(1 + 2.0 ** -8), 0.0, 1 + 2.0 ** -8 + 2.0 ** -20, 2 - 2.0 ** -10]
#           bf16 ties (to even: down, up), negative zero, the largest finite bf16, a negative tie, zero, just above a tie, up into the next binade


@pytest.mark.parametrize('shape', [(1, 1, 1), (3, 7, 9)])
@pytest.mark.parametrize('Cc', [1, 3, 16])
def test_input_pack_bits(Cc, shape):
    """cdnet_input_pack == x.to(bfloat16) in NHWC with zero channels behind C; cdnet_input_pack_f32 == the permuted input; nothing
    written behind [N][H][W][16] (a guard row)"""
    import torch
    from cdnet_amd import _lib
    N, H, W = shape
    P = N * H * W
    for rot in range(len(SPECIALS) if P * Cc < len(SPECIALS) else 1):
        x = torch.randn((N, Cc, H, W), generator=torch.Generator().manual_seed(Cc + H))
        sp = torch.tensor(SPECIALS[rot:] + SPECIALS[:rot], dtype=torch.float32)
        n = min(sp.numel(), x.numel())
        x.view(-1)[:n] = sp[:n]
        x_d = x.cuda()
        want = torch.zeros((N, H, W, 16), dtype=torch.float32)
        want[..., :Cc] = x.permute(0, 2, 3, 1)
        out16 = torch.full((P + 1, 16), R.SENTINEL, dtype=torch.bfloat16, device='cuda')
        out32 = torch.full((P + 1, 16), R.SENTINEL, dtype=torch.float32, device='cuda')
        _lib.call('cdnet_input_pack', _lib.ptr(x_d), N, Cc, H, W, _lib.ptr(out16), _lib.stream_ptr())
        _lib.call('cdnet_input_pack_f32', _lib.ptr(x_d), N, Cc, H, W, _lib.ptr(out32), _lib.stream_ptr())
        torch.cuda.synchronize()
        assert _untouched(out16[P]) and _untouched(out32[P])
        assert torch.equal(out16[:P].cpu().view(torch.int16), want.to(torch.bfloat16).view(P, 16).view(torch.int16))
        assert torch.equal(out32[:P].cpu().view(torch.int32), want.view(P, 16).view(torch.int32))


@pytest.mark.parametrize('K', [1, 3, 9])
@pytest.mark.parametrize('geo', R.STITCH_GEOMETRIES)
def test_window_stitch_bits(geo, K):
    """cdnet_window_stitch on tiles whose value is their own flat index - (window, k, y, x), exact in fp32 - against the reference's
    loop (ref_stitch), for the geometries of utils.window_grid: ragged, exact fit, odd overlap, one row of windows, one window"""
    import torch
    from cdnet_amd import _lib, utils
    hv, wv, size, overlap = geo
    stride, th, tw, ny, nx = utils.window_grid(hv, wv, size, overlap)
    total = ny * nx * K * th * tw
    assert total < 2 ** 24
    tiles = np.arange(total, dtype=np.float32).reshape(ny * nx, K, th, tw)
    t_d = _dev(tiles)
    out = torch.full((K * hv * wv + GUARD,), R.SENTINEL, device='cuda')
    _lib.call('cdnet_window_stitch', _lib.ptr(t_d), K, th, tw, stride, overlap, ny, nx, hv, wv, _lib.ptr(out), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert _untouched(out[K * hv * wv:])
    got = out[:K * hv * wv].view(K, hv, wv).cpu().numpy()
    want = R.ref_stitch(tiles, size, overlap, hv, wv)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.argwhere(got != want)[:4]


@pytest.mark.parametrize('axis', ['rows', 'columns'])
def test_window_stitch_refuses_tiles_shorter_than_their_interior(axis):
    """two windows whose tiles cover the view but are shorter than stride + overlap / 2: a window that is not the last would be read
    past its tile's end (into the next row / channel of the tile tensor) - the argument error, nothing written"""
    import torch
    from cdnet_amd import _lib
    stride, overlap, short, full = 16, 8, 18, 24          # 18 < 16 + 4; (2 - 1) * 16 + 18 = 34 covers 30
    th, tw, ny, nx, hv, wv = (short, full, 2, 1, 30, 24) if axis == 'rows' else (full, short, 1, 2, 24, 30)
    t_d = torch.zeros((ny * nx, 3, th, tw), device='cuda')
    out = torch.full((3 * hv * wv,), R.SENTINEL, device='cuda')
    rc = _lib.load().cdnet_window_stitch(_lib.ptr(t_d), 3, th, tw, stride, overlap, ny, nx, hv, wv, _lib.ptr(out), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == E_ARG and _untouched(out)
    # the same tiles with one window along that axis are fine (the last window is read to the view's end only)
    hv1, wv1 = (short, wv) if axis == 'rows' else (hv, short)
    out = torch.full((3 * hv1 * wv1,), R.SENTINEL, device='cuda')
    _lib.call('cdnet_window_stitch', _lib.ptr(t_d), 3, th, tw, stride, overlap, 1, 1, hv1, wv1, _lib.ptr(out), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert _written(out)
