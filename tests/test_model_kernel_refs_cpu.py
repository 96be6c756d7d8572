"""The float64 references of tests/_model_kernel_refs.py against PyTorch (nn.BatchNorm2d on float64) and the oracle (the DAM head's
modules, the sliding-window loop of oracle/infer.py) - on the CPU, so that the references are known good before a GPU is involved.
Both sides compute in float64: the bounds are a few float64 roundings of the sum of the absolute terms (64 * 2^-53 * S)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _model_kernel_refs as R  # noqa: E402

F64_TOL = 64 * 2.0 ** -53


def _close(got, want, scale, what):
    err = np.abs(np.asarray(got) - np.asarray(want))
    assert np.all(err <= F64_TOL * scale), (what, float((err / (F64_TOL * scale + 1e-300)).max()))


def _data_stats(x, T):
    """x [C][count] float64 -> stats float64 [T][2][C] over T uneven tiles"""
    C, count = x.shape
    edges = np.concatenate([[0], np.cumsum(R.tile_counts(T, count))])
    st = np.zeros((T, 2, C))
    for t in range(T):
        seg = x[:, edges[t]:edges[t + 1]]
        st[t, 0], st[t, 1] = seg.sum(1), (seg * seg).sum(1)
    return st


@pytest.mark.parametrize('case', [(1, 3, 2, True, 0.1, 1e-5), (3, 5, 4, False, 0.1, 1e-5), (7, 6, 32, True, 0.37, 1e-3), (19, 4, 771, True, 0.1, 1e-5)])
def test_ref_bn_finalize_is_batchnorm2d_train(case):
    import torch
    T, C, count, with_bias, mom, eps = case
    rng = np.random.default_rng(count)
    x = rng.standard_normal((C, count)) + rng.uniform(-2, 2, (C, 1))
    g, b, bias = rng.uniform(0.5, 1.5, C) * rng.choice([-1.0, 1.0], C), rng.standard_normal(C), rng.standard_normal(C)
    rm, rv = rng.standard_normal(C), rng.uniform(0.5, 2, C)
    bn = torch.nn.BatchNorm2d(C, eps=eps, momentum=mom).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(g)); bn.bias.copy_(torch.from_numpy(b))
        bn.running_mean.copy_(torch.from_numpy(rm)); bn.running_var.copy_(torch.from_numpy(rv))
        z = torch.from_numpy(x).view(1, C, count, 1)
        y = bn(z + (torch.from_numpy(bias).view(1, C, 1, 1) if with_bias else 0.0))[0, :, :, 0].numpy()
    r = R.ref_bn_finalize(_data_stats(x, T), count, g, b, bias if with_bias else None, eps, mom, rm, rv)
    # the BatchNorm output over z + bias is z * scale + shift (the bias cancels in the normalisation)
    mag = (np.abs(x) + np.abs(r['mean'])[:, None] + 1) * np.abs(r['scale'])[:, None] * (1 + (r['mean'] ** 2 / (r['var'] + eps))[:, None]) + np.abs(b)[:, None]
    _close(x * r['scale'][:, None] + r['shift'][:, None], y, mag, 'y')
    _close(r['running_mean'], bn.running_mean.numpy(), np.abs(rm) + np.abs(r['mean']) + np.abs(bias), 'running_mean')
    _close(r['running_var'], bn.running_var.numpy(), np.abs(rv) + (np.abs(r['mean']) ** 2 + r['var']) * 2, 'running_var')
    _close(r['mean'], x.mean(1), np.abs(x).mean(1), 'mean')
    _close(r['var'], x.var(1), (x * x).mean(1), 'var')
    if count in (2, 4):           # the unbiased factor count / (count - 1) is 2 and 4 / 3
        unb = (bn.running_var.numpy() - (1 - mom) * rv) / mom
        assert np.allclose(unb / x.var(1), count / (count - 1.0), rtol=2.0 ** -40, atol=0)


def test_ref_bn_finalize_guards():
    """count == 1 uses the factor 1, a negative q / count - mean^2 is clamped, outputs without running statistics are None"""
    st = np.zeros((2, 2, 2))
    st[0, 0], st[0, 1] = [3.0, 2.0], [np.nextafter(9.0, 0), 4.0]
    r = R.ref_bn_finalize(st, 1, [1.0, 1.0], [0.0, 0.0], None, 1e-5, 0.1, [0.0, 0.0], [1.0, 1.0])
    assert np.array_equal(r['var'], [0.0, 0.0]) and np.array_equal(r['invstd'], 1 / np.sqrt([1e-5, 1e-5]))
    assert np.array_equal(r['running_var'], [0.9, 0.9]) and np.array_equal(r['running_mean'], 0.1 * np.array([3.0, 2.0]))
    r = R.ref_bn_finalize(st, 1, [1.0, 1.0], [0.0, 0.0], None, 1e-5, 0.1, None, None)
    assert r['running_mean'] is None and r['running_var'] is None and 'running_var' not in r['tol']


@pytest.mark.parametrize('with_bias', [False, True])
def test_ref_bn_fold_is_batchnorm2d_eval(with_bias):
    import torch
    C, eps = 7, 1e-3
    rng = np.random.default_rng(3)
    g, b, bias = rng.uniform(0.5, 1.5, C) * rng.choice([-1.0, 1.0], C), rng.standard_normal(C), rng.standard_normal(C)
    rm, rv = rng.standard_normal(C), rng.uniform(0.5, 2, C)
    rv[0], rv[1] = 0.0, 1e-12
    bn = torch.nn.BatchNorm2d(C, eps=eps).double().eval()
    z = rng.standard_normal((C, 50))
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(g)); bn.bias.copy_(torch.from_numpy(b))
        bn.running_mean.copy_(torch.from_numpy(rm)); bn.running_var.copy_(torch.from_numpy(rv))
        y = bn(torch.from_numpy(z).view(1, C, 50, 1) + (torch.from_numpy(bias).view(1, C, 1, 1) if with_bias else 0.0))[0, :, :, 0].numpy()
    r = R.ref_bn_fold(g, b, rm, rv, bias if with_bias else None, eps)
    mag = (np.abs(z) + np.abs(rm)[:, None] + np.abs(bias)[:, None]) * np.abs(r['scale'])[:, None] + np.abs(b)[:, None]
    _close(z * r['scale'][:, None] + r['shift'][:, None], y, mag, 'y')


def test_ref_head_is_the_oracle_head():
    """ref_head against point_conv, directionAtt, direction_conv, maskAtt, mask_conv of the oracle in float64 (model_unet_rev1.py:258-263)"""
    import torch
    from oracle import models as om
    torch.manual_seed(3)
    ref = om.Unet().double()
    N, H, W = 2, 5, 7
    f = [torch.randn((N, 64, H, W), dtype=torch.float64) for _ in range(3)]
    with torch.no_grad():
        x_point = ref.point_conv(f[2])
        x_dir = ref.direction_conv(ref.directionAtt(f[1], x_point))
        x_mask = ref.mask_conv(ref.maskAtt(f[0], x_dir))
    ps = [ref.point_conv.weight, ref.direction_conv.weight, ref.mask_conv.weight, ref.point_conv.bias, ref.direction_conv.bias,
          ref.mask_conv.bias, ref.directionAtt.Conv1x1.weight, ref.maskAtt.Conv1x1.weight]
    hw = torch.cat([p.detach().reshape(-1) for p in ps]).numpy()
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(N * H * W, -1).numpy()
    (mask, point, dirn), (S_mask, S_point, S_dir) = R.ref_head(flat(f[0]), flat(f[1]), flat(f[2]), hw)
    _close(point, flat(x_point)[:, 0], S_point, 'point')
    _close(dirn, flat(x_dir), S_dir, 'direction')
    _close(mask, flat(x_mask), S_mask, 'mask')
    assert np.all(S_point >= np.abs(point)) and np.all(S_dir >= np.abs(dirn)) and np.all(S_mask >= np.abs(mask))


def test_ref_conv1x1_is_conv2d():
    import torch
    rng = np.random.default_rng(5)
    F, w, b = rng.standard_normal((11, 64)), rng.standard_normal((5, 64)), rng.standard_normal(5)
    want = torch.nn.functional.conv2d(torch.from_numpy(F.T.copy()).view(1, 64, 11, 1), torch.from_numpy(w).view(5, 64, 1, 1), torch.from_numpy(b))
    got, S = R.ref_conv1x1(F, w, b)
    _close(got, want[0, :, :, 0].numpy().T, S, 'logits')


def test_ref_transform_and_ulps():
    x = np.array([-1.5, 0.25, 2.0])
    assert np.array_equal(R.ref_transform(x, [2.0, -4.0, 1.0], [0.5, 1.0, 0.0], [1.0, 0.0, -3.0], True), [0.0, 0.0, 0.0])
    assert np.array_equal(R.ref_transform(x, None, None, [1.0, 0.0, -3.0], False), [-0.5, 0.25, -1.0])
    assert np.array_equal(R.ulp_bf16([1.0, 1.99, 2.0, -0.75, 0.0]), [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** -133])
    assert np.array_equal(R.ulp32([1.0, -3.0]), [2.0 ** -23, 2.0 ** -22])
    assert R.sample_ranges(262600, 262144) == [(0, 4096), (258048, 262600)]
    assert R.sample_ranges(1049600, 1048576) == [(0, 4096), (1044480, 1049600)]
    assert R.sample_ranges(100, 64) == [(0, 100)]


@pytest.mark.parametrize('geo', R.STITCH_GEOMETRIES)
def test_ref_stitch_is_the_oracle_loop(geo):
    """ref_stitch over independently cut windows == oracle/infer.py's split_forward with a network that codes the global pixel (through
    its input) and the position inside the window (exact in fp32)"""
    import torch
    from cdnet_amd import utils
    from oracle import infer
    hv, wv, size, overlap = geo
    stride, th, tw, ny, nx = utils.window_grid(hv, wv, size, overlap)
    gid = (np.arange(hv * wv, dtype=np.float32) + 1).reshape(1, 1, hv, wv)
    x = torch.from_numpy(np.concatenate([gid, gid * 0 + 1, gid * 0], 1))

    def net(xb):
        b, _, h, w = xb.shape
        yy = torch.arange(h, dtype=torch.float32).view(1, 1, h, 1).expand(b, 1, h, w)
        xx = torch.arange(w, dtype=torch.float32).view(1, 1, 1, w).expand(b, 1, h, w)
        return (torch.cat([xb[:, :1], yy, xx], 1), xb[:, :1] + xb[:, 1:2] * 0.5,
                torch.cat([yy * 64 + xx + 4096 * k for k in range(9)], 1))

    want = infer.split_forward(net, x, size, overlap)
    pad = torch.zeros((1, 3, (ny - 1) * stride + th, (nx - 1) * stride + tw))
    pad[:, :, :hv, :wv] = x
    wins = torch.cat([pad[:, :, ky * stride:ky * stride + th, kx * stride:kx * stride + tw] for ky in range(ny) for kx in range(nx)], 0)
    for tiles, w in zip(net(wins), want):
        got = R.ref_stitch(tiles.numpy(), size, overlap, hv, wv)
        assert got.shape == tuple(w.shape[1:]) and np.array_equal(got, w[0].numpy())
