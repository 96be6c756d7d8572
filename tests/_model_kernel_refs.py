"""Plain float64 references, derived error bounds and case builders for the non-convolution kernels of csrc/model.hip, shared by
test_model_kernel_refs_cpu.py (which pins the references to PyTorch / the oracle on the CPU) and test_gpu_model_kernels.py.

Everything here is numpy float64 on the host.  Bounds are derived, never tuned:
  ulp32(x)        one fp32 unit in the last place of x
  U32 = 2^-24     the fp32 unit roundoff; sums of fp32 operations are bounded by 4 * U32 * (sum of |terms|)
  HEAD_EPS = 2^-16  per-logit bound of the heads relative to S, the logit expression over absolute values (64 fp32 fused multiply-adds
                  give 2^-18 * S; the factor 4 covers the quad-sum order and expf)."""
import numpy as np

U32 = 2.0 ** -24
HEAD_EPS = 2.0 ** -16
SENTINEL = -12345.678          # (any value no kernel output takes)


def f64(a):
    return np.asarray(a, dtype=np.float64)


def ulp32(x):
    """one fp32 unit in the last place at |x| (float64 array)"""
    return np.spacing(np.abs(f64(x)).astype(np.float32)).astype(np.float64)


def ulp_bf16(x):
    """one bf16 unit in the last place at |x|: 8 significant bits, the exponent range of fp32"""
    ax = np.abs(f64(x))
    _, e = np.frexp(ax)                              # |x| = m * 2^e, m in [0.5, 1)
    return np.ldexp(1.0, np.maximum(np.where(ax == 0, -125, e), -125) - 8)


def terms_tol(*terms):
    """4 * 2^-24 * (sum of the absolute values of the terms of the defining expression)"""
    return 4.0 * U32 * sum(np.abs(f64(t)) for t in terms)


# ----------------------------------------------------------------------------------------------------------------------------------
# BatchNorm bookkeeping
# ----------------------------------------------------------------------------------------------------------------------------------
def ref_bn_finalize(stats, count, g, b, bias, eps, mom, rm, rv):
    """nn.BatchNorm2d in train() from per-tile statistics.  stats [T][2][C] = (sum, sum of squares) of the bias-free convolution output
    over `count` elements per channel; bias (or None) is the convolution bias that the BatchNorm's input carries on top.  rm / rv = the
    running statistics before the step, or None.  Returns a dict of float64 arrays: mean, var (biased, clamped at 0), invstd, scale,
    shift, running_mean, running_var (None without rm / rv) and tol, the bound of every output."""
    stats, g, b = f64(stats), f64(g), f64(b)
    count, eps, mom = float(count), float(eps), float(mom)
    s, q = stats[:, 0, :].sum(0), stats[:, 1, :].sum(0)
    mean = s / count
    var = np.maximum(q / count - mean * mean, 0.0)
    invstd = 1.0 / np.sqrt(var + eps)
    scale = g * invstd
    shift = b - mean * scale
    r = dict(mean=mean, var=var, invstd=invstd, scale=scale, shift=shift, running_mean=None, running_var=None)
    tol = dict(mean=ulp32(mean), invstd=ulp32(invstd), scale=2 * ulp32(scale), shift=terms_tol(b, mean * scale))
    if rm is not None:
        rm, rv = f64(rm), f64(rv)
        bz = np.zeros_like(mean) if bias is None else f64(bias)
        unb = var * (count / (count - 1.0 if count > 1.0 else 1.0))
        r['running_mean'] = (1.0 - mom) * rm + mom * (mean + bz)
        r['running_var'] = (1.0 - mom) * rv + mom * unb
        tol['running_mean'] = terms_tol((1.0 - mom) * rm, mom * mean, mom * bz)
        tol['running_var'] = terms_tol((1.0 - mom) * rv, mom * unb)
    r['tol'] = tol
    return r


def ref_bn_fold(g, b, rm, rv, bias, eps):
    """nn.BatchNorm2d in eval() over z + bias as y = z * scale + shift.  Returns scale, shift and their bounds."""
    g, b, rm, rv = f64(g), f64(b), f64(rm), f64(rv)
    bz = np.zeros_like(g) if bias is None else f64(bias)
    scale = g / np.sqrt(rv + float(eps))
    shift = b + (bz - rm) * scale
    return dict(scale=scale, shift=shift, tol=dict(scale=2 * ulp32(scale), shift=terms_tol(b, bz * scale, rm * scale)))


BN_REGIMES = ('well', 'offset', 'const', 'negvar', 'neggamma')


def tile_counts(T, count):
    """`count` pixels over T tiles, the first tiles one larger (tiles may be empty: count < T)"""
    n = np.full(T, count // T, dtype=np.int64)
    n[:count % T] += 1
    return n


def bn_stats_case(T, C, count, seed, regime_offset=0):
    """fp32 statistics [T][2][C] of data whose channels cycle through BN_REGIMES (mixed within one call), with gamma, beta, bias, running
    statistics.  The statistics are the kernel's input: the reference reads these same fp32 numbers."""
    rng = np.random.default_rng(seed)
    n = tile_counts(T, count)
    edges = np.concatenate([[0], np.cumsum(n)])
    stats = np.zeros((T, 2, C), np.float32)
    regimes = []
    for c in range(C):
        reg = BN_REGIMES[(c + regime_offset) % len(BN_REGIMES)]
        regimes.append(reg)
        if reg in ('well', 'neggamma'):
            x = rng.uniform(0.3, 2.0) * rng.choice([-1.0, 1.0]) + rng.standard_normal(count)
        elif reg == 'offset':
            x = 100.0 + 0.01 * rng.standard_normal(count)
        else:
            x = np.full(count, 1.5 if reg == 'const' else 3.0)
        cs, cq = np.concatenate([[0.0], np.cumsum(x)]), np.concatenate([[0.0], np.cumsum(x * x)])
        if reg in ('const', 'negvar'):                   # exact tile sums: q / count == mean^2
            s, q = x[0] * n, x[0] * x[0] * n
        else:
            s, q = cs[edges[1:]] - cs[edges[:-1]], cq[edges[1:]] - cq[edges[:-1]]
        stats[:, 0, c], stats[:, 1, c] = s, q
        if reg == 'negvar':                              # one fp32 ulp off the first tile's sum of squares: q / count - mean^2 < 0
            stats[0, 1, c] = np.nextafter(stats[0, 1, c], np.float32(0))
    g = rng.uniform(0.5, 1.5, C)
    g[[i for i, r in enumerate(regimes) if r == 'neggamma']] *= -1.0
    f32 = lambda a: np.asarray(a, np.float32)
    return dict(stats=stats, regimes=regimes, g=f32(g), b=f32(0.2 * rng.standard_normal(C)), bias=f32(0.5 * rng.standard_normal(C)),
                rm=f32(rng.standard_normal(C)), rv=f32(rng.uniform(0.5, 2.0, C)))


def bn_grid_case(C, count, seed):
    """x [C][count] on a 2^-6 grid with |x| < 8, cut into uneven tiles of at most 64 pixels: every fp32 tile sum and sum of squares is
    exact (sum < 2^9 on a 2^-6 grid, squares < 2^12 on a 2^-12 grid: 15 and 24 bits).  Returns x (float64) and stats fp32 [T][2][C]."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-8 * 64 + 1, 8 * 64, size=(C, count)).astype(np.float64) / 64.0
    sizes, left, k = [], count, 0
    while left > 0:
        sizes.append(min(left, (1, 2, 37, 5, 64, 23)[k % 6]))
        left -= sizes[-1]
        k += 1
    edges = np.concatenate([[0], np.cumsum(sizes)])
    stats = np.zeros((len(sizes), 2, C), np.float32)
    for t in range(len(sizes)):
        seg = x[:, edges[t]:edges[t + 1]]
        s, q = seg.sum(1), (seg * seg).sum(1)
        stats[t, 0], stats[t, 1] = s, q
        assert np.array_equal(stats[t, 0].astype(np.float64), s) and np.array_equal(stats[t, 1].astype(np.float64), q), 'tile sums must be exact'
    return x, stats


# ----------------------------------------------------------------------------------------------------------------------------------
# Lazily transformed features and the heads
# ----------------------------------------------------------------------------------------------------------------------------------
def ref_transform(raw, scale=None, shift=None, res=None, relu=False):
    """F = [relu](raw * scale + shift + res) in float64; raw / res [..., C], scale / shift [C]"""
    x = f64(raw)
    if scale is not None:
        x = x * f64(scale) + f64(shift)
    if res is not None:
        x = x + f64(res)
    return np.maximum(x, 0.0) if relu else x


def split_head_weights(hw):
    """the CDNET_HEAD_WEIGHT_FLOATS block: point_conv.w[64], direction_conv.w[9][64], mask_conv.w[3][64], point_conv.b,
    direction_conv.b[9], mask_conv.b[3], directionAtt.w, maskAtt.w[9]"""
    hw = f64(hw).reshape(-1)
    assert hw.size == 855
    o = np.cumsum([0, 64, 576, 192, 1, 9, 3, 1, 9])
    p = [hw[o[i]:o[i + 1]] for i in range(8)]
    return dict(wp=p[0], wd=p[1].reshape(9, 64), wm=p[2].reshape(3, 64), bp=p[3][0], bd=p[4], bm=p[5], a1=p[6][0], a2=p[7])


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def ref_head(F1, F2, F3, head_weights):
    """model_unet_rev1.py:258-263 per pixel in float64.  F_k [P][64].  Returns (mask [P][3], point [P], direction [P][9]) and
    (S_mask, S_point, S_direction): the same expressions with every weight, bias and feature value replaced by its absolute value and
    every gate 1 + sigmoid(.) in [1, 2] by 2."""
    w = split_head_weights(head_weights)
    F1, F2, F3 = f64(F1), f64(F2), f64(F3)
    point = F3 @ w['wp'] + w['bp']
    g1 = 1.0 + _sigmoid(w['a1'] * point)
    dirn = g1[:, None] * (F2 @ w['wd'].T) + w['bd']
    g2 = 1.0 + _sigmoid(dirn @ w['a2'])
    mask = g2[:, None] * (F1 @ w['wm'].T) + w['bm']
    S_point = np.abs(F3) @ np.abs(w['wp']) + abs(w['bp'])
    S_dir = 2.0 * (np.abs(F2) @ np.abs(w['wd']).T) + np.abs(w['bd'])
    S_mask = 2.0 * (np.abs(F1) @ np.abs(w['wm']).T) + np.abs(w['bm'])
    return (mask, point, dirn), (S_mask, S_point, S_dir)


def ref_conv1x1(F, w, b):
    """F [P][64], w [K][64], b [K] -> logits [P][K] and S, the expression over absolute values"""
    F, w, b = f64(F), f64(w), f64(b)
    return F @ w.T + b, np.abs(F) @ np.abs(w).T + np.abs(b)


def sample_ranges(total, split, width=4096):
    """pixel ranges of a large case: the first `width`, the last `width`, and 2 * width around `split` (where a grid-stride loop starts its
    second iteration), clipped and merged"""
    rs = [(0, min(width, total)), (max(total - width, 0), total), (max(split - width, 0), min(split + width, total))]
    rs.sort()
    out = [rs[0]]
    for a, b in rs[1:]:
        if a <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], b))
        else:
            out.append((a, b))
    return out


# ----------------------------------------------------------------------------------------------------------------------------------
# Sliding windows
# ----------------------------------------------------------------------------------------------------------------------------------
def ref_stitch(tiles, size, overlap, hv, wv):
    """utils.py:683-726: tiles [ny*nx][K][th][tw] (window outputs in row-major window order) -> [K][hv][wv].  Each window writes its
    interior - overlap // 2 trimmed except at the border of the padded view - in loop order, later windows over earlier ones."""
    stride = size - overlap
    h = hv + (stride - (hv - size) % stride if hv - size > 0 else 0)
    w = wv + (stride - (wv - size) % stride if wv - size > 0 else 0)
    ys, xs = list(range(0, h - overlap, stride)), list(range(0, w - overlap, stride))
    K = tiles.shape[1]
    out = np.zeros((K, h, w), tiles.dtype)
    for ky, i in enumerate(ys):
        r0 = i + overlap // 2 if i > 0 else 0
        r1 = i + size - overlap // 2 if i + size < h else h
        for kx, j in enumerate(xs):
            c0 = j + overlap // 2 if j > 0 else 0
            c1 = j + size - overlap // 2 if j + size < w else w
            out[:, r0:r1, c0:c1] = tiles[ky * len(xs) + kx][:, r0 - i:r1 - i, c0 - j:c1 - j]
    return out[:, :hv, :wv]


STITCH_GEOMETRIES = [(37, 53, 24, 8), (96, 96, 64, 16), (50, 41, 24, 7), (20, 70, 24, 8), (64, 64, 64, 16)]
