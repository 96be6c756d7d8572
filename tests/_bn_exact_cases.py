"""Rows, lattices, the float64 reference and the guard of the exact per-element tests of csrc/bn_bwd.hip, shared by
test_bn_refs_cpu.py (which pins the reference to CPU autograd, runs the guard for every row and checks the plan decoder) and
test_gpu_bn_bwd_exact.py.

Reference (numpy float64, no autograd; `reference`).  For pixel (n, y, x) and channel c:
  v    = raw * scale + shift (NULL scale / shift: identity); relu = 2: a = res, the stored output; else v += res when there is one and
         a = max(v, 0) with relu, else v; 16-bit formats: a = bf16(a).  (v is rounded to fp32 once after the multiply-add and once
         after the residual add, as the forward does: the mask and the arg-max are discontinuous in it.  On the lattices both are exact.)
  g    = sum over the sources: G[n, y + oy, x + ox, coff + c] inside Hg x Wg, else 0; a pooled source gives G[n, y >> 1, x >> 1, coff + c]
         when that lies inside Hg x Wg and (y, x) is the first maximum in raster order of `a` over the existing pixels of its 2 x 2 window
  dz   = 0 if relu and not a > 0, else g;   xhat = (raw - mean) * invstd, or 0 without BatchNorm
  dbeta = sum dz, dgamma = sum dz * xhat over the M = N H W pixels;  k1 = gamma * invstd, k2 = dbeta / M, k3 = dgamma / M
  dRaw = k1 * (dz - k2 - xhat * k3); without BatchNorm dRaw = dz;  dz_out = dz in the activation type.
  16-bit flat path with a residual: the sums pass stores dz as bf16 and the apply pass reads that, so dRaw is computed from bf16(dz)
  while the sums use the unrounded dz.

Lattices.  mean, invstd, scale and shift are arguments of the call, never recomputed by the kernels, so the rows choose them freely.
  L0  raw, res multiples of 1/4 in [-4, 4] (pooled rows: in [-1, 1], so that maxima tie), scale in {+-1/2, +-1, +-2}, shift and mean
      multiples of 1/4, invstd in {1/2, 1, 2}, gamma a signed power of two, gradients integers in [-3, 3].  v and a are multiples of 1/8
      below 16 (7 bits: exact in bf16), xhat a multiple of 1/8, dz an integer with |dz| <= 9: every partial sum of dz and of dz * xhat is
      an integer multiple of 1/8 below 2^24 / 8 (the guard proves it on the row's data), so exact in fp32 in any order: dbeta, dgamma and
      dz_out are compared with ==.  Pooled rows copy a value onto a neighbour inside some windows (ties are placed, not hoped for).
  L1  16-bit pooled rows: raw = 1 + k / 128, k < 16, scale 1 and shift 2 / 6 / 14: v has 9 - 11 significant bits, is exact in fp32 and not
      representable in bf16, and neighbouring values collapse when rounded: the first maximum of bf16(a) is not the first maximum of v.
      xhat is a multiple of 1/256; everything downstream stays exact as in L0.
  R   randn data as in _bn_cases.py with true batch statistics, for the inexact sums.

Bounds where equality is impossible (derived, never tuned; U32 = 2^-24):
  dRaw with BatchNorm: |got - want| <= slop = c * U32 * |k1| * (|dz| + |k2| + |xhat * k3|), c = 6: the fp32 roundings of
      `k1 * (dz - k2 - xh * k3)` as built with -ffp-contract=off - xh * k3 (1), dz - k2 (2), the second subtraction (3), the product with
      k1 (4) - and the two double -> float casts of k2 and k3 (5, 6); every one acts on an intermediate value of magnitude at most the
      sum in parentheses.  bf16 outputs add half a bf16 ulp at |want| + slop.  On L0 xhat and k1 are exact.  R rows: c = 9 (xhat's own
      subtraction and product, and the product gamma * invstd in k1), and k2, k3 carry the sums' bounds: |k1| * (tol_dbeta + |xhat|
      tol_dgamma) / M on top.
  R rows, dbeta: n_add * U32 * sum |dz|; dgamma: (n_add + 3) * U32 * sum |dz * xhat| (xhat's two roundings and the product).
      n_add = the longest chain of fp32 additions behind one partial-row entry + 1: a thread adds `trips` x 4 values (flat / generic:
      BN_U = 4 pixels per trip; window: the 4 pixels of its window), bn_write_partial adds the 256 / VPP threads of a slot, the partial
      rows are summed in double and rounded to fp32 once.  n_add = 4 * trips + 256 / VPP + 1 (`n_add`).
  R rows, dz with more than one source: ngin * U32 * sum_k |g_k| (the fp32 sum of the sources); it enters the sums' bounds as well."""
import ctypes as C
import dataclasses

import numpy as np

from _model_kernel_refs import U32, ulp_bf16

SENTINEL = -12345.678
PATH_WINDOW, PATH_FLAT, PATH_GENERIC = 1, 2, 3
PATH_NAMES = {0: 'none', 1: 'window', 2: 'flat', 3: 'generic'}
BN_U, BLOCKS_CAP, MAX_BLOCKS = 4, 512, 2048
SLACK = 64                       # elements of sentinel before and after every output tensor


# ----------------------------------------------------------------------------------------------------------------------------------
# the launch-plan record (cdnet_bn_backward_last_plan, bit layout in include/cdnet_hip.h)
# ----------------------------------------------------------------------------------------------------------------------------------
def plan_encode(path, f32, n, res, kp, apply, dz_source, nb):
    return path | int(f32) << 2 | n << 3 | int(res) << 5 | kp << 6 | int(apply) << 8 | int(dz_source) << 9 | nb << 10


def plan_decode(p):
    return dict(path=p & 3, f32=(p >> 2) & 1, n=(p >> 3) & 3, res=(p >> 5) & 1, kp=(p >> 6) & 3, apply=(p >> 8) & 1,
                dz_source=(p >> 9) & 1, nb=(p >> 10) & 0xfff)


def plan_str(p):
    d = plan_decode(p)
    return '%s%s n=%d res=%d kp=%d %s%s nb=%d' % (PATH_NAMES[d['path']], '32' if d['f32'] else '16', d['n'], d['res'], d['kp'],
                                                    'apply' if d['apply'] else 'sums', '(dz)' if d['dz_source'] else '', d['nb'])


def instantiation(p):
    """the kernel template instantiation behind a plan record (what `launch` switches on): nb dropped"""
    d = plan_decode(p)
    return (PATH_NAMES[d['path']], d['f32'], d['n'], d['res'], d['apply'])


def all_instantiations():
    """every instantiation launch<APPLY>() of bn_bwd.hip can produce: 12 window, 24 flat, 4 generic"""
    out = set()
    for f32 in (0, 1):
        for ap in (0, 1):
            out |= {('window', f32, nf, 0, ap) for nf in (0, 1, 2)}
            out |= {('flat', f32, ng, r, ap) for ng in (1, 2, 3) for r in (0, 1)}
            out.add(('generic', f32, 0, 0, ap))
    return out


def grid(count, Cc, V, unroll):
    """bn_grid of bn_bwd.hip"""
    per_block = (256 // (Cc // V)) * unroll
    return max(1, min(BLOCKS_CAP, -(-count // per_block)))


# ----------------------------------------------------------------------------------------------------------------------------------
# rows
# ----------------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Row:
    id: str
    fmt: str                     # 'f16' / 'bf16' (storage of raw and res; gradients, dRaw, dz bf16) or 'f32'
    shape: tuple                 # (N, H, W)
    C: int
    srcs: tuple                  # source kinds in argument order: same, slice, pad, pool1 (floor), pool2 (ceil), pool2s (ceil, channel slice)
    path: int                    # the path the row must reach
    res: bool = False
    relu: int = 1
    bn: bool = True
    null_shift: bool = False
    lat: str = 'L0'
    seed: int = 1

    @property
    def f32(self):
        return self.fmt == 'f32'

    @property
    def M(self):
        return self.shape[0] * self.shape[1] * self.shape[2]

    @property
    def pooled(self):
        return [k for k, s in enumerate(self.srcs) if s.startswith('pool')]

    @property
    def nwin(self):
        N, H, W = self.shape
        return N * ((H + 1) // 2) * ((W + 1) // 2)

    @property
    def window_pattern(self):
        """bn_plan's `window`: one pooled source, every other one same-size and un-shifted, BatchNorm, no residual"""
        return len(self.pooled) == 1 and all(s in ('same', 'slice') or s.startswith('pool') for s in self.srcs) and self.bn and not self.res

    @property
    def V(self):
        return 4 if self.f32 and self.path != PATH_GENERIC else 8

    @property
    def nb(self):
        return grid(self.nwin, self.C, self.V, 1) if self.window_pattern else grid(self.M, self.C, self.V, BN_U)

    @property
    def reuse(self):
        """the apply pass reads the dz the sums pass stored"""
        return self.path == PATH_FLAT and self.res and self.bn

    def plans(self, reuse=True):
        """(sums plan or None without BatchNorm, apply plan); reuse = False: a process with CDNET_BN_DZ_REUSE=0"""
        kp = self.pooled[0] if self.path == PATH_WINDOW else 0
        n = {PATH_WINDOW: len(self.srcs) - 1, PATH_FLAT: len(self.srcs), PATH_GENERIC: 0}[self.path]
        res = self.res and self.path == PATH_FLAT
        sums = plan_encode(self.path, self.f32, n, res, kp, 0, 0, self.nb) if self.bn else None
        if self.reuse and reuse:
            return sums, plan_encode(PATH_FLAT, self.f32, 1, 0, 0, 1, 1, self.nb)
        return sums, plan_encode(self.path, self.f32, n, res, kp, 1, 0, self.nb)

    def n_add(self):
        VPP = self.C // self.V
        ppb = 256 // VPP
        trips = -(-self.nwin // (self.nb * ppb)) if self.window_pattern and self.path == PATH_WINDOW else \
            -(-self.M // (self.nb * ppb * BN_U))
        return 4 * trips + 256 // VPP + 1


A, B, K = (2, 13, 21), (2, 5, 7), (2, 33, 35)
FMTS = ('f16', 'bf16', 'f32')


def _rows():
    rows = []
    seed = [100]

    def add(id_, fmt, shape, Cc, srcs, path, **kw):
        seed[0] += 1
        kw.setdefault('seed', seed[0])
        rows.append(Row(id_, fmt, shape, Cc, tuple(srcs), path, **kw))

    # ---- shape A, C = 32: single trip ----
    flat_srcs = {1: ('same',), 2: ('same', 'slice'), 3: ('slice', 'same', 'same')}
    for fmt in FMTS:
        for ng in (1, 2, 3):
            for res in (False, True):
                add('A-flat-%s-ng%d-res%d' % (fmt, ng, res), fmt, A, 32, flat_srcs[ng], PATH_FLAT, res=res)
        add('A-flat-%s-ng1-relu0' % fmt, fmt, A, 32, flat_srcs[1], PATH_FLAT, relu=0)
        add('A-flat-%s-ng2-res1-relu0' % fmt, fmt, A, 32, flat_srcs[2], PATH_FLAT, res=True, relu=0)
        add('A-flat-%s-ng1-res1-relu2' % fmt, fmt, A, 32, flat_srcs[1], PATH_FLAT, res=True, relu=2)
        add('A-flat-%s-ng3-res1-relu2' % fmt, fmt, A, 32, flat_srcs[3], PATH_FLAT, res=True, relu=2)
    k = 0
    for fmt in FMTS:
        for mode in ('pool1', 'pool2'):
            for nf in (0, 1, 2):
                for kp in range(nf + 1):
                    srcs = ['slice', 'same'][:nf]
                    srcs.insert(kp, mode)
                    lats = ('L0', 'L1') if fmt != 'f32' and k % 3 == 0 else ('L0',)
                    k += 1
                    for lat in lats:
                        add('A-window-%s-%s-nf%d-kp%d-%s' % (fmt, mode, nf, kp, lat), fmt, A, 32, srcs, PATH_WINDOW, lat=lat)
    for fmt in ('f16', 'f32'):
        add('A-generic-%s-pad' % fmt, fmt, A, 32, ('pad',), PATH_GENERIC)
        add('A-generic-%s-pad+same-res' % fmt, fmt, A, 32, ('pad', 'same'), PATH_GENERIC, res=True)
        add('A-generic-%s-nobn' % fmt, fmt, A, 32, ('same', 'slice'), PATH_GENERIC, bn=False)
        add('A-generic-%s-nobn-res' % fmt, fmt, A, 32, ('same',), PATH_GENERIC, bn=False, res=True)
    for fmt in ('bf16', 'f32'):
        add('A-generic-%s-pool1+res' % fmt, fmt, A, 32, ('pool1',), PATH_GENERIC, res=True)
        add('A-generic-%s-pool2s+same+res' % fmt, fmt, A, 32, ('pool2s', 'same'), PATH_GENERIC, res=True)
        add('A-generic-%s-two-pools' % fmt, fmt, A, 32, ('pool2', 'pool1'), PATH_GENERIC)
    add('A-generic-bf16-two-pools-L1', 'bf16', A, 32, ('pool1', 'pool2'), PATH_GENERIC, lat='L1')
    add('A-generic-f16-pool2+pad-L1', 'f16', A, 32, ('pool2', 'pad'), PATH_GENERIC, lat='L1')
    add('A-generic-f32-window-null-shift', 'f32', A, 32, ('pool2', 'same'), PATH_GENERIC, null_shift=True)
    add('A-window-f16-null-shift', 'f16', A, 32, ('same', 'pool2'), PATH_WINDOW, null_shift=True)
    # ---- shape B: one thread per pixel (C = 8); 3 (16-bit) / 6 (fp32) threads per pixel, which do not divide 256 (C = 24) ----
    for Cc in (8, 24):
        for fmt in ('bf16', 'f32'):
            add('B-flat-%s-c%d' % (fmt, Cc), fmt, B, Cc, ('same', 'same'), PATH_FLAT, res=True)
            add('B-window-%s-c%d' % (fmt, Cc), fmt, B, Cc, ('pool2', 'same'), PATH_WINDOW)
            add('B-generic-%s-c%d' % (fmt, Cc), fmt, B, Cc, ('pad', 'pool1'), PATH_GENERIC)
    add('B-window-f16-c24-L1', 'f16', B, 24, ('pool2',), PATH_WINDOW, lat='L1')
    # ---- C = 48 ----
    add('C48-window-f16', 'f16', A, 48, ('slice', 'pool1'), PATH_WINDOW)
    add('C48-window-f32', 'f32', A, 48, ('pool2', 'same'), PATH_WINDOW)
    add('C48-flat-f16', 'f16', A, 48, ('same',), PATH_FLAT)
    # ---- C = 1032, fp32: beyond the 4-channel kernels, everything on the generic path ----
    add('W-flat-generic', 'f32', B, 1032, ('same', 'slice'), PATH_GENERIC)
    add('W-flat-generic-relu2', 'f32', B, 1032, ('same',), PATH_GENERIC, res=True, relu=2)
    add('W-window-generic', 'f32', B, 1032, ('same', 'pool2'), PATH_GENERIC)
    # ---- shape K: 2310 pixels / 612 ceil windows at 4 pixels / 1 window per block: the capped grid, a ragged last trip ----
    add('K-flat-f16', 'f16', K, 2048, ('same',), PATH_FLAT)
    add('K-flat-bf16-ng2-res', 'bf16', K, 2048, ('same', 'same'), PATH_FLAT, res=True)
    add('K-window-f16', 'f16', K, 2048, ('pool2', 'same'), PATH_WINDOW)
    add('K-generic-bf16', 'bf16', K, 2048, ('pad',), PATH_GENERIC)
    add('K-flat-f32', 'f32', K, 1024, ('same',), PATH_FLAT)
    add('K-flat-f32-ng2-res', 'f32', K, 1024, ('same', 'same'), PATH_FLAT, res=True)
    add('K-window-f32', 'f32', K, 1024, ('same', 'pool2'), PATH_WINDOW)
    # ---- one pixel, one window ----
    for fmt in ('f16', 'f32'):
        add('P1-flat-%s' % fmt, fmt, (1, 1, 1), 8, ('same',), PATH_FLAT)
        add('P1-window-%s-ceil' % fmt, fmt, (1, 1, 1), 8, ('pool2',), PATH_WINDOW)
        add('P2-window-%s-floor' % fmt, fmt, (1, 2, 2), 8, ('pool1',), PATH_WINDOW, seed=6)     # (a seed whose 8 pairs hold both kinds of tie)
    # ---- random data ----
    add('R-K-flat-f16', 'f16', K, 2048, ('same',), PATH_FLAT, lat='R')
    add('R-K-window-f32', 'f32', K, 1024, ('pool2', 'same'), PATH_WINDOW, lat='R')
    add('R-A-generic-bf16', 'bf16', A, 32, ('pad', 'pool1'), PATH_GENERIC, lat='R')
    return rows


ROWS = _rows()
ROW_BY_ID = {r.id: r for r in ROWS}
assert len(ROW_BY_ID) == len(ROWS)


# ----------------------------------------------------------------------------------------------------------------------------------
# number formats
# ----------------------------------------------------------------------------------------------------------------------------------
def bf16(x):
    """round-to-nearest-even to bf16 of values that fp32 holds (float64 in, float64 out)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32).astype(np.float64)


def to_fmt(x, fmt):
    x = np.asarray(x, np.float64)
    if fmt == 'f16':
        return x.astype(np.float16).astype(np.float64)
    if fmt == 'bf16':
        return bf16(x.astype(np.float32))
    return x.astype(np.float32).astype(np.float64)


def representable(x, fmt):
    x = np.asarray(x, np.float64)
    return bool(np.array_equal(to_fmt(x, fmt), x))


def act_fmt(row):
    return 'f32' if row.f32 else 'bf16'


# ----------------------------------------------------------------------------------------------------------------------------------
# data
# ----------------------------------------------------------------------------------------------------------------------------------
def src_geometry(kind, H, W, Cc):
    """dict(Hg, Wg, oy, ox, pooled, coff, cstride) of a source kind"""
    g = dict(Hg=H, Wg=W, oy=0, ox=0, pooled=0, coff=0, cstride=Cc)
    if kind == 'slice':
        g.update(coff=16, cstride=Cc + 16)
    elif kind == 'pad':
        g.update(Hg=H + 1, Wg=W + 3, oy=1, ox=2, coff=8, cstride=Cc + 16)
    elif kind == 'pool1':
        g.update(Hg=H // 2, Wg=W // 2, pooled=1)
    elif kind == 'pool2':
        g.update(Hg=(H + 1) // 2, Wg=(W + 1) // 2, pooled=2)
    elif kind == 'pool2s':
        g.update(Hg=(H + 1) // 2, Wg=(W + 1) // 2, pooled=2, coff=8, cstride=Cc + 8)
    else:
        assert kind == 'same', kind
    return g


def read_mask(g, N, H, W, Cc):
    """[N][Hg][Wg][cstride] bool: the elements of a source a correct kernel may read"""
    m = np.zeros((N, g['Hg'], g['Wg'], g['cstride']), bool)
    cs = slice(g['coff'], g['coff'] + Cc)
    if g['pooled']:
        m[:, :, :, cs] = True
    else:
        m[:, g['oy']:g['oy'] + H, g['ox']:g['ox'] + W, cs] = True
    return m


def _plant_ties(rng, arrs, N, H, W, Cc, p=0.35):
    """inside a fraction p of the (window, channel) pairs, copy one existing pixel's value onto another one of the window"""
    Hp, Wp = (H + 1) // 2, (W + 1) // 2
    hit = rng.random((N, Hp, Wp, Cc)) < p
    qi = rng.integers(0, 4, (N, Hp, Wp, Cc))
    qj = (qi + rng.integers(1, 4, (N, Hp, Wp, Cc))) % 4
    n_, py, px, c_ = np.nonzero(hit)
    qi, qj = qi[hit], qj[hit]
    yi, xi, yj, xj = 2 * py + (qi >> 1), 2 * px + (qi & 1), 2 * py + (qj >> 1), 2 * px + (qj & 1)
    ok = (yi < H) & (xi < W) & (yj < H) & (xj < W)
    for a in arrs:
        if a is not None:
            a[n_[ok], yj[ok], xj[ok], c_[ok]] = a[n_[ok], yi[ok], xi[ok], c_[ok]]


def make_data(row):
    """the row's inputs as float64 arrays holding values the row's formats represent: raw, res, scale, shift, mean, invstd, gamma
    (None where the call passes NULL) and srcs: list of dict(G = [N][Hg][Wg][cstride] with NaN wherever a correct kernel does not read,
    + the geometry)"""
    rng = np.random.default_rng(row.seed)
    (N, H, W), Cc = row.shape, row.C
    af = act_fmt(row)
    d = dict(res=None, scale=None, shift=None, mean=None, invstd=None, gamma=None)
    shp = (N, H, W, Cc)
    if row.lat == 'L0':
        amp = 4 if row.pooled else 16                                   # quarters: |raw| <= 1 on pooled rows, <= 4 elsewhere
        d['raw'] = rng.integers(-amp, amp + 1, shp) / 4.0
        if row.res:
            r = rng.integers(-amp, amp + 1, shp) / 4.0
            d['res'] = np.maximum(r, 0.0) if row.relu == 2 else r
        if row.pooled:
            _plant_ties(rng, [d['raw'], d['res']], N, H, W, Cc)
        if row.bn:
            d['scale'] = rng.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], Cc, p=[0.1, 0.1, 0.1, 0.2, 0.3, 0.2])
            d['shift'] = None if row.null_shift else rng.integers(-4, 5, Cc) / 4.0
            d['mean'] = rng.integers(-4, 5, Cc) / 4.0
            d['invstd'] = rng.choice([0.5, 1.0, 2.0], Cc)
            d['gamma'] = rng.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], Cc)
        grad = lambda s: rng.integers(-3, 4, s).astype(np.float64)
    elif row.lat == 'L1':
        assert not row.f32 and row.pooled and row.bn and not row.res
        d['raw'] = 1.0 + rng.integers(0, 16, shp) / 128.0
        d['scale'] = np.where(np.arange(Cc) % 8 == 3, -1.0, 1.0)            # (a negative channel: everything behind the ReLU)
        d['shift'] = np.where(d['scale'] > 0, rng.choice([2.0, 6.0, 14.0], Cc), 0.0)
        d['mean'] = rng.integers(0, 9, Cc) / 4.0
        d['invstd'] = rng.choice([0.5, 1.0, 2.0], Cc)
        d['gamma'] = rng.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], Cc)
        grad = lambda s: rng.integers(-3, 4, s).astype(np.float64)
    else:
        assert row.lat == 'R' and row.bn and not row.res
        d['raw'] = to_fmt(rng.standard_normal(shp), row.fmt)
        x = d['raw'].reshape(-1, Cc)
        d['mean'] = to_fmt(x.mean(0), 'f32')
        d['invstd'] = to_fmt(1.0 / np.sqrt(x.var(0) + 1e-5), 'f32')
        d['gamma'] = to_fmt((rng.random(Cc) + 0.5) * np.where(np.arange(Cc) % 4 == 0, -1.0, 1.0), 'f32')
        d['scale'] = to_fmt(d['gamma'] * d['invstd'], 'f32')
        d['shift'] = to_fmt(0.2 * rng.standard_normal(Cc) - d['mean'] * d['scale'], 'f32')
        grad = lambda s: to_fmt(rng.standard_normal(s), af)
    d['srcs'] = []
    for kind in row.srcs:
        g = src_geometry(kind, H, W, Cc)
        G = grad((N, g['Hg'], g['Wg'], g['cstride']))
        G[~read_mask(g, N, H, W, Cc)] = np.nan
        d['srcs'].append(dict(g, G=G, kind=kind))
    return d


# ----------------------------------------------------------------------------------------------------------------------------------
# the float64 reference
# ----------------------------------------------------------------------------------------------------------------------------------
def _windows(a, H, W):
    """[N][H][W][C] -> [N][Hp][Wp][4][C] in raster order of the window (q = 2 dy + dx); pixels that do not exist hold -inf"""
    N, Cc = a.shape[0], a.shape[3]
    Hp, Wp = (H + 1) // 2, (W + 1) // 2
    p = np.full((N, 2 * Hp, 2 * Wp, Cc), -np.inf)
    p[:, :H, :W] = a
    return p.reshape(N, Hp, 2, Wp, 2, Cc).transpose(0, 1, 3, 2, 4, 5).reshape(N, Hp, Wp, 4, Cc)


def _unwindows(w, H, W):
    N, Hp, Wp, _, Cc = w.shape
    return w.reshape(N, Hp, Wp, 2, 2, Cc).transpose(0, 1, 3, 2, 4, 5).reshape(N, 2 * Hp, 2 * Wp, Cc)[:, :H, :W]


def first_max(a, H, W):
    """[N][H][W][C] bool: the pixel is the first maximum in raster order among the existing pixels of its 2 x 2 window"""
    w = _windows(a, H, W)
    sel = np.arange(4)[None, None, None, :, None] == np.argmax(w, axis=3)[:, :, :, None, :]          # (argmax: the first occurrence)
    return _unwindows(sel, H, W)


def activation(shape, d, relu, f32):
    """(a as the consumers saw it, a before the bf16 rounding)"""
    raw = d['raw']
    v = raw
    if d['scale'] is not None:
        sh = d['shift'] if d['shift'] is not None else 0.0
        v = (raw * d['scale'] + sh).astype(np.float32).astype(np.float64)            # (the product is exact in float64: one rounding)
    if relu == 2:
        pre = d['res']
    else:
        if d['res'] is not None:
            v = (v + d['res']).astype(np.float32).astype(np.float64)
        pre = np.maximum(v, 0.0) if relu else v
    return (pre if f32 else bf16(pre)), pre


def reference(row, d, relu=None, reuse=True):
    (N, H, W), Cc = row.shape, row.C
    relu = row.relu if relu is None else relu
    a, pre = activation(row.shape, d, relu, row.f32)
    g = np.zeros((N, H, W, Cc))
    gabs = np.zeros((N, H, W, Cc))
    sel = first_max(a, H, W) if row.pooled else None
    for s in d['srcs']:
        G = s['G'][..., s['coff']:s['coff'] + Cc]
        t = np.zeros((N, H, W, Cc))
        if s['pooled']:
            hh, ww = min(2 * s['Hg'], H), min(2 * s['Wg'], W)              # pixels whose window has a pooled gradient
            up = np.repeat(np.repeat(G, 2, axis=1), 2, axis=2)[:, :hh, :ww]
            t[:, :hh, :ww] = np.where(sel[:, :hh, :ww], up, 0.0)
        else:
            y0, y1 = max(0, -s['oy']), min(H, s['Hg'] - s['oy'])
            x0, x1 = max(0, -s['ox']), min(W, s['Wg'] - s['ox'])
            t[:, y0:y1, x0:x1] = G[:, y0 + s['oy']:y1 + s['oy'], x0 + s['ox']:x1 + s['ox']]
        g += t
        gabs += np.abs(t)
    dz = np.where(~(a > 0), 0.0, g) if relu else g
    bn = d['mean'] is not None
    xhat = (d['raw'] - d['mean']) * d['invstd'] if bn else np.zeros_like(g)
    r = dict(a=a, pre=pre, sel=sel, dz=dz, gabs=gabs, xhat=xhat, dz_out=to_fmt(dz, act_fmt(row)))
    if not bn:
        r.update(draw=dz, slop=np.zeros_like(dz))
        return r
    M = float(row.M)
    r['dbeta'], r['dgamma'] = dz.sum((0, 1, 2)), (dz * xhat).sum((0, 1, 2))
    r['k1'], r['k2'], r['k3'] = d['gamma'] * d['invstd'], r['dbeta'] / M, r['dgamma'] / M
    dza = bf16(dz) if (row.reuse and reuse and not row.f32) else dz
    r['draw'] = r['k1'] * (dza - r['k2'] - xhat * r['k3'])
    mag = np.abs(r['k1']) * (np.abs(dza) + np.abs(r['k2']) + np.abs(xhat * r['k3']))
    if row.lat == 'R':
        ngin = len(d['srcs'])
        dz_tol = ngin * U32 * gabs if ngin > 1 else np.zeros_like(dz)
        n_add = row.n_add()
        r['tol_dbeta'] = n_add * U32 * np.abs(dz).sum((0, 1, 2)) + dz_tol.sum((0, 1, 2))
        r['tol_dgamma'] = (n_add + 3) * U32 * np.abs(dz * xhat).sum((0, 1, 2)) + (dz_tol * np.abs(xhat)).sum((0, 1, 2))
        r['dz_tol'] = dz_tol
        r['slop'] = 9 * U32 * mag + np.abs(r['k1']) * (dz_tol + (r['tol_dbeta'] + np.abs(xhat) * r['tol_dgamma']) / M)
    else:
        r['slop'] = 6 * U32 * mag
    return r


def draw_bound(row, ref):
    """per-element bound of dRaw (see the module docstring)"""
    s = ref['slop']
    return s if row.f32 else s + 0.5 * ulp_bf16(np.abs(ref['draw']) + s)


def round_quot(s, M):
    """k2 / k3 as the finalize kernel must give them: the fp32 rounding of the float64 quotient"""
    return np.float32(np.float64(s) / np.float64(M))


# ----------------------------------------------------------------------------------------------------------------------------------
# the guard: CPU only, from the reference alone
# ----------------------------------------------------------------------------------------------------------------------------------
def _quantum(x):
    """the largest power of two of which every element is a multiple"""
    x = np.asarray(x, np.float64)
    nz = x[x != 0]
    if nz.size == 0:
        return 1.0
    m, e = np.frexp(nz)
    mant = (np.abs(m) * 2.0 ** 53).astype(np.uint64)
    tz = np.zeros(mant.shape, np.int64)
    for sh in (32, 16, 8, 4, 2, 1):
        z = (mant & np.uint64((1 << sh) - 1)) == 0
        tz += np.where(z, sh, 0)
        mant = np.where(z, mant >> np.uint64(sh), mant)
    return float(2.0 ** int((e - 53 + tz).min()))


def pool_counts(row, ref):
    """counts over (window, channel) pairs of a pooled row"""
    N, H, W = row.shape
    wa, wp = _windows(ref['a'], H, W), _windows(ref['pre'], H, W)
    mx = wa.max(3)
    at_max = wa == mx[:, :, :, None, :]
    tied = (mx > 0) & (at_max.sum(3) > 1)
    exist = np.isfinite(wa)
    return dict(pairs=int(mx.size), tied=int(tied.sum()), tied_at0=int((tied & at_max[:, :, :, 0, :]).sum()),
                tied_not0=int((tied & ~at_max[:, :, :, 0, :]).sum()), stick_out=int((~exist.all(3)).sum()),
                rounded_argmax=int(((np.argmax(wa, 3) != np.argmax(wp, 3)) & (mx > 0)).sum()))


def pool_needs(row):
    """what the guard demands of pool_counts: 1 % of the (window, channel) pairs and at least 4 - of the 8 pairs of a one-window shape
    at least 1; 0 where the geometry rules the event out (a one-pixel window cannot tie, even sides leave no window sticking out)"""
    N, H, W = row.shape
    pairs = row.nwin * row.C
    need = max(4, -(-pairs // 100)) if row.nwin > 1 else 1
    can_tie = H * W > 1
    n = dict(tied=need if can_tie else 0, tied_at0=need if can_tie else 0, tied_not0=need if can_tie and H * W > 2 else 0,
             stick_out=need if (H % 2 or W % 2) else 0, rounded_argmax=need if row.lat == 'L1' else 0)
    return n


def guard(row, d, ref):
    """asserts that the row is exact where it claims to be and that its data exercise what the row is there for"""
    af = act_fmt(row)
    assert representable(d['raw'], row.fmt), row.id
    if d['res'] is not None:
        assert representable(d['res'], af if row.relu == 2 else row.fmt), row.id
    for s in d['srcs']:
        G = s['G']
        m = read_mask(s, row.shape[0], row.shape[1], row.shape[2], row.C)
        assert np.isnan(G[~m]).all() and not np.isnan(G[m]).any() and representable(G[m], af), row.id
    assert np.isfinite(ref['draw']).all() and np.isfinite(ref['dz']).all(), row.id
    if row.lat != 'R':
        # every intermediate value exact: the affine and the residual add in fp32 (activation() rounds: compare with the unrounded)
        v = d['raw']
        if d['scale'] is not None:
            v = v * d['scale'] + (d['shift'] if d['shift'] is not None else 0.0)
        if row.relu != 2 and d['res'] is not None:
            v = v + d['res']
        pre = d['res'] if row.relu == 2 else (np.maximum(v, 0.0) if row.relu else v)
        assert np.array_equal(pre, ref['pre']) and representable(v, 'f32'), row.id + ': v is not exact in fp32'
        if row.lat == 'L0':
            assert representable(ref['pre'], af), row.id + ': the activation is not representable'
        assert representable(ref['xhat'], 'f32') and representable(ref['dz'], af), row.id
        assert representable(ref['dz'] * ref['xhat'], 'f32'), row.id
        q1, q2 = _quantum(ref['dz']), _quantum(ref['dz'] * ref['xhat'])
        assert np.abs(ref['dz']).sum((0, 1, 2)).max() / q1 < 2 ** 24, row.id + ': sum |dz| leaves the exact range'
        assert np.abs(ref['dz'] * ref['xhat']).sum((0, 1, 2)).max() / q2 < 2 ** 24, row.id + ': sum |dz xhat| leaves the exact range'
        if row.bn:
            assert representable(ref['k1'], 'f32') and np.abs(ref['k1']).min() >= 0.25, row.id
    # the ReLU cuts a visible share of the elements and passes a visible share
    if row.relu and row.M * row.C >= 256:
        zero = float((~(ref['a'] > 0)).mean())
        assert 0.02 < zero < 0.98, (row.id, zero)
    if row.pooled:
        cnt, need = pool_counts(row, ref), pool_needs(row)
        if row.lat != 'R':
            for k, v in need.items():
                assert cnt[k] >= v, '%s: %s = %d of %d (window, channel) pairs, needs %d' % (row.id, k, cnt[k], cnt['pairs'], v)
        return cnt
    return None


# ----------------------------------------------------------------------------------------------------------------------------------
# device side (imported lazily: the CPU tests use everything above)
# ----------------------------------------------------------------------------------------------------------------------------------
class OutBuffer:
    """a sentinel-filled tensor inside a sentinel-filled allocation with SLACK elements on both ends"""

    def __init__(self, shape, dtype):
        import torch
        n = int(np.prod(shape))
        self.full = torch.full((n + 2 * SLACK,), SENTINEL, dtype=dtype, device='cuda')
        self.t = self.full[SLACK:SLACK + n].view(*shape)
        self.sent = float(torch.full((1,), SENTINEL, dtype=dtype)[0])

    def ptr(self):
        return C.c_void_p(self.t.data_ptr())

    def read(self):
        """(the tensor as float64 numpy, the slack still holds the sentinel)"""
        f = self.full.double().cpu().numpy()
        n = f.size - 2 * SLACK
        ok = bool((f[:SLACK] == self.sent).all() and (f[SLACK + n:] == self.sent).all())
        return f[SLACK:SLACK + n].reshape(tuple(self.t.shape)), ok


def torch_dtype(fmt):
    import torch
    return {'f16': torch.float16, 'bf16': torch.bfloat16, 'f32': torch.float32}[fmt]


def to_device(x, fmt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch_dtype(fmt)).cuda().contiguous()


class DeviceCase:
    """the row's inputs on the device (kept alive here) and the filled cdnet_bn_bwd_args"""

    def __init__(self, row, d, relu=None):
        from cdnet_amd import trainer
        (N, H, W), Cc = row.shape, row.C
        af = act_fmt(row)
        relu = row.relu if relu is None else relu
        self.row, self.keep = row, []
        dev = lambda x, fmt: self.keep.append(to_device(x, fmt)) or self.keep[-1]
        a = self.A = trainer.BnBwdArgs()
        a.raw = dev(d['raw'], row.fmt).data_ptr()
        a.res = dev(d['res'], af if relu == 2 else row.fmt).data_ptr() if d['res'] is not None else None
        self.vec = {}
        for k in ('scale', 'shift', 'mean', 'invstd', 'gamma'):
            self.vec[k] = dev(d[k], 'f32') if d[k] is not None else None
            if k != 'gamma':
                setattr(a, k, self.vec[k].data_ptr() if d[k] is not None else None)
        a.ngin = len(d['srcs'])
        for k, s in enumerate(d['srcs']):
            a.gin[k].g = dev(s['G'], af).data_ptr()
            for f in ('Hg', 'Wg', 'oy', 'ox', 'pooled', 'coff', 'cstride'):
                setattr(a.gin[k], f, s[f])
        a.f16 = {'bf16': 0, 'f16': 1, 'f32': 2}[row.fmt]
        a.relu, a.N, a.H, a.W, a.C = relu, N, H, W, Cc

    def gamma_ptr(self):
        return C.c_void_p(self.vec['gamma'].data_ptr()) if self.vec['gamma'] is not None else None


def ws_floats(Cc):
    return MAX_BLOCKS * 2 * Cc + 3 * Cc


def make_buffers(row, with_dz=None):
    import torch
    (N, H, W), Cc = row.shape, row.C
    adt = torch_dtype(act_fmt(row))
    with_dz = row.res if with_dz is None else with_dz
    return dict(draw=OutBuffer((N, H, W, Cc), adt), dz=OutBuffer((N, H, W, Cc), adt) if with_dz else None,
                dgamma=OutBuffer((Cc,), torch.float32), dbeta=OutBuffer((Cc,), torch.float32),
                ws=OutBuffer((ws_floats(Cc),), torch.float32))


def buffers_untouched(b):
    for k, o in b.items():
        if o is not None:
            got, ok = o.read()
            if not ok or not (got == o.sent).all():
                return k
    return None


def run_fused(dc, b, ws_floats_arg=None, gamma=True):
    """cdnet_bn_backward on the case; returns the status code (0: launched) - the caller reads the buffers and the plan record"""
    import torch
    from cdnet_amd import _lib
    row = dc.row
    lib = _lib.load()
    bn = row.bn
    rc = lib.cdnet_bn_backward(C.byref(dc.A), dc.gamma_ptr() if gamma else None, b['dgamma'].ptr() if bn else None,
                               b['dbeta'].ptr() if bn else None, b['ws'].ptr(),
                               ws_floats(row.C) if ws_floats_arg is None else ws_floats_arg, b['draw'].ptr(),
                               b['dz'].ptr() if b['dz'] is not None else None, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


def worst(err, bound):
    """(largest err / bound, its index); a zero bound with a zero error counts 0, with a non-zero error inf"""
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(err == 0, 0.0, err / bound)
    q = np.where(np.isnan(q), np.inf, q)
    i = np.unravel_index(int(np.argmax(q)), q.shape)
    return float(q[i]), tuple(int(k) for k in i)


def describe(name, got, want, i):
    return '%s%s: got %r want %r' % (name, list(i), float(got[i]), float(want[i]))


def check_row(row, d, ref, reuse=True):
    """cdnet_bn_backward on the row: the plan of both passes, the sentinels, every element against the reference (equality, or the
    derived bound).  Returns {quantity: worst err / bound} of the quantities that carry a bound."""
    from cdnet_amd import _lib
    lib = _lib.load()
    (N, H, W), Cc = row.shape, row.C
    dc, b = DeviceCase(row, d), make_buffers(row)
    sums_before = lib.cdnet_bn_backward_last_sums_plan()
    rc = run_fused(dc, b)
    assert rc == 0, '%s: refused: %s' % (row.id, lib.cdnet_last_error().decode(errors='replace'))
    want_sums, want_apply = row.plans(reuse)
    got_apply, got_sums = lib.cdnet_bn_backward_last_plan(), lib.cdnet_bn_backward_last_sums_plan()
    assert got_apply == want_apply, '%s: the apply pass ran [%s], the row expects [%s]' % (row.id, plan_str(got_apply), plan_str(want_apply))
    if want_sums is None:
        assert got_sums == sums_before, '%s: a layer without BatchNorm ran a sums pass [%s]' % (row.id, plan_str(got_sums))
    else:
        assert got_sums == want_sums, '%s: the sums pass ran [%s], the row expects [%s]' % (row.id, plan_str(got_sums), plan_str(want_sums))
    report = {}
    exact = row.lat != 'R'

    def tensor(name, buf, want, bound):
        got, ok = buf.read()
        assert ok, '%s: wrote outside %s' % (row.id, name)
        unwritten = got == buf.sent
        assert not unwritten.any(), '%s: %d elements of %s were not written, the first at [n, y, x, c] = %s' % (
            row.id, int(unwritten.sum()), name, [int(k[0]) for k in np.nonzero(unwritten)])
        err = np.abs(got - want)
        if bound is None:
            bad = got != want
            assert not bad.any(), '%s: %d of %d elements of %s differ; ' % (row.id, int(bad.sum()), bad.size, name) + \
                describe(name, got, want, tuple(int(k[0]) for k in np.nonzero(bad)))
        else:
            q, i = worst(err, bound)
            report[name] = q
            assert q <= 1.0, '%s: err / bound = %.3g; ' % (row.id, q) + describe(name, got, want, i) + ' bound %.3g' % float(bound[i])

    af = act_fmt(row)
    if row.bn:
        tensor('draw', b['draw'], ref['draw'], draw_bound(row, ref))
    else:
        tensor('draw', b['draw'], to_fmt(ref['draw'], af), None)
    if b['dz'] is not None:
        tensor('dz_out', b['dz'], ref['dz_out'], None if exact or len(d['srcs']) == 1 else
               ref['dz_tol'] + (0 if row.f32 else 0.5 * ulp_bf16(np.abs(ref['dz']) + ref['dz_tol'])))
    ws, ok = b['ws'].read()
    assert ok, row.id + ': wrote outside the workspace'
    if not row.bn:
        for k in ('ws', 'dgamma', 'dbeta'):
            got, ok = b[k].read()
            assert ok and (got == b[k].sent).all(), '%s: a layer without BatchNorm wrote %s' % (row.id, k)
        return report
    tensor('dbeta', b['dbeta'], ref['dbeta'], None if exact else ref['tol_dbeta'])
    tensor('dgamma', b['dgamma'], ref['dgamma'], None if exact else ref['tol_dgamma'])
    nb = row.nb
    rows_, coef, rest = ws[:nb * 2 * Cc], ws[nb * 2 * Cc:nb * 2 * Cc + 3 * Cc].reshape(3, Cc), ws[nb * 2 * Cc + 3 * Cc:]
    sent = b['ws'].sent
    assert not (rows_ == sent).any(), '%s: %d entries of the %d partial rows were not written' % (row.id, int((rows_ == sent).sum()), nb)
    assert not (coef == sent).any(), row.id + ': coefficients not written'
    assert (rest == sent).all(), '%s: %d workspace floats behind row %d and the coefficients were written' % (row.id, int((rest != sent).sum()), nb)
    if exact:
        assert np.array_equal(rows_.reshape(nb, 2, Cc).sum(0), np.stack([ref['dbeta'], ref['dgamma']])), row.id + ': partial rows'
        assert np.array_equal(coef[0], ref['k1']), row.id + ': k1'
        assert np.array_equal(coef[1], round_quot(ref['dbeta'], row.M).astype(np.float64)), row.id + ': k2'
        assert np.array_equal(coef[2], round_quot(ref['dgamma'], row.M).astype(np.float64)), row.id + ': k3'
    return report
