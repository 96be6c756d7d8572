"""Case table, float64 references, data lattices and the device runner of the weight-gradient tests (csrc/wgrad.hip), shared by
test_wgrad_refs_cpu.py (pins the references to PyTorch autograd on the CPU), test_gpu_wgrad_exact.py, test_gpu_wgrad_reduce.py and
test_gpu_wgrad_bound.py.

The exact tests rest on lattices: inputs chosen so that every product a * g and every partial sum of them is a multiple of a lattice
unit and stays below 2^24 units - exactly representable in fp32.  Then the result does not depend on the summation order, on `ksplit` or
on the kernel form, and must EQUAL the float64 reference.  One dropped, doubled or misplaced term moves an element by >= one unit.
  L0  stored input integers in [-3, 3] (some -0.0), scale in {+-1, +-2, 0.5}, shift integers in [-2, 2] (some -0.0), residual and
      gradient integers in [-3, 3]: the transformed input is a multiple of 0.5, |t| <= 11, exact in fp16 and bf16.  Unit 0.5.
  L1  (fp32 tensors, plain sources) input multiples of 2^-8 in [-4, 4): at most 11 significant bits, so the bf16 split hi + lo is exact
      and lo != 0 for most values; gradient integers in [-3, 3] (lo = 0).  Unit 2^-8.  A missing lo_a * hi_g product shows.
  L2  L1 with input and gradient swapped: a missing hi_a * lo_g product shows.
`guard` asserts the regime (sum |a * g| per element, in units, below 2^24) before anything runs.

Every row names ci_tiles, its split factors and the kernel instantiation it must reach (cdnet_conv_backward_weight_last_form), per
precision: '16' = bf16 / fp16 tensors and a bf16 gradient, '32' = fp32 tensors and an fp32 gradient (the same stored values)."""
import zlib
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

SENTINEL = 12345.678           # no lattice value, no sum of them
SLACK = 96                     # floats of sentinel before and after dW in its buffer
DEFER = 0x100                  # CDNET_WGRAD_DEFER_REDUCE

# kind -> (taps, npar, ostride, reduce mode)
KINDS = {'conv3': (9, 1, 1, 0), 'conv1': (1, 1, 1, 0), 'convT4': (4, 4, 2, 2), 'convT2': (1, 4, 2, 3), 'conv3s2': (9, 1, 1, 6)}

# ---- kernel forms (bit layout of include/cdnet_hip.h) ---------------------------------------------------------------------------
GEN, WS, F32K, WS32 = 1, 2, 3, 4
PLAIN, FAST, GENERIC = 0, 1, 2


def form(family, ci_t, co_t, taps, res=0, xf=0, qm=0):
    return family | (ci_t << 4) | (co_t << 8) | (taps << 12) | (res << 16) | (xf << 17) | (qm << 19)


def ws(ci_t, co_t, taps, xf, res=0):
    return form(WS, ci_t, co_t, taps, res, xf)


def gen(ci_t, co_t, taps, res=0):
    return form(GEN, ci_t, co_t, taps, res, GENERIC)


def f32k(ci_t, co_t, taps, qm=0):
    return form(F32K, ci_t, co_t, taps, 0, 0, qm)


def ws32(taps, xf, qm):
    return form(WS32, 2, 2, taps, 0, xf, qm)


def form_str(f):
    fam = {0: 'none', GEN: 'wgrad_kernel', WS: 'wgrad_ws_kernel', F32K: 'wgrad_f32_kernel', WS32: 'wgrad_ws32_kernel'}.get(f & 15, '?')
    return '%s<CI_T %d, CO_T %d, TAPS %d, RES %d, XF %d, QM %d>' % (fam, (f >> 4) & 15, (f >> 8) & 15, (f >> 12) & 15, (f >> 16) & 1,
                                                                   (f >> 17) & 3, (f >> 19) & 7)


# ---- the table --------------------------------------------------------------------------------------------------------------------
@dataclass
class S:
    """one input source of a layer: C stored channels (creal of them real), storage type of the 16-bit run, lazy transform, stored size
    (hs, ws; None = the layer's logical size, or what the pool mode needs), F.pad offset"""
    C: int
    creal: int = None
    store: str = 'bf16'
    aff: bool = False
    relu: bool = False
    res: bool = False
    pool: int = 0
    off: tuple = (0, 0)
    hs: int = None
    ws: int = None


@dataclass
class Case:
    id: str
    kind: str
    shape: tuple               # (N, H, W): the layer's logical input size (conv3s2: its OUTPUT size; the input is 2H x 2W)
    Cout: int
    srcs: list
    ci_t: int
    ksplits: tuple
    form16: list               # expected form per source, 16-bit tensors (None: not run)
    form32: list = None        # fp32 tensors (None: the ABI refuses this row or it has no fp32 counterpart)
    lattices: tuple = ('L0',)


def PL(C, **k): return S(C, **k)
def FA(C, **k): return S(C, store='fp16', aff=True, relu=True, **k)                 # the training-mode fast path
def FR(C, **k): return S(C, store='fp16', aff=True, relu=True, res=True, **k)       # ... with a residual branch
def GA(C, **k): return S(C, aff=True, **k)                                          # generic: bf16 affine, no ReLU
def GR(C, **k): return S(C, relu=True, **k)                                         # generic: ReLU only
def GH(C, **k): return S(C, store='fp16', **k)                                      # generic: fp16 as stored
def GX(C, **k): return S(C, aff=True, res=True, **k)                                # generic with residual: wgrad_kernel's RES form


P0, P1, P2, P3, P4 = (1, 8, 16), (1, 7, 15), (1, 9, 17), (1, 5, 33), (3, 17, 33)
# 8 x 16-pixel tiles: P4 has 27 (workgroups get 27 | 13-14 | 5-6 | 3-4 | 3 | 1-2 | 1 | 0-1 | 0-1 tiles), 14 and 40 do not divide it and
# exceed one image's 9 tiles; wgrad_ws32_kernel's 4 x 16 tiles: 45 (45 | 22-23 | 9 | 6-7 | 5 | 3-4 | 1-2 | 1-2 | 0-1), one image has 15
SWEEP = (1, 2, 5, 7, 9, 14, 27, 40, 50)
K1, K4 = (1, 2), (1, 3, 5)      # one-tile shapes (1 | 0-1 tiles per workgroup), four-tile shapes (4 | 1-2 | 0-1)


def _ks(shape):
    return K1 if shape in (P0, P1) else (K4 if shape in (P2, P3) else (2, 7))


CASES = []


def _add(id, kind, shape, Cout, srcs, ci_t, f16, f32=None, ks=None, lattices=('L0',)):
    CASES.append(Case(id, kind, shape, Cout, srcs, ci_t, ks or _ks(shape), f16, f32, lattices))


# ---- CI 32 / CO 128 (ci_tiles 1): C in {32, 40}, Cout in {128, 136, 24}; at most 32 output channels: wgrad_ws_kernel<1, 1>
_add('c1-3x3-plain-sweep', 'conv3', P4, 128, [PL(32)], 1, [ws(1, 4, 9, PLAIN)], [f32k(1, 4, 9)], ks=SWEEP)
_add('c1-3x3-plain-ragged', 'conv3', P2, 136, [PL(40)], 1, [ws(1, 4, 9, PLAIN)], [f32k(1, 4, 9)], lattices=('L0', 'L1', 'L2'))
_add('c1-3x3-fast', 'conv3', P1, 128, [FA(40)], 1, [ws(1, 4, 9, FAST)], [f32k(1, 4, 9)])
_add('c1-3x3-fast-res', 'conv3', P2, 136, [FR(32)], 1, [ws(1, 4, 9, FAST, 1)], [f32k(1, 4, 9)])
_add('c1-3x3-gen-relu', 'conv3', P0, 128, [GR(32)], 1, [ws(1, 4, 9, GENERIC)], [f32k(1, 4, 9)])
_add('c1-3x3-gen-res', 'conv3', P2, 136, [GX(40)], 1, [gen(1, 4, 9, 1)], [f32k(1, 4, 9)])
_add('c1-3x3-pool-floor', 'conv3', P2, 128, [GA(32, pool=1)], 1, [gen(1, 4, 9)])
_add('c1-3x3-pool-ceil-kq', 'conv3', P1, 24, [GA(40, pool=2)], 1, [gen(1, 4, 9)])
_add('c1-3x3-kq-plain-sweep', 'conv3', P4, 24, [PL(40)], 1, [ws(1, 1, 9, PLAIN)], [f32k(1, 4, 9)], ks=SWEEP)
_add('c1-3x3-kq-fast', 'conv3', P2, 24, [FA(32)], 1, [ws(1, 1, 9, FAST)], [f32k(1, 4, 9)])
_add('c1-3x3-kq-fast-res', 'conv3', P1, 32, [FR(40)], 1, [ws(1, 1, 9, FAST, 1)], [f32k(1, 4, 9)])
_add('c1-3x3-kq-gen-f16', 'conv3', P2, 24, [GH(32)], 1, [ws(1, 1, 9, GENERIC)])
_add('c1-3x3-kq-gen-res', 'conv3', P2, 24, [GX(32)], 1, [gen(1, 4, 9, 1)], [f32k(1, 4, 9)])
_add('c1-1x1-plain', 'conv1', P2, 136, [PL(40)], 1, [ws(1, 4, 1, PLAIN)], [f32k(1, 4, 1)])
_add('c1-1x1-kq-fast', 'conv1', P4, 24, [FA(32)], 1, [ws(1, 1, 1, FAST)], [f32k(1, 4, 1)])
_add('c1-1x1-kq-gen', 'conv1', P1, 8, [GA(40)], 1, [ws(1, 1, 1, GENERIC)], [f32k(1, 4, 1)])
_add('c1-T4-plain', 'convT4', P2, 136, [PL(40)], 1, [ws(1, 4, 4, PLAIN)], [f32k(1, 4, 4)], lattices=('L0', 'L1', 'L2'))
_add('c1-T4-kq-fast', 'convT4', P1, 24, [FA(32)], 1, [ws(1, 1, 4, FAST)], [f32k(1, 4, 4)])
_add('c1-T4-kq-plain', 'convT4', P4, 24, [PL(32)], 1, [ws(1, 1, 4, PLAIN)], [f32k(1, 4, 4)])
_add('c1-T2-plain', 'convT2', P2, 128, [PL(32)], 1, [ws(1, 4, 1, PLAIN)], [f32k(1, 4, 1)])
_add('c1-T2-kq-gen', 'convT2', P1, 24, [GA(40)], 1, [ws(1, 1, 1, GENERIC)], [f32k(1, 4, 1)])
_add('c1-s2-plain', 'conv3s2', P2, 136, [PL(16)], 1, [ws(1, 4, 9, PLAIN)] * 2, [f32k(1, 4, 9)] * 2)        # (fp32 entry takes the views)
_add('c1-s2-kq', 'conv3s2', P1, 24, [PL(20)], 1, [ws(1, 1, 9, PLAIN)] * 2, [f32k(1, 4, 9)] * 2)

# ---- CI 64 / CO 64 (ci_tiles 2): C in {64, 72, 16 with 3 real}, Cout in {64, 72, 32, 8}; fp32 3x3 / 1x1: wgrad_ws32_kernel
_add('c2-3x3-plain-sweep', 'conv3', P4, 64, [PL(64)], 2, [ws(2, 2, 9, PLAIN)], [ws32(9, 0, 0)], ks=SWEEP, lattices=('L0', 'L1', 'L2'))
_add('c2-3x3-fast-ragged', 'conv3', P2, 72, [FA(72)], 2, [ws(2, 2, 9, FAST)], [ws32(9, 1, 0)])
_add('c2-3x3-fast-res', 'conv3', P3, 72, [FR(72)], 2, [ws(2, 2, 9, FAST, 1)], [ws32(9, 2, 0)])
_add('c2-3x3-gen-affine', 'conv3', P1, 64, [GA(72)], 2, [ws(2, 2, 9, GENERIC)], [ws32(9, 2, 0)])
_add('c2-3x3-gen-relu', 'conv3', P2, 8, [GR(64)], 2, [ws(2, 2, 9, GENERIC)], [ws32(9, 2, 2)])
_add('c2-3x3-gen-f16', 'conv3', P0, 72, [GH(64)], 2, [ws(2, 2, 9, GENERIC)])
_add('c2-3x3-gen-res', 'conv3', P2, 72, [GX(72)], 2, [gen(2, 2, 9, 1)], [ws32(9, 2, 0)])
_add('c2-3x3-pool-floor', 'conv3', P2, 72, [GA(64, pool=1)], 2, [gen(2, 2, 9)])
_add('c2-3x3-pool-ceil', 'conv3', P4, 32, [GA(72, pool=2)], 2, [gen(2, 2, 9)])
_add('c2-3x3-pool-ceil-relu', 'conv3', P1, 64, [FA(64, pool=2)], 2, [gen(2, 2, 9)])       # (the non-negative packed maximum)
_add('c2-3x3-stem', 'conv3', P2, 64, [PL(16, creal=3)], 2, [ws(2, 2, 9, PLAIN)], [ws32(9, 0, 3)])
_add('c2-3x3-stem-sweep', 'conv3', P4, 72, [PL(16, creal=3)], 2, [ws(2, 2, 9, PLAIN)], [ws32(9, 0, 3)], ks=SWEEP)
_add('c2-3x3-pad01', 'conv3', P2, 64, [GA(64, hs=8, ws=14, off=(0, 1))], 2, [ws(2, 2, 9, GENERIC)], [ws32(9, 2, 0)])
_add('c2-3x3-pad11', 'conv3', P4, 72, [FA(72, hs=15, ws=30, off=(1, 1))], 2, [ws(2, 2, 9, FAST)], [ws32(9, 1, 0)])
_add('c2-3x3-concat', 'conv3', P2, 72, [PL(64), FR(72, hs=8, ws=14, off=(0, 1))], 2, [ws(2, 2, 9, PLAIN), ws(2, 2, 9, FAST, 1)],
     [ws32(9, 0, 0), ws32(9, 2, 0)])
_add('c2-3x3-concat-pool', 'conv3', P3, 64, [FA(32, pool=1), GX(40, hs=4, ws=31, off=(1, 1))], 2, [gen(2, 2, 9), gen(2, 2, 9, 1)])
_add('c2-1x1-concat', 'conv1', P2, 72, [FA(72), PL(16, creal=3)], 2, [ws(2, 2, 1, FAST), ws(2, 2, 1, PLAIN)], [ws32(1, 1, 0), ws32(1, 0, 3)])
_add('c2-s2-plain', 'conv3s2', P2, 72, [PL(32)], 2, [ws(2, 2, 9, PLAIN)] * 2, [ws32(9, 0, 0)] * 2, lattices=('L0', 'L1'))
_add('c2-s2-sweep', 'conv3s2', P4, 32, [PL(16)], 2, [ws(2, 2, 9, PLAIN)] * 2, [ws32(9, 0, 1)] * 2, ks=SWEEP)
# the fp32 quadrant modes on each side of their `<= 32` thresholds, for taps 9, 1 (wgrad_ws32_kernel), 4 and the k2 transposed form
# (wgrad_f32_kernel<2, 2>); source forms plain / fast / fast with residual (16-bit names: fp32 runs XF 0 / 1 / 2)
_QM_WS32 = {(32, 32): 1, (64, 32): 2, (32, 64): 3, (40, 40): 0}
_QM_F32K = {(32, 32): 1, (64, 32): 2, (32, 64): 0, (40, 40): 0}
_SHAPES = [P1, P2, P3, P4]
for _i, ((_c, _co), _qm) in enumerate(_QM_WS32.items()):
    for _kind, _taps in (('conv3', 9), ('conv1', 1)):
        for _xf, (_mk, _f16) in enumerate(((PL, ws(2, 2, _taps, PLAIN)), (FA, ws(2, 2, _taps, FAST)), (FR, ws(2, 2, _taps, FAST, 1)))):
            _sh = _SHAPES[(_i + _xf + _taps) % 4]
            _add('c2-qm-%s-%dx%d-xf%d' % (_kind, _c, _co, _xf), _kind, _sh, _co, [_mk(_c)], 2, [_f16], [ws32(_taps, _xf, _qm)],
                 ks=SWEEP if (_sh == P4 and _xf == 0) else None, lattices=('L0', 'L1', 'L2') if _xf == 0 else ('L0',))
for _i, ((_c, _co), _qm) in enumerate(_QM_F32K.items()):
    for _kind, _taps in (('convT4', 4), ('convT2', 1)):
        _mk, _f16 = ((PL, ws(2, 2, _taps, PLAIN)), (FA, ws(2, 2, _taps, FAST)))[_i % 2]
        _sh = _SHAPES[(_i + _taps) % 4]
        _add('c2-qm-%s-%dx%d' % (_kind, _c, _co), _kind, _sh, _co, [_mk(_c)], 2, [_f16], [f32k(2, 2, _taps, _qm)],
             lattices=('L0', 'L1', 'L2') if _mk is PL else ('L0',))

# ---- CI 128 / CO 32 (ci_tiles 4): C in {128, 136}, Cout in {32, 40}; 16-bit: always wgrad_kernel<4, 1>
_add('c4-3x3-plain-sweep', 'conv3', P4, 32, [PL(128)], 4, [gen(4, 1, 9)], [f32k(4, 1, 9)], ks=SWEEP, lattices=('L0', 'L1', 'L2'))
_add('c4-3x3-fast-ragged', 'conv3', P2, 40, [FA(136)], 4, [gen(4, 1, 9)], [f32k(4, 1, 9)])
_add('c4-3x3-fast-res', 'conv3', P1, 40, [FR(128)], 4, [gen(4, 1, 9, 1)], [f32k(4, 1, 9)])
_add('c4-3x3-gen-res', 'conv3', P2, 32, [GX(136)], 4, [gen(4, 1, 9, 1)], [f32k(4, 1, 9)])
_add('c4-3x3-pool-ceil', 'conv3', P2, 40, [GA(136, pool=2)], 4, [gen(4, 1, 9)])
_add('c4-3x3-pool-floor-relu', 'conv3', P1, 32, [FA(128, pool=1)], 4, [gen(4, 1, 9)])
_add('c4-1x1', 'conv1', P2, 40, [PL(136)], 4, [gen(4, 1, 1)], [f32k(4, 1, 1)])
_add('c4-T4', 'convT4', P2, 40, [FA(136)], 4, [gen(4, 1, 4)], [f32k(4, 1, 4)])
_add('c4-T4-sweep', 'convT4', P4, 32, [PL(128)], 4, [gen(4, 1, 4)], [f32k(4, 1, 4)], ks=(1, 7, 40))
_add('c4-T2', 'convT2', P1, 32, [PL(128)], 4, [gen(4, 1, 1)], [f32k(4, 1, 1)])
_add('c4-s2', 'conv3s2', P2, 40, [PL(68)], 4, [gen(4, 1, 9)] * 2, [f32k(4, 1, 9)] * 2)

# ---- the remaining kind x source-form instantiations (no model builds most of them; the ABI reaches them)
for _n, (_kind, _ci, _co, _src, _f16, _f32) in enumerate([
        ('conv1', 1, 136, FA(40), ws(1, 4, 1, FAST), f32k(1, 4, 1)), ('convT2', 1, 128, FR(32), ws(1, 4, 1, FAST, 1), f32k(1, 4, 1)),
        ('conv1', 1, 128, GR(40), ws(1, 4, 1, GENERIC), f32k(1, 4, 1)), ('convT2', 1, 24, PL(40), ws(1, 1, 1, PLAIN), f32k(1, 4, 1)),
        ('conv1', 1, 32, FR(32), ws(1, 1, 1, FAST, 1), f32k(1, 4, 1)), ('convT4', 1, 128, FA(32), ws(1, 4, 4, FAST), f32k(1, 4, 4)),
        ('convT4', 1, 136, FR(40), ws(1, 4, 4, FAST, 1), f32k(1, 4, 4)), ('convT4', 1, 128, GA(40), ws(1, 4, 4, GENERIC), f32k(1, 4, 4)),
        ('convT4', 1, 32, FR(32), ws(1, 1, 4, FAST, 1), f32k(1, 4, 4)), ('convT4', 1, 8, GH(40), ws(1, 1, 4, GENERIC), None),
        ('conv1', 2, 72, GA(72), ws(2, 2, 1, GENERIC), ws32(1, 2, 0)), ('convT4', 2, 72, FR(64), ws(2, 2, 4, FAST, 1), f32k(2, 2, 4)),
        ('convT4', 2, 64, GR(72), ws(2, 2, 4, GENERIC), f32k(2, 2, 4)),
        ('conv1', 1, 128, GA(40, pool=2), gen(1, 4, 1), None), ('convT2', 1, 136, GX(32), gen(1, 4, 1, 1), f32k(1, 4, 1)),
        ('convT4', 1, 24, GA(32, pool=1), gen(1, 4, 4), None), ('convT4', 1, 128, GX(40), gen(1, 4, 4, 1), f32k(1, 4, 4)),
        ('convT2', 2, 72, FA(64, pool=2), gen(2, 2, 1), None), ('conv1', 2, 64, GX(72), gen(2, 2, 1, 1), ws32(1, 2, 0)),
        ('convT4', 2, 64, GA(72, pool=2), gen(2, 2, 4), None), ('convT4', 2, 72, GX(64), gen(2, 2, 4, 1), f32k(2, 2, 4)),
        ('conv1', 4, 40, GX(128), gen(4, 1, 1, 1), f32k(4, 1, 1)), ('convT4', 4, 32, FR(136), gen(4, 1, 4, 1), f32k(4, 1, 4))]):
    _add('x%02d-%s-c%d' % (_n, _kind, _ci), _kind, _SHAPES[_n % 3], _co, [_src], _ci, [_f16], None if _f32 is None else [_f32])

CASE_BY_ID = {c.id: c for c in CASES}
assert len(CASE_BY_ID) == len(CASES)


def runs(precisions=('16', '32'), lattices=('L0', 'L1', 'L2')):
    """(case, precision, lattice) of every run of the exact tests; L1 / L2 exist for plain fp32 sources only"""
    out = []
    for c in CASES:
        for p in precisions:
            if (c.form16 if p == '16' else c.form32) is None:
                continue
            for lat in c.lattices:
                if lat in lattices and (lat == 'L0' or p == '32'):
                    out.append((c, p, lat))
    return out


def table_forms():
    return {f for c in CASES for fs in (c.form16, c.form32) if fs for f in fs}


# every instantiation cdnet_conv_backward_weight can reach without CDNET_WGRAD_DEBUG, read from launch_wgrad / launch_wgrad_f32 /
# launch_wgrad_ws32 (csrc/wgrad.hip)
REACHABLE = set()
for _t in (9, 4, 1):
    # launch_wgrad, 16-bit: un-pooled CI_T 1 / 2 sources -> wgrad_ws_kernel (plain | fast [+ residual] | generic without residual),
    # <1, 4> with at most 32 output channels -> <1, 1>; pooled, CI_T 4 and generic + residual -> wgrad_kernel
    for _ci, _co in ((1, 1), (1, 4), (2, 2)):
        REACHABLE |= {ws(_ci, _co, _t, PLAIN), ws(_ci, _co, _t, FAST), ws(_ci, _co, _t, FAST, 1), ws(_ci, _co, _t, GENERIC)}
    REACHABLE |= {gen(4, 1, _t), gen(4, 1, _t, 1), gen(1, 4, _t), gen(1, 4, _t, 1), gen(2, 2, _t), gen(2, 2, _t, 1)}
    # launch_wgrad_f32: <2, 2> with taps 9 | 1 at ostride 1 -> wgrad_ws32_kernel; quadrant modes 1 / 2 of wgrad_f32_kernel<2, 2> for the
    # transposed forms only
    REACHABLE |= {f32k(1, 4, _t), f32k(4, 1, _t)}
REACHABLE |= {f32k(2, 2, _t, _q) for _t in (4, 1) for _q in (0, 1, 2)} | {f32k(2, 2, 9)}
REACHABLE |= {ws32(_t, _x, _q) for _t in (9, 1) for _x in (0, 1, 2) for _q in (0, 1, 2, 3)}

# reachable through the ABI, not run by the table - with the reason
NOT_COVERED = {
    f32k(2, 2, 9): 'wgrad_f32_kernel<2, 2, 9>: only with CDNET_WGRAD_WS32=0 (read once per process) or tensors of 2^30 elements',
}
# (also not run: everything behind CDNET_WGRAD_DEBUG bits 8 and 16 - the variable is read once per process)


# ---- data -------------------------------------------------------------------------------------------------------------------------
def dims(case):
    """(N, H, W, Ho, Wo): logical input size of the kernel call and the gradient's size"""
    N, H, W = case.shape
    o = KINDS[case.kind][2]
    return N, H, W, H * o, W * o


def stored_hw(case, s):
    N, H, W = case.shape
    if case.kind == 'conv3s2':
        return 2 * H, 2 * W
    if s.pool:                                   # odd sizes: the floor mode drops a row / column, ceil-mode windows stick out
        return (s.hs or (2 * H + 1 if s.pool == 1 else 2 * H - 1)), (s.ws or (2 * W + 1 if s.pool == 1 else 2 * W - 1))
    return s.hs or H, s.ws or W


def make_data(case, lattice='L0'):
    """stored tensors of a case as float64 NCHW torch tensors: dict(src=[dict(x, scale, shift, res)], g=...)"""
    rng = np.random.default_rng(zlib.crc32((case.id + lattice).encode()))
    N, H, W, Ho, Wo = dims(case)
    t64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))

    def ints(shape, lo=-3, hi=3):
        return rng.integers(lo, hi + 1, size=shape).astype(np.float64)

    def fine(shape):
        return rng.integers(-1024, 1024, size=shape).astype(np.float64) / 256.0

    def real(shape):
        return rng.standard_normal(size=shape)

    srcs = []
    for s in case.srcs:
        hs, ws_ = stored_hw(case, s)
        shp = (N, s.C, hs, ws_)
        d = dict(scale=None, shift=None, res=None)
        if lattice == 'L0':
            x = ints(shp)
            x[(x == 0) & (rng.random(shp) < 0.5)] = -0.0
            if s.aff:
                d['scale'] = t64(rng.choice([1.0, -1.0, 2.0, -2.0, 0.5], size=s.C))
                sh = ints((s.C,), -2, 2)
                sh[(sh == 0) & (rng.random(s.C) < 0.5)] = -0.0
                d['shift'] = t64(sh)
            if s.res:
                d['res'] = t64(ints(shp))
        elif lattice in ('L1', 'L2'):
            assert not (s.aff or s.relu or s.res or s.pool), 'L1 / L2 are lattices of plain sources'
            x = fine(shp) if lattice == 'L1' else ints(shp)
        else:                                    # 'real': the derived-bound tests
            x = real(shp)
            if s.aff:
                sc = rng.random(s.C) + 0.5
                sc[::3] *= -1.0
                d['scale'], d['shift'] = t64(sc.astype(np.float32)), t64((0.3 * real((s.C,))).astype(np.float32))
            if s.res:
                d['res'] = t64(real(shp))
        d['x'] = t64(x)
        srcs.append(d)
    gshape = (N, case.Cout, Ho, Wo)
    g = fine(gshape) if lattice == 'L2' else (real(gshape) if lattice == 'real' else ints(gshape))
    return dict(src=srcs, g=t64(g), lattice=lattice)


def store_dtype(s, prec):
    return torch.float32 if prec == '32' else (torch.float16 if s.store == 'fp16' else torch.bfloat16)


def rounded(data, case, prec):
    """the stored values as the device tensors hold them (float64 again): identity on the lattices"""
    out = dict(src=[], g=data['g'].to(torch.float32 if prec == '32' else torch.bfloat16).double(), lattice=data['lattice'])
    for s, d in zip(case.srcs, data['src']):
        dt = store_dtype(s, prec)
        out['src'].append(dict(x=d['x'].to(dt).double(), res=None if d['res'] is None else d['res'].to(dt).double(),
                               scale=d['scale'], shift=d['shift']))
    return out


# ---- float64 reference --------------------------------------------------------------------------------------------------------------
def transformed(s, d, prec):
    """the source's lazy transform with the kernels' rounding points: fma(x, scale, shift) rounded to fp32, + residual rounded to fp32,
    ReLU, (16-bit path) rounded to bf16; then the 2x2 maximum (ceil mode: windows that stick out use the pixels that exist)"""
    t = d['x']
    if d['scale'] is not None:
        t = (t * d['scale'].view(1, -1, 1, 1) + d['shift'].view(1, -1, 1, 1)).float().double()
    if d['res'] is not None:
        t = (t + d['res']).float().double()
    if s.relu:
        t = t.clamp_min(0.0)
    if prec == '16':
        t = t.float().bfloat16().double()
    if s.pool:
        t = F.max_pool2d(t, 2, ceil_mode=(s.pool == 2))
    return t


def logical_input(case, data, prec):
    """the layer's input [N][sum C][H][W] (conv3s2: the full-resolution input [N][Cp][2H][2W]): every source transformed and placed at
    its F.pad offset (cropped to the layer's size), channels concatenated in torch.cat order"""
    N, H, W = case.shape
    if case.kind == 'conv3s2':
        return transformed(case.srcs[0], data['src'][0], prec)
    parts = []
    for s, d in zip(case.srcs, data['src']):
        t = transformed(s, d, prec)
        a = torch.zeros((N, s.C, H, W), dtype=torch.float64)
        oy, ox = s.off
        h, w = min(t.shape[2], H - oy), min(t.shape[3], W - ox)
        a[:, :, oy:oy + h, ox:ox + w] = t[:, :, :h, :w]
        parts.append(a)
    return torch.cat(parts, 1)


def _taps_sum(kind, A, G):
    """sum over images and pixels of A (x) G per kernel tap, in the PyTorch weight layout, straight from the layer's definition"""
    N, _, H, W = A.shape
    if kind in ('conv3', 'conv1'):
        k = 3 if kind == 'conv3' else 1
        Ap = F.pad(A, (k // 2,) * 4)
        return torch.stack([torch.stack([torch.einsum('nchw,nohw->oc', Ap[:, :, ky:ky + H, kx:kx + W], G) for kx in range(k)], -1)
                            for ky in range(k)], -2)
    if kind == 'conv3s2':                        # y[oy] reads x[2 oy - 1 + kh]
        Ho, Wo = G.shape[2:]
        Ap = F.pad(A, (1,) * 4)
        return torch.stack([torch.stack([torch.einsum('nchw,nohw->oc', Ap[:, :, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2], G) for kx in range(3)], -1)
                            for ky in range(3)], -2)
    if kind == 'convT4':                         # x[iy] lands on y[2 iy - 1 + kh]
        Gp = F.pad(G, (1,) * 4)
        return torch.stack([torch.stack([torch.einsum('nchw,nohw->co', A, Gp[:, :, ky:ky + 2 * H:2, kx:kx + 2 * W:2]) for kx in range(4)], -1)
                            for ky in range(4)], -2)
    assert kind == 'convT2'                      # x[iy] lands on y[2 iy + kh]
    return torch.stack([torch.stack([torch.einsum('nchw,nohw->co', A, G[:, :, ky::2, kx::2]) for kx in range(2)], -1) for ky in range(2)], -2)


def ref_dw(case, data, prec):
    """(dW, sum |a * g|) float64 in the PyTorch layout over the STORED channels of every source (padded channels included: the real
    ones are selected by `owned`)"""
    r = rounded(data, case, prec)
    A = logical_input(case, r, prec)
    return _taps_sum(case.kind, A, r['g']), _taps_sum(case.kind, A.abs(), r['g'].abs())


def unit(lattice):
    return {'L0': 0.5, 'L1': 2.0 ** -8, 'L2': 2.0 ** -8}[lattice]


def guard(case, data, prec, dw, sabs):
    """the exact regime: every term and every partial sum is a whole number of lattice units below 2^24"""
    u = unit(data['lattice'])
    assert float(sabs.max()) / u < 2.0 ** 24, (case.id, float(sabs.max()) / u)
    assert torch.equal(dw / u, torch.round(dw / u)) and torch.equal(dw.float().double(), dw), case.id
    r = rounded(data, case, prec)
    for d0, d1 in zip(data['src'], r['src']):
        assert torch.equal(d0['x'], d1['x']) and (d0['res'] is None or torch.equal(d0['res'], d1['res'])), case.id      # stored exactly
    assert torch.equal(data['g'], r['g']), case.id
    if data['lattice'] == 'L0':
        for s, d in zip(case.srcs, data['src']):
            t = d['x'] * (1.0 if d['scale'] is None else d['scale'].view(1, -1, 1, 1)) + (0.0 if d['shift'] is None else d['shift'].view(1, -1, 1, 1))
            t = t + (0.0 if d['res'] is None else d['res'])
            assert float(t.abs().max()) <= 11.0 and torch.equal(t * 2, torch.round(t * 2)), case.id
            assert torch.equal(t.bfloat16().double(), t) and torch.equal(t.half().double(), t), case.id


# ---- which dW elements a source's call owns ------------------------------------------------------------------------------------------
def layer_channels(case):
    """(stored channels per kernel source, src_coff per source, Csrc_real per source, Cin_real)"""
    if case.kind == 'conv3s2':
        Cp = case.srcs[0].C
        return [2 * Cp, 2 * Cp], [0, 2 * Cp], [2 * Cp, 2 * Cp], 4 * Cp
    Cs = [s.C for s in case.srcs]
    real = [s.creal or s.C for s in case.srcs]
    coffs, c = [], 0
    for s in case.srcs:                          # (a padded source is the layer's last: the stem has one)
        coffs.append(c)
        c += s.C
    return Cs, coffs, real, sum(real) if any(s.creal for s in case.srcs) else c


def dw_shape(case):
    k = {'conv3': 3, 'conv1': 1, 'convT4': 4, 'convT2': 2, 'conv3s2': 3}[case.kind]
    _, _, _, cin_real = layer_channels(case)
    if case.kind == 'conv3s2':
        cin_real //= 4
    return (cin_real, case.Cout, k, k) if case.kind.startswith('convT') else (case.Cout, cin_real, k, k)


def real_dw(case, dw_stored):
    """the reference over stored channels -> the layer's dW (padded input channels dropped)"""
    Cs, coffs, real, cin_real = layer_channels(case)
    if case.kind == 'conv3s2':
        return dw_stored
    ax = 0 if case.kind.startswith('convT') else 1
    keep = torch.cat([torch.arange(c0, c0 + r) for c0, r in zip(np.cumsum([0] + Cs[:-1]).tolist(), real)])
    return dw_stored.index_select(ax, keep)


def owned(case, i):
    """bool mask over dW: the elements the call for kernel source i must write (everything else must stay untouched)"""
    Cs, coffs, real, cin_real = layer_channels(case)
    m = torch.zeros(dw_shape(case), dtype=torch.bool)
    if case.kind == 'conv3s2':                   # row-parity view a holds input rows 2y + a: kh = 1 (a = 0) or kh in {0, 2} (a = 1)
        m[:, :, [1] if i == 0 else [0, 2], :] = True
    elif case.kind.startswith('convT'):
        m[coffs[i]:coffs[i] + real[i]] = True
    else:
        m[:, coffs[i]:coffs[i] + real[i]] = True
    return m


# ---- numpy restatement of the reduce: sum over the split slices, scatter into the PyTorch layout ----------------------------------------
def scatter_index(mode, npar, ci_blocks, co_blocks, taps, CI, CO, Csrc_real, Cin_real, src_coff, Cout):
    """for every element of one slice of the slab [npar][ci_blocks][co_blocks][taps][CI][CO] the flat index of the dW element it is
    summed into, -1 where it is dropped (padded channels, structurally zero tap / parity pairs of the stride-2 form)"""
    per = npar * ci_blocks * co_blocks * taps * CI * CO
    r = np.arange(per, dtype=np.int64)
    co_l = r % CO; r //= CO
    ci_l = r % CI; r //= CI
    tap = r % taps; r //= taps
    cb = r % co_blocks; r //= co_blocks
    ib = r % ci_blocks; par = r // ci_blocks
    cs, co = ib * CI + ci_l, cb * CO + co_l
    ci = src_coff + cs
    ok = (cs < Csrc_real) & (co < Cout)
    if mode == 0:
        o = (co * Cin_real + ci) * taps + tap
    elif mode == 6:
        Ct = Cin_real // 4
        a, b, c = ci // (2 * Ct), (ci // Ct) % 2, ci % Ct
        kh, kw = 2 * (tap // 3 - 1) + a + 1, 2 * (tap % 3 - 1) + b + 1
        ok &= (kh >= 0) & (kh <= 2) & (kw >= 0) & (kw <= 2)
        o = ((co * Ct + c) * 3 + kh) * 3 + kw
    elif mode == 2:
        a, b, ty, tx = par // 2, par % 2, tap // 2, tap % 2
        kh = np.where(a == 0, np.where(ty == 0, 1, 3), np.where(ty == 0, 0, 2))
        kw = np.where(b == 0, np.where(tx == 0, 1, 3), np.where(tx == 0, 0, 2))
        o = ((ci * Cout + co) * 4 + kh) * 4 + kw
    else:
        assert mode == 3
        o = ((ci * Cout + co) * 2 + par // 2) * 2 + par % 2
    return np.where(ok, o, -1)


def reduce_ref(slab, idx, dw0):
    """slab [ksplit][per] of lattice values (exact in any order), idx from scatter_index, dw0 the flat dW before the call"""
    s = slab.astype(np.float64).sum(0)
    out = dw0.copy()
    out[idx[idx >= 0]] = s[idx >= 0].astype(np.float32)
    return out


def emulate_slab(kind, A, G, CI, CO):
    """one slice of the slab as the kernels define it - slab[par][ib][cb][tap][ci][co] = sum over pixels p of A[p + tap] * G[ostride p +
    par] - for ONE source (A [N][C][H][W] the logical input, G the gradient), float64.  The tap offsets are the staging code's: 3x3
    tap t reads halo pixel (t / 3, t % 3) - 1; the k4 transposed form reads halo row (pa == 0 ? (ty == 0 ? 1 : 0) : (ty == 0 ? 2 : 1))."""
    taps, npar, ostride, _ = KINDS[kind]
    N, C, H, W = A.shape
    Cout = G.shape[1]
    cib, cob = -(-C // CI), -(-Cout // CO)
    Ap = F.pad(A, (1, 1, 1, 1, 0, cib * CI - C))
    Gz = F.pad(G, (0, 0, 0, 0, 0, cob * CO - Cout))
    slab = torch.zeros((npar, cib, cob, taps, CI, CO), dtype=torch.float64)
    for par in range(npar):
        pa, pb = par >> 1, par & 1
        Gs = Gz[:, :, pa::ostride, pb::ostride]
        for t in range(taps):
            if taps == 9:
                r, c = t // 3, t % 3
            elif taps == 4:
                ty, tx = t >> 1, t & 1
                r = (1 if ty == 0 else 0) if pa == 0 else (2 if ty == 0 else 1)
                c = (1 if tx == 0 else 0) if pb == 0 else (2 if tx == 0 else 1)
            else:
                r, c = 1, 1
            full = torch.einsum('nchw,nohw->co', Ap[:, :, r:r + H, c:c + W], Gs)
            slab[par, :, :, t] = full.view(cib, CI, cob, CO).permute(0, 2, 1, 3)
    return slab.reshape(-1)


# ---- error bound of the real-valued tests ---------------------------------------------------------------------------------------------
def chain_length(family, shape, ksplit):
    """longest chain of fp32 roundings behind one dW element ("Weight-gradient error bound"):
    pixels of a tile (each MFMA counted as its k-depth of sequential roundings - an ASSUMPTION, the order inside an MFMA is not
    documented; x 3 MFMAs per k-step on the fp32 path) x tiles per slice, + 3 for the folds across the waves of a workgroup (at most
    three sequential additions), + the reduce: ceil(ksplit / 4) additions per k-lane, 3 in the tree of eight, 2 across the four lanes"""
    N, H, W = shape
    th = 4 if family == WS32 else 8
    ntiles = N * -(-H // th) * -(-W // 16)
    per_tile = th * 16 * (3 if family in (WS32, F32K) else 1)
    return per_tile * -(-ntiles // ksplit) + 3 + -(-ksplit // 4) + 3 + 2


def bound(family, shape, ksplit, sabs):
    c = chain_length(family, shape, ksplit)
    u = 2.0 ** -24
    return ((2.0 ** -16 if family in (WS32, F32K) else 0.0) + c * u) * sabs


# ---- device side ----------------------------------------------------------------------------------------------------------------------
def _nhwc(t, dtype):
    return t.permute(0, 2, 3, 1).contiguous().to(dtype).cuda()


def device_sources(case, data, prec):
    """(list of engine.Src, gradient tensor, keep-alive list)"""
    from cdnet_amd import engine
    g = _nhwc(data['g'], torch.float32 if prec == '32' else torch.bfloat16)
    N, H, W = case.shape
    if case.kind == 'conv3s2':
        s = case.srcs[0]
        xd = _nhwc(data['src'][0]['x'], store_dtype(s, prec))
        W2 = 2 * W
        return [engine.Src(xd, view=(a * W2 * s.C, H, W, 2 * s.C, 2 * W2 * s.C)) for a in (0, 1)], g
    out = []
    for s, d in zip(case.srcs, data['src']):
        dt = store_dtype(s, prec)
        f = lambda v: None if v is None else v.float().cuda()
        out.append(engine.Src(_nhwc(d['x'], dt), f(d['scale']), f(d['shift']), relu=s.relu, pool=s.pool,
                              res=None if d['res'] is None else _nhwc(d['res'], dt), off=s.off))
    return out, g


class DwBuffer:
    """dW inside a larger sentinel-filled buffer"""

    def __init__(self, shape):
        self.shape, self.n = shape, int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * SLACK,), SENTINEL, dtype=torch.float32, device='cuda')

    def ptr(self):
        import ctypes as C
        return C.c_void_p(self.buf.data_ptr() + 4 * SLACK)

    def read(self):
        """(dW on the host, True if the slack on both ends still holds the sentinel)"""
        h = self.buf.cpu()
        s = torch.full((SLACK,), SENTINEL, dtype=torch.float32)
        return h[SLACK:SLACK + self.n].view(self.shape), torch.equal(h[:SLACK], s) and torch.equal(h[SLACK + self.n:], s)


def launch(case, srcs, g, i, ksplit, dwbuf, defer=False):
    """cdnet_conv_backward_weight for kernel source i; returns (form of the launch, slab, arguments of cdnet_wgrad_reduce_desc_fill)"""
    import ctypes as C
    from cdnet_amd import _lib, engine
    lib = _lib.load()
    taps, npar, ostride, mode = KINDS[case.kind]
    N, H, W = case.shape
    Cs, coffs, real, cin_real = layer_channels(case)
    s = srcs[i]
    slab = torch.full((lib.cdnet_conv_wgrad_slab_floats(s.C, case.Cout, taps, npar, case.ci_t, ksplit),), float('nan'),
                      dtype=torch.float32, device='cuda')            # (a slice without tiles must still write zeros)
    cs = engine.ConvSrc()
    s.fill(cs)
    _lib.call('cdnet_conv_backward_weight', C.byref(cs), coffs[i], real[i], cin_real, _lib.ptr(g), case.Cout, N, H, W, taps, npar, ostride,
              case.ci_t, ksplit, _lib.ptr(slab), dwbuf.ptr(), mode | (DEFER if defer else 0), _lib.stream_ptr())
    return lib.cdnet_conv_backward_weight_last_form(), slab, (s.C, coffs[i], real[i], cin_real, case.Cout, taps, npar, case.ci_t, ksplit,
                                                              _lib.ptr(slab), dwbuf.ptr(), mode)


def reduce_batch(arg_list):
    """one cdnet_wgrad_reduce_batch launch over the descriptors of `arg_list` (arguments of cdnet_wgrad_reduce_desc_fill without block0)"""
    import ctypes as C
    from cdnet_amd import _lib
    descs = (_lib.WgradReduceDesc * len(arg_list))()
    b0 = 0
    for i, a in enumerate(arg_list):
        _lib.call('cdnet_wgrad_reduce_desc_fill', *a, b0, C.byref(descs[i]))
        assert descs[i].block0 == b0 and descs[i].blocks > 0
        b0 += descs[i].blocks
    tab = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).cuda()
    _lib.call('cdnet_wgrad_reduce_batch', _lib.ptr(tab), len(arg_list), b0, _lib.stream_ptr())
    torch.cuda.synchronize()
    return descs
