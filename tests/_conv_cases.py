"""Case table, data lattices, float64 reference and device runner of the exact convolution tests (cdnet_conv_forward: csrc/conv.hip,
conv16ws.hip, conv32.hip, conv32ws.hip - forward, transposed and backward-data), shared by test_conv_refs_cpu.py (pins the reference
to PyTorch on the CPU and proves every row to be in the exact regime) and test_gpu_conv_exact.py.  Built after _wgrad_cases.py, whose
source descriptions (S), lazy source transform, placement of padded sources and sentinel constants it reuses.

Lattices: data chosen so that every product a * w and every partial sum is a whole number of lattice units below 2^24 - exact in fp32.
The result then does not depend on the tile, the chunk order, the split into hi / lo operands or the kernel form and must EQUAL the
float64 reference.  One missing, doubled or misplaced term moves an element by at least one unit.
  L0  stored inputs integers in [-3, 3] (some -0.0), source scale in {+-1, +-2, 0.5}, shift and residual integers; weights integers in
      [-3, 3]; bias, oshift and the eres tensor integers, oscale / eres_scale in {+-1, +-2, 0.5}.  Unit 0.5.  Exact in bf16, fp16 and fp32.
  L1  (fp32 mode, plain sources) inputs multiples of 2^-8 in [-4, 4): the bf16 split hi + lo is exact and lo != 0; weights integers.
      Unit 2^-8.  A missing a_lo * w_hi product shows.
  L2  L1 with the roles swapped: the weight pack's lo image is non-zero, a missing a_hi * w_lo product shows.
  LS  (rows with `stats`) inputs, residuals and weights in {-1, 0, 1} at density 1/4, source scale +-1, shift in {-1, 0, 1}: the
      per-channel sum of squared accumulators over the whole launch stays exact too.  Unit 1.
`guard` asserts the regime of a row from the reference alone, before any GPU call.

Every row names the kernel instantiation it must reach (cdnet_conv_forward_last_form; `form` / `form_str` mirror the bit layout of
include/cdnet_hip.h).  Small launches are put on the persistent kernels by cdnet_conv_args.debug bit 64 and their grids are capped by
debug >> 8 (per launch, through engine.conv_forward's debug_or - never through the CDNET_CONV_DEBUG variable, read once per process).

Outputs start from a sentinel inside a larger buffer: the slack on both ends, the channels outside [out_coff, out_coff + Cout) and the
pooled output's slack must still hold it afterwards.  Statistics rows start from NaN.

Instantiations.  The launch sites record 152 distinct forms (REACHABLE below, read from the launchers); the table reaches 149 of them:
  conv_fwd_kernel             27 of 27   nine (tile, CK, BN) keys x taps 9 / 4 / 1
  conv_ws_kernel              24 of 24   BN 64 / 32 x XF 0 / 1 / 2 x STATS x STREAM
  conv_ws16_kernel            40 of 40   BN 64 / 32 x XF 0 / 2 x {streamed k32, out image with quad requests [+ mix], out image with pair
                                         requests [+ mix], direct stores: NCS 1, NCS 2, NCS 0, NCS 0 + mix, NCS 0 + streamed}
  conv_f32_kernel              9 of  9   three (tile, BN) keys x taps 9 / 4 / 1
  conv1x1_f32_stream_kernel   24 of 24   BN 64 / 32 x NCH 1 / 2 / 4 x XF x ERES
  conv_ws32_kernel            25 of 28   BN 64 / 32 x XF 0 / 1 / 2 x STATS (12), NCS 1 / 2 at BN 64 with XF 0 / 1 x STATS (8; XF 2 or BN 32 on
                                         fewer than four chunks: the launcher declines), mix BN 64 / 32 x XF 0 / 2 (4), pool (1),
                                         BatchNorm-backward sums XF 0 / 1 / 2 (3, not reached)
test_conv_refs_cpu.py asserts `table_forms() | NOT_COVERED == REACHABLE` and the two counts.  Not reached, with the reason:
  conv_ws32_kernel's three BatchNorm-backward forms (ws = 2): their second output is a pair of real-valued sums (dz * xhat), not
      lattice-exact; tests/test_gpu_fp32_kernels.py::test_conv_ws32_bn_backward_statistics_epilogue holds them.
(The A/B build switches CDNET_WS16_PAIR_DEFAULT / CDNET_WS16_QUAD_DEFAULT and the CDNET_WS16_OUT variable, read once per process, select
among the same forms and are left at their defaults.)
Not covered at all, each with its existing test:
  ws = 2, the BatchNorm-backward statistics epilogue: test_gpu_fp32_kernels.py::test_conv_ws32_bn_backward_statistics_epilogue;
  dot_out, the fused classifier (a real-valued dot product over the rounded output): test_gpu_conv16ws.py::test_conv_ws16_fused_classifier_output;
  dilated.hip: test_gpu_dilated_conv.py::test_dilated_conv and test_gpu_fullnet_train_kernels.py already compare per element with float64.
Source ReLU modes 0, 1 and 2 are run: the convolution kernels read the field as a flag (mode 2, "mask from the stored output", has a
meaning of its own for cdnet_bn_backward only; conv_ws32_kernel's fast transform form asks for mode 1)."""
import zlib
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

import _wgrad_cases as wc
from _wgrad_cases import S, SENTINEL, SLACK

# ---- kernel forms (bit layout of include/cdnet_hip.h) -----------------------------------------------------------------------------
FWD, WS, WS16, F32K, STREAM, WS32 = 1, 2, 3, 4, 5, 6
_FAMILY = {0: 'none', FWD: 'conv_fwd_kernel', WS: 'conv_ws_kernel', WS16: 'conv_ws16_kernel', F32K: 'conv_f32_kernel',
           STREAM: 'conv1x1_f32_stream_kernel', WS32: 'conv_ws32_kernel'}
_SITE = {WS16: ('direct', 'out-pair', 'out-quad', 'k32'), WS32: ('plain', 'bns', 'mix', 'pool')}
# debug bits (csrc/conv_args.h)
QUAD, ONE_TILE, PERSIST, OLD_WS16, NO_STREAM = 16, 32, 64, 128, 256


def form(family, bn, taps, xf=0, stats=0, stream=0, mix=0, ncs=0, site=0, tile=16, ck=16, nch=0, eres=0):
    return (family | ({32: 0, 64: 1, 128: 2}[bn] << 4) | (taps << 6) | (xf << 10) | (int(stats) << 12) | (int(stream) << 13) | (int(mix) << 14) |
            (ncs << 15) | (site << 17) | ((1 if tile == 8 else 0) << 20) | ({16: 0, 32: 1, 64: 2}[ck] << 21) | (nch << 23) | (int(eres) << 26))


def form_str(f):
    fam = f & 15
    site = (f >> 17) & 7
    return '%s<BN %d, TAPS %d, XF %d, STATS %d, STREAM %d, MIX %d, NCS %d, site %s, tile %d, CK %d, NCH %d, ERES %d>' % (
        _FAMILY.get(fam, '?'), (32, 64, 128, -1)[(f >> 4) & 3], (f >> 6) & 15, (f >> 10) & 3, (f >> 12) & 1, (f >> 13) & 1, (f >> 14) & 1,
        (f >> 15) & 3, _SITE[fam][site] if fam in _SITE and site < 4 else site, 8 if (f >> 20) & 1 else 16, (16, 32, 64, -1)[(f >> 21) & 3],
        (f >> 23) & 7, (f >> 26) & 1)


# kind -> (taps, transposed, pack mode).  bwd*: backward-data through packs 1 (Conv2d) and 4 / 5 (ConvTranspose2d k4 s2 p1 / k2 s2 over the two
# row-parity views of the output gradient); mix: a nine-tap first and a one-tap second source (taps1 = 1)
KINDS = {'conv3': (9, False, 0), 'conv1': (1, False, 0), 'convT4': (4, True, 2), 'convT2': (1, True, 3), 'bwd3': (9, False, 1), 'bwd1': (1, False, 1),
         'bwdT4': (9, False, 4), 'bwdT2': (1, False, 5), 'mix': (9, False, 0)}


@dataclass
class Row:
    id: str
    prec: str                  # '16': bf16 / fp16 tensors, one bf16 MFMA per product; '32': fp32 tensors, the split pack
    kind: str
    shape: tuple               # (N, H, W): the launch's logical input size
    Cout: int
    srcs: list                 # wc.S per source (bwdT4 / bwdT2: ONE entry, the channel count of a row-parity view = 2 x the gradient's channels)
    cfg: tuple                 # (tile, CK, BN)
    form: int
    debug: int = 0
    lattices: tuple = ('L0',)
    bias: bool = False
    oaff: int = 0              # 1: oshift, 2: oscale + oshift
    orelu: bool = False
    eres: int = 0              # 1: the other branch as stored, 2: with its affine
    eres_relu: bool = True
    eres_store: str = 'fp16'
    out_f16: bool = False
    stats: bool = False
    pool_out: bool = False
    pad_chunks: int = 0
    coff: int = 0
    cstride: int = None
    scaled: bool = False       # cdnet_pack_conv_weights_scaled with power-of-two channel scales
    persistent: bool = False   # the grid cap (debug >> 8) applies
    cap: int = 0


ROWS = []


def _add(id, prec, kind, shape, Cout, srcs, cfg, form_, **kw):
    ROWS.append(Row(id, prec, kind, shape, Cout, srcs, cfg, form_, **kw))


def PL(C, **k): return S(C, **k)
def FA(C, **k): return S(C, store='fp16', aff=True, relu=True, **k)                 # raw fp16 + BatchNorm + ReLU: the fast transform
def FR(C, **k): return S(C, store='fp16', aff=True, relu=True, res=True, **k)       # ... with a residual branch
def GA(C, **k): return S(C, aff=True, **k)                                          # affine, no ReLU
def GR(C, **k): return S(C, relu=True, **k)                                         # ReLU without scale / shift
def GH(C, **k): return S(C, store='fp16', **k)                                      # fp16 as stored
def BR(C, **k): return S(C, aff=True, relu=True, **k)                               # BatchNorm + ReLU in the storage type (fp32 mode: the fast form)


_TAP_KINDS = {9: ('conv3', 'bwd3', 'conv3'), 4: ('convT4', 'convT4', 'convT4'), 1: ('conv1', 'convT2', 'bwd1')}
_COUTS = (8, 16, 72)

# ---- conv_fwd_kernel: all nine (tile, CK, BN) keys for taps 9, 4 and 1 (debug bit 32: the one-tile kernel whatever the shape) ------------------
_FWD_KEYS = [(16, 16, 32), (16, 16, 64), (16, 32, 32), (16, 32, 64), (16, 32, 128), (16, 64, 64), (8, 32, 64), (8, 32, 128), (8, 64, 64)]
_SH16 = [(1, 13, 21), (1, 33, 5), (2, 17, 16)]          # ragged against 16-pixel tiles, W < tile, more than one tile per image
_SH8 = [(2, 9, 7), (1, 5, 17), (1, 8, 8)]
for _ti, _taps in enumerate((9, 4, 1)):
    for _i, _key in enumerate(_FWD_KEYS):
        _t, _ck, _bn = _key
        _kind = _TAP_KINDS[_taps][_i % 3]
        _sh = (_SH16 if _t == 16 else _SH8)[(_i + _ti) % 3]
        _co = _COUTS[(_i + _ti) % 3] if _kind[:3] != 'bwd' else 16 * (1 + _i % 2)
        _c = _ck * (1 + (_i + _ti) % 2)
        _add('fwd-%s-t%d-ck%d-bn%d' % (_kind, _t, _ck, _bn), '16', _kind, _sh, _co, [PL(_c)], _key, form(FWD, _bn, _taps, tile=_t, ck=_ck),
             debug=ONE_TILE, bias=bool(_i & 1), oaff=(_i + _ti) % 3, orelu=bool((_i >> 1) & 1))


def _fwd(id, kind, shape, Cout, srcs, key, **kw):
    _add('fwd-' + id, '16', kind, shape, Cout, srcs, key, form(FWD, key[2], KINDS[kind][0], tile=key[0], ck=key[1]), debug=ONE_TILE, **kw)


_fwd('two-src-offsets', 'conv3', (1, 13, 21), 72, [GH(16), GA(32, hs=10, ws=17, off=(2, 3))], (16, 16, 32), bias=True, oaff=2)
_fwd('two-src-1x1', 'conv1', (2, 9, 7), 16, [FA(32), PL(64, hs=7, ws=5, off=(1, 2))], (8, 32, 64), oaff=1, orelu=True)
_fwd('pool-floor', 'conv3', (1, 13, 21), 16, [GA(32, pool=1)], (16, 32, 64), bias=True)               # (scales of both signs: the affine comes first)
_fwd('pool-ceil', 'conv3', (2, 9, 7), 72, [GA(64, pool=2)], (8, 64, 64), oaff=2)
_fwd('pool-ceil-relu', 'conv3', (1, 13, 21), 8, [BR(16, pool=2)], (16, 16, 64))                       # (the non-negative packed maximum)
_fwd('pool-T4', 'convT4', (1, 5, 17), 16, [GA(32, pool=1)], (8, 32, 128))
_fwd('residual', 'conv3', (1, 13, 21), 72, [FR(32)], (16, 16, 64), oaff=2, orelu=True)
_fwd('residual-bf16', 'conv1', (1, 33, 5), 16, [S(32, aff=True, res=True)], (16, 32, 32))
_fwd('relu-only', 'convT2', (2, 9, 7), 8, [GR(32)], (8, 32, 64))
_fwd('parity-views-T4', 'bwdT4', (1, 13, 21), 32, [PL(32)], (16, 16, 32), bias=True)
_fwd('parity-views-T4-ck32', 'bwdT4', (2, 9, 7), 64, [PL(64)], (8, 32, 64))
_fwd('parity-views-T2', 'bwdT2', (1, 13, 21), 16, [PL(32)], (16, 32, 64))
_fwd('eres', 'conv3', (1, 13, 21), 64, [FA(64)], (16, 16, 64), bias=True, eres=1)                      # (the configuration that requests eres up front)
_fwd('eres-affine', 'conv3', (2, 17, 16), 72, [FA(32)], (16, 16, 64), eres=2, oaff=2)
_fwd('eres-bf16-no-relu', 'conv3', (1, 13, 21), 16, [PL(32)], (16, 32, 32), eres=1, eres_store='bf16', eres_relu=False, oaff=2)
_fwd('eres-bf16-affine-1x1', 'conv1', (2, 9, 7), 72, [PL(64)], (8, 64, 64), eres=2, eres_store='bf16', bias=True)
_fwd('out-f16', 'conv3', (1, 13, 21), 72, [PL(32)], (16, 16, 64), out_f16=True, bias=True)
_fwd('out-f16-T4', 'convT4', (2, 9, 7), 16, [FA(32)], (8, 32, 64), out_f16=True, oaff=2)
_fwd('stats', 'conv3', (2, 17, 16), 72, [PL(32)], (16, 16, 64), stats=True, out_f16=True, lattices=('LS',))
_fwd('stats-bias-ragged', 'conv3', (1, 13, 21), 16, [FA(32)], (16, 32, 32), stats=True, bias=True, lattices=('LS',))
_fwd('stats-T4', 'convT4', (2, 9, 7), 72, [PL(64)], (8, 64, 64), stats=True, lattices=('LS',))
_fwd('stats-1x1', 'conv1', (1, 33, 5), 8, [PL(64)], (16, 32, 128), stats=True, lattices=('LS',))
_fwd('stem-3-of-16', 'conv3', (1, 13, 21), 72, [PL(16, creal=3)], (16, 16, 64), bias=True)
_fwd('scaled-pack', 'conv3', (1, 13, 21), 72, [PL(32)], (16, 16, 32), scaled=True, oaff=1, orelu=True)
_fwd('slice', 'conv3', (1, 13, 21), 16, [PL(32)], (16, 16, 64), coff=8, cstride=40)
_fwd('relu-mode-2', 'conv3', (1, 13, 21), 16, [S(32, aff=True, relu=2)], (16, 16, 64))                 # (any non-zero relu is the ReLU)
_fwd('slice-T2', 'convT2', (2, 9, 7), 72, [PL(32)], (8, 32, 64), coff=16, cstride=96)


# ---- conv_ws_kernel (the older 16-bit persistent kernel): launches with statistics, or debug bit 128; it takes no grid cap -----------------------
def _ws_srcs(xf, C):
    return [(PL, FA, GA)[xf](C)]


for _bn in (64, 32):
    for _xf in (0, 1, 2):
        for _st in (0, 1):
            for _sm in (0, 1):
                _srcs = _ws_srcs(_xf, 128 if _sm else 64)
                if _sm and _xf == 2:
                    _srcs = [FR(64), GA(128, hs=30, ws=29, off=(1, 2))]          # twelve chunks across two sources, a residual, pad offsets
                _add('ws-bn%d-xf%d-st%d-sm%d' % (_bn, _xf, _st, _sm), '16', 'conv3', (2, 32, 32) if _bn == 64 else (1, 32, 48), _bn, _srcs, (16, 16, _bn),
                     form(WS, _bn, 9, _xf, _st, _sm), debug=PERSIST | (0 if _st else OLD_WS16), stats=bool(_st), bias=bool(_sm), oaff=0 if _st else 2,
                     orelu=not _st, lattices=('LS',) if _st else ('L0',))
# about 320 tiles of 16 x 16 at 64 channels: with 256 CUs workgroups run one and two tiles; and two output-channel tiles
_add('ws-320-tiles', '16', 'conv3', (5, 128, 128), 64, [PL(64)], (16, 16, 64), form(WS, 64, 9, 0, 1, 0), debug=PERSIST, stats=True, lattices=('LS',))
_add('ws-ctiles-2', '16', 'conv3', (3, 48, 64), 72, [PL(64)], (16, 16, 64), form(WS, 64, 9, 0, 1, 0), debug=PERSIST, stats=True, lattices=('LS',))


# ---- conv_ws16_kernel ------------------------------------------------------------------------------------------------------------------
def _w16(id, Cout, srcs, bn, xf, cap, kind='conv3', dbg=0, shape=(3, 32, 32), **f):
    fk = {k: f.pop(k) for k in ('stream', 'mix', 'ncs', 'site') if k in f}
    _add('ws16-' + id, '16', kind, shape, Cout, srcs, (16, 16, bn), form(WS16, bn, 9, xf, **fk), debug=PERSIST | dbg, persistent=True, cap=cap, **f)


for _bn in (64, 32):
    for _xf in (0, 2):
        _m = PL if _xf == 0 else (FA if _bn == 64 else GA)
        _p = 'bn%d-xf%d-' % (_bn, _xf)
        _big = 96 if _bn == 64 else 160                                   # streamed weights: beyond 82 KB of resident chunks
        _w16(_p + 'pair', _bn, [_m(64)], _bn, _xf, 1, site=1, bias=True, orelu=True)
        _w16(_p + 'quad', 48 if _bn == 64 else 16, [_m(64)], _bn, _xf, 2, dbg=QUAD, site=2, oaff=1)
        _w16(_p + 'pair-mix', _bn, [_m(64), _m(32)], _bn, _xf, 3, kind='mix', site=1, mix=1, oaff=1, orelu=True)
        _w16(_p + 'quad-mix', _bn, [_m(64), _m(64)], _bn, _xf, 5, kind='mix', dbg=QUAD, site=2, mix=1, bias=True)
        _w16(_p + 'k32', _bn, [_m(_big)], _bn, _xf, 2, site=3, stream=1, bias=True, oaff=1, orelu=True)
        _w16(_p + 'k32-two-src', 16 if _bn == 32 else 80, [_m(_big - 32), PL(32, hs=30, ws=27, off=(2, 3))], _bn, 2 if _xf else 0, 5, site=3, stream=1)
        _w16(_p + 'ncs1', _bn, [_m(16)], _bn, _xf, 3, ncs=1, oaff=1, orelu=True)
        _w16(_p + 'ncs2-32ch', 48, [_m(32)], _bn, _xf, 1, ncs=2, bias=True)
        _w16(_p + 'ncs2-48ch', 16, [_m(48)], _bn, _xf, 5, ncs=2)
        # the direct-store form with four or more resident chunks: an odd chunk count (BN 32: five chunks stay resident) or an odd n0
        _w16(_p + 'direct', _bn, [_m(80)] if _bn == 32 else [_m(16), _m(48)], _bn, _xf, 2, ncs=0, orelu=True)
        _w16(_p + 'direct-mix', _bn, [_m(64), _m(16)], _bn, _xf, 1, kind='mix', mix=1, ncs=0, oaff=1)
        _w16(_p + 'direct-stream', _bn, [_m(16), _m(_big - 16)], _bn, _xf, 3, stream=1, ncs=0, bias=True)
_w16('pad-chunk-pair', 32, [PL(64), PL(16)], 32, 0, 2, site=1, pad_chunks=1, bias=True)                       # nchunk = real + 1, resident
_w16('pad-chunk-k32', 64, [PL(64), PL(16, hs=31, ws=30, off=(1, 1))], 64, 0, 3, site=3, stream=1, pad_chunks=1)  # ... and streamed
_w16('pool-out-pair', 64, [PL(64)], 64, 0, 2, site=1, pool_out=True, orelu=True, oaff=1)
_w16('pool-out-quad-xf2', 48, [FA(64)], 64, 2, 1, dbg=QUAD, site=2, pool_out=True, orelu=True, bias=True)
_w16('pool-out-k32', 32, [GA(160)], 32, 2, 5, site=3, stream=1, pool_out=True, orelu=True)
_w16('slice-pair', 16, [PL(64)], 64, 0, 3, site=1, coff=24, cstride=48)
_w16('slice-direct', 48, [FA(48)], 64, 2, 2, ncs=2, coff=8, cstride=64)
_w16('ctiles-3', 144, [PL(64)], 64, 0, 5, site=1, bias=True, orelu=True)
_w16('relu-mode-2', 64, [S(64, aff=True, relu=2)], 64, 2, 2, site=1)
_w16('bwd3-pair', 64, [PL(64)], 64, 0, 1, kind='bwd3', site=1)
_w16('bwdT4-views', 32, [PL(32)], 32, 0, 2, kind='bwdT4', site=1, shape=(2, 16, 32))                           # two row-parity views, 2 + 2 chunks


# ---- conv_f32_kernel: its three (tile, BN) keys for taps 9, 4 and 1 (debug bits 32 and 256 keep the other fp32 kernels away) ---------------------
_F32_KEYS = [(16, 16, 64), (16, 16, 32), (8, 16, 64)]
_PLAIN32 = ('L0', 'L1', 'L2')


def _f32(id, kind, shape, Cout, srcs, key, dbg=0, **kw):
    _add('f32-' + id, '32', kind, shape, Cout, srcs, key, form(F32K, key[2], KINDS[kind][0], tile=key[0]), debug=ONE_TILE | NO_STREAM | dbg, **kw)


for _ti, _taps in enumerate((9, 4, 1)):
    for _i, _key in enumerate(_F32_KEYS):
        _kind = _TAP_KINDS[_taps][(_i + _ti) % 3]
        _sh = (_SH16 if _key[0] == 16 else _SH8)[(_i + _ti) % 3]
        _f32('%s-t%d-bn%d' % (_kind, _key[0], _key[2]), _kind, _sh, 32 if _kind[:3] == 'bwd' else _COUTS[(_i + _ti) % 3], [PL(32 if _i else 64)], _key,
             bias=bool(_i & 1), oaff=(_i + _ti) % 3, orelu=bool(_ti & 1), lattices=_PLAIN32)
_f32('full-tiles', 'conv3', (2, 32, 16), 64, [PL(64)], (16, 16, 64), bias=True, oaff=2, lattices=_PLAIN32)           # the full-tile epilogue
_f32('full-tiles-general', 'conv3', (2, 32, 16), 64, [PL(64)], (16, 16, 64), dbg=16, bias=True, oaff=2, lattices=_PLAIN32)
_f32('full-tiles-eres', 'conv3', (1, 16, 32), 64, [BR(32)], (16, 16, 64), eres=2, oaff=2)
_f32('full-tiles-eres-general', 'conv3', (1, 16, 32), 64, [BR(32)], (16, 16, 64), dbg=16, eres=2, oaff=2)
_f32('eres-ragged', 'conv3', (1, 13, 21), 72, [PL(32)], (16, 16, 64), eres=1, bias=True)
_f32('eres-1x1-no-relu', 'conv1', (2, 9, 7), 16, [GA(32)], (8, 16, 64), eres=2, eres_relu=False)
_f32('stats-full', 'conv3', (2, 32, 16), 64, [PL(32)], (16, 16, 64), stats=True, lattices=('LS',))
_f32('stats-full-general', 'conv3', (2, 32, 16), 64, [PL(32)], (16, 16, 64), dbg=16, stats=True, lattices=('LS',))
_f32('stats-ragged', 'conv3', (1, 13, 21), 72, [BR(32)], (16, 16, 32), stats=True, bias=True, lattices=('LS',))
_f32('stats-T4', 'convT4', (2, 9, 7), 16, [PL(32)], (8, 16, 64), stats=True, lattices=('LS',))
_f32('two-src-offsets', 'conv3', (1, 13, 21), 72, [PL(16), GA(32, hs=10, ws=17, off=(2, 3))], (16, 16, 64), bias=True)
_f32('residual', 'conv3', (2, 17, 16), 16, [S(32, aff=True, relu=True, res=True)], (16, 16, 32), oaff=2, orelu=True)
_f32('relu-only-T2', 'convT2', (2, 9, 7), 72, [GR(32)], (8, 16, 64))
_f32('T4-two-src', 'convT4', (1, 13, 21), 16, [PL(16), BR(16)], (16, 16, 32), lattices=('L0',))
_f32('bwd1', 'bwd1', (1, 33, 5), 32, [PL(48)], (16, 16, 32), lattices=_PLAIN32)
_f32('parity-views-T4', 'bwdT4', (1, 13, 21), 32, [PL(32)], (16, 16, 32), lattices=_PLAIN32)
_f32('parity-views-T2', 'bwdT2', (2, 9, 7), 64, [PL(32)], (8, 16, 64), lattices=_PLAIN32)
_f32('slice', 'conv3', (1, 13, 21), 16, [PL(32)], (16, 16, 32), coff=8, cstride=40)
_f32('256-channels', 'conv3', (1, 16, 16), 32, [PL(256)], (16, 16, 32), lattices=('L1', 'L2'))                       # 9 x 256 terms

# ---- conv1x1_f32_stream_kernel: BN 64 / 32 x NCH 1 / 2 / 4 x XF x ERES; every row also on conv_f32_kernel (debug bit 256) --------------------------
# pixel counts 31, 32, 33 (one block of 32 pixels minus one, exactly, plus one) and 259 (eight blocks and a tail of 3)
_PIX = [(1, 1, 31), (1, 4, 8), (1, 3, 11), (1, 7, 37)]
_n = 0
for _bn in (64, 32):
    for _nch in (1, 2, 4):
        for _xf in (0, 1):
            for _er in (0, 1):
                _src = (PL, GA if _n % 2 else BR)[_xf](16 * _nch)
                _co = (_bn, _bn + 8, 16)[_n % 3]
                _kw = dict(eres=1 + _n % 2, eres_relu=bool(_n % 3)) if _er else dict(orelu=bool(_n % 2))
                _lat = _PLAIN32 if not _xf else ('L0',)
                for _dbg, _f, _tag in ((0, form(STREAM, _bn, 1, _xf, nch=_nch, eres=_er), ''), (NO_STREAM, form(F32K, _bn, 1), '-on-f32')):
                    _add('s1x1-bn%d-nch%d-xf%d-er%d%s' % (_bn, _nch, _xf, _er, _tag), '32', 'conv1', _PIX[_n % 4], _co, [_src], (16, 16, _bn), _f, debug=_dbg,
                         bias=bool(_n % 2), oaff=(0, 2)[(_n // 2) % 2], lattices=_lat, **_kw)
                _n += 1
# a wave runs several blocks plus a tail: 393 132 pixels = 12 285 blocks of 32 and 12 pixels over the 4096 resident waves of 256 CUs
_add('s1x1-three-rounds', '32', 'conv1', (3, 362, 362), 32, [PL(16)], (16, 16, 32), form(STREAM, 32, 1, 0, nch=1), bias=True, lattices=('L1',))
_add('s1x1-slice', '32', 'conv1', (1, 7, 37), 16, [PL(32)], (16, 16, 32), form(STREAM, 32, 1, 0, nch=2), coff=8, cstride=40)
# no instantiation: a ReLU without scale / shift, three chunks - these must fall back to conv_f32_kernel
_add('s1x1-fallback-relu-only', '32', 'conv1', (1, 3, 11), 64, [GR(32)], (16, 16, 64), form(F32K, 64, 1))
_add('s1x1-fallback-3-chunks', '32', 'conv1', (1, 7, 37), 32, [PL(48)], (16, 16, 32), form(F32K, 32, 1), lattices=_PLAIN32)
_add('s1x1-fallback-offset', '32', 'conv1', (1, 7, 37), 64, [PL(32, hs=6, ws=30, off=(1, 2))], (16, 16, 64), form(F32K, 64, 1))


# ---- conv_ws32_kernel ------------------------------------------------------------------------------------------------------------------
def _w32(id, Cout, srcs, bn, xf, cap, kind='conv3', shape=(3, 32, 32), **f):
    fk = {k: f.pop(k) for k in ('stats', 'mix', 'ncs', 'site') if k in f}
    _add('ws32-' + id, '32', kind, shape, Cout, srcs, (16, 16, bn), form(WS32, bn, 9, xf, **fk), debug=PERSIST, persistent=True, cap=cap,
         stats=bool(fk.get('stats')), **f)


_CAPS = (1, 2, 3, 5)
_n = 0
for _bn in (64, 32):
    for _xf in (0, 1, 2):
        for _st in (0, 1):
            _srcs = [(PL, BR, GA)[_xf](64)]
            if _xf == 2 and _st:
                _srcs = [S(64, aff=True, relu=True, res=True)]
            _w32('bn%d-xf%d-st%d' % (_bn, _xf, _st), (_bn, _bn + 8, 16)[_n % 3], _srcs, _bn, _xf, _CAPS[_n % 4], stats=_st, bias=bool(_n % 2),
                 oaff=0 if _st else 2, orelu=not _st, lattices=('LS',) if _st else (_PLAIN32 if _xf == 0 else ('L0',)))
            _n += 1
for _ncs, _c in ((1, 16), (2, 32), (2, 48)):
    for _xf in (0, 1):
        for _st in (0, 1):
            if _c == 48 and _xf != _st:
                continue
            _w32('ncs%d-%dch-xf%d-st%d' % (_ncs, _c, _xf, _st), (64, 72, 16)[_n % 3], [(PL, BR)[_xf](_c)], 64, _xf, _CAPS[_n % 4], stats=_st, ncs=_ncs,
                 bias=bool(_n % 2), oaff=0 if _st else 1, lattices=('LS',) if _st else (_PLAIN32 if _xf == 0 else ('L0',)))
            _n += 1
for _bn in (64, 32):
    _w32('mix-bn%d-xf0' % _bn, _bn, [PL(64), PL(16)], _bn, 0, 3, kind='mix', mix=1, site=2, oaff=1, orelu=True, scaled=True, lattices=_PLAIN32)
    _w32('mix-bn%d-xf1-as-2' % _bn, _bn, [BR(64), BR(32)], _bn, 2, 2, kind='mix', mix=1, site=2, bias=True)
_w32('pool', 64, [PL(64)], 64, 0, 3, site=3, pool_out=True, orelu=True, oaff=2, lattices=_PLAIN32)                     # (oscale of both signs)
_w32('pool-128ch-2-ctiles', 128, [PL(128)], 64, 0, 5, site=3, pool_out=True, orelu=True, bias=True, shape=(1, 32, 32))
_w32('two-src-offsets', 72, [BR(64), BR(32, hs=29, ws=28, off=(1, 2))], 64, 1, 2, bias=True)
_w32('two-src-stats', 32, [PL(64), GA(16)], 32, 2, 5, stats=1, lattices=('LS',))
_w32('relu-mode-2', 64, [S(64, aff=True, relu=2)], 64, 2, 3)                                                         # (fast means relu == 1: generic)
_w32('slice', 32, [PL(64)], 32, 0, 3, coff=16, cstride=64, lattices=_PLAIN32)
_w32('bwdT4-views', 64, [PL(32)], 64, 0, 2, kind='bwdT4', shape=(2, 16, 32), lattices=_PLAIN32)
_w32('256-channels', 64, [PL(256)], 64, 0, 1, shape=(1, 16, 32), lattices=('L1', 'L2'))

ROW_BY_ID = {r.id: r for r in ROWS}


def runs():
    return [(r, lat) for r in ROWS for lat in r.lattices]


def table_forms():
    return {r.form for r in ROWS}


# every form a launcher can record (the launch sites of launch_conv, try_launch_conv_ws, try_launch_ws16, launch_conv32,
# launch_conv1x1_stream, try_launch_ws32)
REACHABLE = {form(FWD, k[2], t, tile=k[0], ck=k[1]) for k in _FWD_KEYS for t in (9, 4, 1)}
REACHABLE |= {form(WS, bn, 9, xf, st, sm) for bn in (64, 32) for xf in (0, 1, 2) for st in (0, 1) for sm in (0, 1)}
for _bn in (64, 32):
    for _xf in (0, 2):
        REACHABLE |= {form(WS16, _bn, 9, _xf, site=3, stream=1), form(WS16, _bn, 9, _xf, site=2), form(WS16, _bn, 9, _xf, site=2, mix=1),
                      form(WS16, _bn, 9, _xf, site=1), form(WS16, _bn, 9, _xf, site=1, mix=1), form(WS16, _bn, 9, _xf, ncs=1), form(WS16, _bn, 9, _xf, ncs=2),
                      form(WS16, _bn, 9, _xf), form(WS16, _bn, 9, _xf, mix=1), form(WS16, _bn, 9, _xf, stream=1)}
REACHABLE |= {form(F32K, k[2], t, tile=k[0]) for k in _F32_KEYS for t in (9, 4, 1)}
REACHABLE |= {form(STREAM, bn, 1, xf, nch=n, eres=e) for bn in (64, 32) for n in (1, 2, 4) for xf in (0, 1) for e in (0, 1)}
REACHABLE |= {form(WS32, bn, 9, xf, st) for bn in (64, 32) for xf in (0, 1, 2) for st in (0, 1)}
REACHABLE |= {form(WS32, 64, 9, xf, st, ncs=n) for xf in (0, 1) for st in (0, 1) for n in (1, 2)}
REACHABLE |= {form(WS32, bn, 9, xf, mix=1, site=2) for bn in (64, 32) for xf in (0, 2)} | {form(WS32, 64, 9, 0, site=3)}
REACHABLE |= {form(WS32, 64, 9, xf, site=1) for xf in (0, 1, 2)}
NOT_COVERED = {form(WS32, 64, 9, xf, site=1): 'conv_ws32_kernel(bns) XF %d: the BatchNorm-backward sums (ws = 2) are real-valued, not lattice-exact; '
               'test_gpu_fp32_kernels.py::test_conv_ws32_bn_backward_statistics_epilogue' % xf for xf in (0, 1, 2)}


# ---- data ------------------------------------------------------------------------------------------------------------------------------
def unit(lattice):
    return {'L0': 0.5, 'L1': 2.0 ** -8, 'L2': 2.0 ** -8, 'LS': 1.0}[lattice]


def out_hw(row):
    N, H, W = row.shape
    o = 2 if KINDS[row.kind][1] else 1
    return H * o, W * o


def weight_shapes(row):
    """torch-layout shapes of the layer's weight tensors (mix: the 3x3 and the 1x1 one)"""
    Cs = [s.creal or s.C for s in row.srcs]
    cin, co = sum(Cs), row.Cout
    k = {'conv3': 3, 'conv1': 1, 'convT4': 4, 'convT2': 2, 'bwd3': 3, 'bwd1': 1, 'bwdT4': 4, 'bwdT2': 2}.get(row.kind)
    if row.kind == 'mix':
        return [(co, Cs[0], 3, 3), (co, Cs[1], 1, 1)]
    if row.kind in ('conv3', 'conv1'):
        return [(co, cin, k, k)]
    if row.kind in ('convT4', 'convT2'):
        return [(cin, co, k, k)]
    if row.kind in ('bwd3', 'bwd1'):
        return [(cin, co, k, k)]                 # the forward Conv2d's [out_channels][in_channels]: the gradient has `cin` channels
    return [(co, cin // 2, k, k)]                # the ConvTranspose2d's [in_channels][out_channels]; a view holds 2 x out_channels


def make_data(row, lattice):
    """stored tensors of a row as float64 torch tensors: src = [dict(x, scale, shift, res)] (NCHW; bwdT*: one entry, the full-resolution
    gradient), w = weight tensors in the torch layout, the epilogue's vectors and the eres tensor"""
    rng = np.random.default_rng(zlib.crc32((row.id + lattice).encode()))
    N, H, W = row.shape
    t64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    ints = lambda shape, lo=-3, hi=3: rng.integers(lo, hi + 1, size=shape).astype(np.float64)
    fine = lambda shape: rng.integers(-1024, 1024, size=shape).astype(np.float64) / 256.0
    sparse = lambda shape: rng.integers(-1, 2, size=shape).astype(np.float64) * (rng.random(shape) < 0.375)       # non-zero at density 1/4
    pm = lambda n: rng.choice([1.0, -1.0, 2.0, -2.0, 0.5], size=n)
    xgen = {'L0': ints, 'L1': fine, 'L2': ints, 'LS': sparse}[lattice]
    wgen = {'L0': ints, 'L1': ints, 'L2': fine, 'LS': sparse}[lattice]
    srcs = []
    for s in row.srcs:
        if row.kind in ('bwdT4', 'bwdT2'):
            shp = (N, s.C // 2, 2 * H, 2 * W)
        else:
            shp = (N, s.C) + tuple(wc.stored_hw(row, s))
        assert lattice in ('L0', 'LS') or not (s.aff or s.relu or s.res or s.pool), 'L1 / L2 are lattices of plain sources'
        x = xgen(shp)
        if lattice == 'L0':
            x[(x == 0) & (rng.random(shp) < 0.5)] = -0.0
        d = dict(x=t64(x), scale=None, shift=None, res=None)
        if s.aff:
            sh = ints((s.C,), -2, 2) if lattice != 'LS' else ints((s.C,), -1, 1)
            sh[(sh == 0) & (rng.random(s.C) < 0.5)] = -0.0
            d['scale'], d['shift'] = t64(pm(s.C) if lattice != 'LS' else rng.choice([1.0, -1.0], size=s.C)), t64(sh)
        if s.res:
            d['res'] = t64(xgen(shp))
        srcs.append(d)
    Ho, Wo = out_hw(row)
    co = row.Cout
    out = dict(src=srcs, w=[t64(wgen(shp)) for shp in weight_shapes(row)], lattice=lattice, bias=None, oscale=None, oshift=None, eres=None,
               eres_scale=None, eres_shift=None, cout_scale=None)
    if row.bias:
        out['bias'] = t64(ints((co,)))
    if row.oaff:
        out['oshift'] = t64(ints((co,), -2, 2))
    if row.oaff == 2:
        out['oscale'] = t64(pm(co))
    if row.eres:
        out['eres'] = t64(ints((N, co, Ho, Wo)))
    if row.eres == 2:
        out['eres_scale'], out['eres_shift'] = t64(pm(co)), t64(ints((co,), -2, 2))
    if row.scaled:
        out['cout_scale'] = t64(rng.choice([1.0, 2.0, -1.0, -2.0, 4.0, -4.0], size=co))
    return out


# ---- float64 reference -----------------------------------------------------------------------------------------------------------------
def conv_taps(kind, A, Wt):
    """the layer from its definition, tap by tap, float64.  A [N][C][H][W] logical input (bwd*: the output gradient), Wt the torch-layout weight"""
    N, C, H, W = A.shape
    e = torch.einsum
    if kind in ('conv3', 'conv1'):               # y[p] = sum w[k] x[p + k - pad]
        k = Wt.shape[2]
        Ap = F.pad(A, (k // 2,) * 4)
        return sum(e('nchw,oc->nohw', Ap[:, :, ky:ky + H, kx:kx + W], Wt[:, :, ky, kx]) for ky in range(k) for kx in range(k))
    if kind == 'convT4':                         # x[i] lands on y[2 i - 1 + k]
        out = torch.zeros((N, Wt.shape[1], 2 * H + 2, 2 * W + 2), dtype=torch.float64)
        for ky in range(4):
            for kx in range(4):
                out[:, :, ky:ky + 2 * H:2, kx:kx + 2 * W:2] += e('nchw,co->nohw', A, Wt[:, :, ky, kx])
        return out[:, :, 1:-1, 1:-1]
    if kind == 'convT2':                         # x[i] lands on y[2 i + k]
        out = torch.zeros((N, Wt.shape[1], 2 * H, 2 * W), dtype=torch.float64)
        for ky in range(2):
            for kx in range(2):
                out[:, :, ky::2, kx::2] = e('nchw,co->nohw', A, Wt[:, :, ky, kx])
        return out
    if kind in ('bwd3', 'bwd1'):                 # dx[p] = sum w[k] dy[p - k + pad]
        k = Wt.shape[2]
        Ap = F.pad(A, (k // 2,) * 4)
        return sum(e('nohw,oc->nchw', Ap[:, :, k - 1 - ky:k - 1 - ky + H, k - 1 - kx:k - 1 - kx + W], Wt[:, :, ky, kx]) for ky in range(k) for kx in range(k))
    Hh, Wh = H // 2, W // 2
    if kind == 'bwdT4':                          # dx[i] = sum w[k] dy[2 i - 1 + k]
        Ap = F.pad(A, (1,) * 4)
        return sum(e('nohw,co->nchw', Ap[:, :, ky:ky + 2 * Hh:2, kx:kx + 2 * Wh:2], Wt[:, :, ky, kx]) for ky in range(4) for kx in range(4))
    assert kind == 'bwdT2'                       # dx[i] = sum w[k] dy[2 i + k]
    return sum(e('nohw,co->nchw', A[:, :, ky::2, kx::2], Wt[:, :, ky, kx]) for ky in range(2) for kx in range(2))


def stored_weights(row, data):
    """the weights over the STORED channels (padded input channels: zeros), channel scales of the scaled pack applied (only the first
    tensor of a mix row carries them: the BatchNorm fold of the 3x3 branch)"""
    out = []
    for i, w in enumerate(data['w']):
        if any(s.creal for s in row.srcs):
            assert row.kind in ('conv3', 'conv1') and len(row.srcs) == 1
            w = F.pad(w, (0, 0, 0, 0, 0, row.srcs[0].C - w.shape[1]))
        if data['cout_scale'] is not None and i == 0:
            assert row.kind in ('conv3', 'conv1', 'mix')
            w = w * data['cout_scale'].view(-1, 1, 1, 1)
        out.append(w)
    return out


def logical_inputs(row, data):
    """per weight tensor the float64 tensor it is applied to"""
    r = wc.rounded(dict(src=data['src'], g=torch.zeros(1, dtype=torch.float64), lattice=data['lattice']), row, row.prec)
    if row.kind in ('bwdT4', 'bwdT2'):
        return [r['src'][0]['x']]
    if row.kind == 'mix':
        return [wc.logical_input(_One(row, i), dict(src=[r['src'][i]]), row.prec) for i in (0, 1)]
    return [wc.logical_input(row, r, row.prec)]


class _One:
    """one source of a row as a layer of its own (for wc.logical_input)"""

    def __init__(self, row, i):
        self.shape, self.kind, self.srcs = row.shape, row.kind, [row.srcs[i]]


def accumulators(row, data):
    """(acc, sum |a * w|): the bias-free accumulators [N][Cout][Ho][Wo], float64"""
    kinds = ['conv3', 'conv1'] if row.kind == 'mix' else [row.kind]
    A, Ws = logical_inputs(row, data), stored_weights(row, data)
    acc = sum(conv_taps(k, a, w) for k, a, w in zip(kinds, A, Ws))
    sabs = sum(conv_taps(k, a.abs(), w.abs()) for k, a, w in zip(kinds, A, Ws))
    return acc, sabs


def out_dtype(row):
    return torch.float32 if row.prec == '32' else (torch.float16 if row.out_f16 else torch.bfloat16)


def epilogue(row, data, acc):
    """list of the epilogue's intermediates, float64, the last one the value before the store's rounding"""
    v = lambda t: t.view(1, -1, 1, 1)
    steps = []
    x = acc
    if data['bias'] is not None:
        x = x + v(data['bias']); steps.append(x)
    if data['oscale'] is not None:
        x = x * v(data['oscale']); steps.append(x)
    if data['oshift'] is not None:
        x = x + v(data['oshift']); steps.append(x)
    if row.orelu:
        x = x.clamp_min(0.0)
    if data['eres'] is not None:
        if row.prec == '16':
            x = x.float().half().double()        # the convolution's result is staged in fp16
        e = data['eres']
        if data['eres_scale'] is not None:
            e = e * v(data['eres_scale']) + v(data['eres_shift']); steps.append(e)
        x = e + x; steps.append(x)
        if row.eres_relu:
            x = x.clamp_min(0.0)
    steps.append(x)
    return steps


def reference(row, data):
    """dict(acc, sabs, steps, out [N][Ho][Wo][Cout] in the output's type, pool [N][Ho/2][Wo/2][Cout] or None, ssum / ssq [Cout] float64)"""
    acc, sabs = accumulators(row, data)
    steps = epilogue(row, data, acc)
    out = steps[-1].float().to(out_dtype(row))                      # float64 -> float32 is exact (guard), then nearest-even
    pool = F.max_pool2d(out.double(), 2).to(out.dtype).permute(0, 2, 3, 1).contiguous() if row.pool_out else None
    return dict(acc=acc, sabs=sabs, steps=steps, out=out.permute(0, 2, 3, 1).contiguous(), pool=pool, ssum=acc.sum((0, 2, 3)), ssq=(acc * acc).sum((0, 2, 3)))


def guard(row, data, ref):
    """the exact regime, from the reference alone: stored values exact in their types, sum |a * w| per output element below 2^24 units,
    every accumulator and epilogue intermediate a whole number of (quarter) units below 2^24 of them, the final value an fp32 number;
    rows with statistics: the per-channel sum |acc| and sum acc^2 below 2^24 units / squared units"""
    u = unit(data['lattice'])
    whole = lambda t, q: torch.equal(t / q, torch.round(t / q)) and float(t.abs().max()) / q < 2.0 ** 24
    assert float(ref['sabs'].max()) / u < 2.0 ** 24, (row.id, float(ref['sabs'].max()) / u)
    assert whole(ref['acc'], u), row.id
    for t in ref['steps']:
        assert whole(t, u / 4), row.id
    assert torch.equal(ref['steps'][-1].float().double(), ref['steps'][-1]), row.id
    r = wc.rounded(dict(src=data['src'], g=torch.zeros(1, dtype=torch.float64), lattice=data['lattice']), row, row.prec)
    for s, d0, d1 in zip(row.srcs, data['src'], r['src']):
        assert torch.equal(d0['x'], d1['x']) and (d0['res'] is None or torch.equal(d0['res'], d1['res'])), row.id              # stored exactly
        t = d0['x'] * (1.0 if d0['scale'] is None else d0['scale'].view(1, -1, 1, 1)) + (0.0 if d0['shift'] is None else d0['shift'].view(1, -1, 1, 1))
        t = t + (0.0 if d0['res'] is None else d0['res'])
        if row.prec == '16':
            assert torch.equal(t.bfloat16().double(), t) and torch.equal(t.half().double(), t), row.id
    wdt = torch.bfloat16 if row.prec == '16' else torch.float32
    for w in stored_weights(row, data):
        assert torch.equal(w.to(wdt).double(), w), row.id
        if row.prec == '32':                     # the split pack: hi + lo must hold the weight exactly
            hi = w.bfloat16().double()
            assert torch.equal((w - hi).bfloat16().double(), w - hi), row.id
    if data['eres'] is not None:
        edt = torch.float32 if row.prec == '32' else (torch.float16 if row.eres_store == 'fp16' else torch.bfloat16)
        assert torch.equal(data['eres'].to(edt).double(), data['eres']), row.id
    if row.stats:
        assert float(ref['acc'].abs().sum((0, 2, 3)).max()) / u < 2.0 ** 24 and float(ref['ssq'].max()) / (u * u) < 2.0 ** 24, (row.id, float(ref['ssq'].max()) / (u * u))


# ---- device side -----------------------------------------------------------------------------------------------------------------------
class OutBuffer:
    """an NHWC output [N][H][W][cstride] inside a larger sentinel-filled buffer"""

    def __init__(self, shape, dtype):
        self.shape, self.n, self.dtype = tuple(shape), int(np.prod(shape)), dtype
        self.buf = torch.full((self.n + 2 * SLACK,), SENTINEL, dtype=dtype, device='cuda')
        self.t = self.buf[SLACK:SLACK + self.n].view(self.shape)

    def read(self):
        """(the tensor on the host, True if the slack on both ends still holds the sentinel)"""
        h = self.buf.cpu()
        s = torch.full((SLACK,), SENTINEL, dtype=self.dtype)
        return h[SLACK:SLACK + self.n].view(self.shape), torch.equal(h[:SLACK], s) and torch.equal(h[SLACK + self.n:], s)


def device_args(row, data):
    """the launch's device tensors, built once per (row, lattice): dict(srcs, wp, kw) for engine.conv_forward"""
    from cdnet_amd import engine
    taps, transposed, mode = KINDS[row.kind]
    N, H, W = row.shape
    f32 = row.prec == '32'
    dev = lambda v: None if v is None else v.float().cuda()
    srcs = []
    if row.kind in ('bwdT4', 'bwdT2'):
        Ct = row.srcs[0].C // 2
        gy = wc._nhwc(data['src'][0]['x'], wc.store_dtype(row.srcs[0], row.prec))
        srcs = [engine.Src(gy, view=(a * 2 * W * Ct, H, W, 2 * Ct, 4 * W * Ct)) for a in (0, 1)]
    else:
        for s, d in zip(row.srcs, data['src']):
            dt = wc.store_dtype(s, row.prec)
            srcs.append(engine.Src(wc._nhwc(d['x'], dt), dev(d['scale']), dev(d['shift']), relu=s.relu, pool=s.pool,
                                   res=None if d['res'] is None else wc._nhwc(d['res'], dt), off=s.off))
    packs = []
    for i, w in enumerate(data['w']):
        cin_pad = None
        if any(s.creal for s in row.srcs):
            cin_pad = row.srcs[0].C
        if row.pad_chunks:
            cin_pad = w.shape[1] + 16 * row.pad_chunks           # the padding chunk's weights: zeros
        packs.append(engine.pack_weights(w.float().cuda().contiguous(), row.cfg, mode, Cin_pad=cin_pad, split=f32,
                                         cout_scale=dev(data['cout_scale']) if i == 0 else None))
    kw = dict(taps=taps, transposed=transposed, bias=dev(data['bias']), oscale=dev(data['oscale']), oshift=dev(data['oshift']), orelu=row.orelu,
              H=H, W=W, taps1=1 if row.kind == 'mix' else 0, pad_chunks=row.pad_chunks, out_coff=row.coff)
    if data['eres'] is not None:
        edt = torch.float32 if f32 else (torch.float16 if row.eres_store == 'fp16' else torch.bfloat16)
        kw['eres'] = engine.Src(wc._nhwc(data['eres'], edt), dev(data['eres_scale']), dev(data['eres_shift']), relu=row.eres_relu)
    return dict(srcs=srcs, wp=packs[0] if len(packs) == 1 else torch.cat(packs), kw=kw)


def stats_rows(row):
    N, H, W = row.shape
    t = row.cfg[0]
    return N * (4 if KINDS[row.kind][1] else 1) * (-(-H // t)) * (-(-W // t))


def make_buffers(row):
    """the launch's outputs before it: out and pool_out filled with the sentinel, the statistics rows with NaN"""
    N, H, W = row.shape
    Ho, Wo = out_hw(row)
    return dict(out=OutBuffer((N, Ho, Wo, row.cstride or row.Cout), out_dtype(row)),
                pool=OutBuffer((N, Ho // 2, Wo // 2, row.Cout), out_dtype(row)) if row.pool_out else None,
                stats=torch.full((stats_rows(row), 2, row.Cout), float('nan'), dtype=torch.float32, device='cuda') if row.stats else None)


def launch(row, dargs, debug, bufs=None):
    """one cdnet_conv_forward through engine.conv_forward with `debug` for this launch alone; returns dict(form, out (OutBuffer), pool, stats)"""
    from cdnet_amd import _lib, engine
    b = bufs or make_buffers(row)
    engine.conv_forward(dargs['srcs'], dargs['wp'], row.Cout, row.cfg, out=b['out'].t, stats=b['stats'], pool_out=None if b['pool'] is None else b['pool'].t,
                        debug_or=debug, **dargs['kw'])
    torch.cuda.synchronize()
    return dict(b, form=_lib.load().cdnet_conv_forward_last_form())
