"""Rows, data families, the float64 reference, the guard and the derived bounds of the exact per-element tests of csrc/dam_loss.hip,
csrc/mask_loss.hip and csrc/loss_util.h, shared by test_loss_refs_cpu.py (which pins the reference to float64 autograd of the oracle,
runs the guard and the coverage assertions, holds an fp32 emulation of the kernels inside every bound and shows that the rows catch
twelve wrong variants) and test_gpu_loss_exact.py.

Reference (numpy float64, no autograd; `reference`), from the fp32 logits and the u8 / f16 targets, after train_util_dam.py:123-142,
167-276, 499-580 as restated in oracle/train.py.  p = softmax(mask), q = softmax(direction), w = weight / 20 (1 with WMAP clear).
  loss (`dam`, LossLay<ND>'s order): I_c = sum p_c [label = c], P_c = sum p_c, T_c = sum [label = c]; Pw_i = sum w q_i, Tw_j = sum w t_j,
      SS_j = sum w q_j t_j, SN_j = sum w q_next(j) t_j, SP_j = sum w q_prev(j) t_j (j >= 1, next / prev cyclic over 1 .. ND-1); ce, dce,
      mse; tp, fp, fn of (first arg-max of the direction logits = 1) against (direction class = 1).  t is the one-hot of the direction
      class where the label of SAMPLE 0 (quirk) or of the sample itself is foreground; a sample whose direction map is constant - at any
      class - has t = channel 0 everywhere (:141, the `single` flag).
      coef per sample: alpha_c = -2 / (B (P_c + T_c + 1)), beta_c = 2 (I_c + 1) / (B (P_c + T_c + 1)^2); bsum_i, a_self_j, a_next_j, a_prev_j
      the same two expressions over (SS_j, Pw_j + Tw_j), (SN_j, Pw_next(j) + Tw_j), (SP_j, Pw_prev(j) + Tw_j), class 0 doubled with WMAP.
      losses: total, dce, wdice, mse, ce, dice, then accuracy, IoU, recall, precision, F1 (utils.py:67-110, mean over the samples).
      dmask = p_c (g_c - sum p g) + [CE] w (p_c - [label = c]) / (B P), g_c = beta_c + [label = c] alpha_c;
      ddir  = q_c (h_c - sum q h) + w (q_c - [dir = c]) / (B P), h_c = (bsum_c + a) (w / ND with WMAP), a = a_self / a_next / a_prev of the
      pixel's target j for c = j / next(j) / prev(j);  dpoint = 2 (point - target) / (B P).
  `mask`: the nine mask sums, ce, tp / fp / fn of the mask arg-max; alpha, beta; total, ce, dice, five metrics; dmask by term word.
  `val` (ValLay<ND>'s order): I, P, T, sum -log p_label; Iq, Pq, Tq over q' = q with q'_0 *= p_0 against the one-hot of lut[direction class]
      (none where the LUT holds -1) under SAMPLE 0's foreground; sum -w log q_dir; sum (point - target / 255)^2; tp, fp, fn of the mask arg-max.

Data families (`make_data`).  Label, direction class and weight are drawn independently per pixel, so every (label, direction) pair
occurs, a non-zero direction over background included; for B >= 2 the last sample is constant at direction class ND - 1, for B >= 3
sample B - 2 has label 0 everywhere; rows with spec 'bg0' have no foreground in sample 0.
  L  saturated: one logit 0, the rest -128.  expf(-128) is 0 in fp32: p is one-hot, log p in {0, -128}.  Weight bytes {20, 40, 60}, point
     logits and f16 targets multiples of 1/4 in [-2, 2].  The winning direction channel is drawn among t, next(t), prev(t) and another.
     Every sum is a sum of integers or multiples of 1/16 below 2^24 quanta: exact in fp32 in any order, compared with ==.
  T  ties: 1 or 2 (direction: 1, 2 or 4) logits 0, the rest -128: p in {1, 1/2, 1/4, 0}.  All sums but the cross-entropies stay exact; the
     first-maximum rule decides tp / fp / fn.
  R  random: logits randn * 2, weight bytes 0 .. 255, point randn, targets random f16.
  val rows carry a LUT: 'rank' (class 2 absent from the data, LUT[2] = -1, the later classes one channel down) or 'perm' (a permutation of
  the channels with one PRESENT class marked -1: its pixels have no target).

Bounds (derived, never tuned).  U = 2^-24, half an fp32 ulp.  The kernels are modelled once, in their own order of operations as built
with -ffp-contract=off (`model_dam`, `model_mask`, `model_val`), over an arithmetic `ops`: with `F32` the model is the fp32 emulation the
CPU test runs, with `V` it carries for every value a first-order running error bound: every fp32 +, -, *, fma adds U |result| to the
propagated errors of its operands - each rounding weighted by the magnitude it acts on, cancellation included; an operation whose
operands are exact and whose result is representable in fp32 adds nothing (that is what makes L and T exact); adding an exact 0 or
multiplying by an exact 0, +-1 or power of two adds nothing.  Constants:
  expf, logf, fp32 division: 2 ulp = 4 U of the result each.  ASSUMED: this ROCm install ships no HIP math accuracy table.  Also assumed: a
      division whose exact quotient is representable returns it, expf(0) = 1, expf(x <= -104) = 0, logf(1) = 0.
  one term of a sum (c_term): softmax argument l - m (1), expf (4, and the argument's error U |l - m| through the exponential), the sum
      over NC classes (NC - 1), the division (4), logf (4), w = byte / 20 (4), the product with w (1), each acting on its own magnitude,
      so c_term is evaluated per pixel by `V`, not as one constant.
  a sum (all terms of one sign): |got - want| <= n_add U sum |term| + sum err(term).  n_add is the longest chain of fp32 additions one term
      passes through: trips (pixels per thread, ceil(P / (nchunk TPB))) + TPB (row_sum's serial lane sum) + nchunk / 4 + nchunk % 4 + 2
      (chunk_sum's first chain, its tail and the two joining additions).  val_sums_reduce_kernel sums the chunks in double and casts
      once: trips + TPB + 1.  A sum whose terms are exact multiples of a quantum 2^-k, k <= 4, with sum |term| < 2^24 quanta is exact.
  coefficients, losses, gradients: the sums' bounds propagated by `V` through the kernels' expressions.
  pixel metrics: double arithmetic over exact counts, cast once: one U of the float64 value.
  Every bound is multiplied by 1 + 2^-10 for the second-order terms (the longest chain is below 400 operations, 400 U < 2^-15)."""
import ctypes as C
import dataclasses
import functools

import numpy as np

U32 = 2.0 ** -24
ULP_EXP = ULP_LOG = ULP_DIV = 2                # assumed (see the docstring)
HI = 1.0 + 2.0 ** -10
SENTINEL = -12345.678
SLACK = 64
WMAP, CE, DICE = 1, 2, 4
FULL = WMAP | CE | DICE
DAM_WORDS = (FULL, CE | DICE, WMAP | DICE, DICE)
f64, f32 = np.float64, np.float32


# ----------------------------------------------------------------------------------------------------------------------------------
# layouts (LossLay<ND>, ValLay<ND>, mask_loss.hip)
# ----------------------------------------------------------------------------------------------------------------------------------
class LossLay:
    def __init__(self, ND):
        self.ND, self.PW, self.TW, self.SS, self.SN, self.SP, self.SC = ND, 9, 9 + ND, 9 + 2 * ND, 9 + 3 * ND, 9 + 4 * ND, 9 + 5 * ND
        self.SUMS, self.COEF, self.TPB = self.SC + 6, 6 + 4 * ND, 128 if ND > 9 else 256

    def name(self, k):
        for base, n in ((self.SC, 'ce dce mse tp fp fn'.split()),):
            if k >= base:
                return n[k - base]
        for base, n in ((self.SP, 'SP'), (self.SN, 'SN'), (self.SS, 'SS'), (self.TW, 'Tw'), (self.PW, 'Pw'), (6, 'T'), (3, 'P'), (0, 'I')):
            if k >= base:
                return '%s_%d' % (n, k - base)


class ValLay:
    def __init__(self, ND):
        self.ND, self.IQ, self.PQ, self.TQ, self.VS = ND, 10, 10 + ND, 10 + 2 * ND, 10 + 3 * ND
        self.SUMS, self.TPB = self.VS + 5, 128 if ND > 9 else 256

    def name(self, k):
        if k >= self.VS:
            return 'dce mse tp fp fn'.split()[k - self.VS]
        for base, n in ((self.TQ, 'Tq'), (self.PQ, 'Pq'), (self.IQ, 'Iq')):
            if k >= base:
                return '%s_%d' % (n, k - base)
        return 'ce' if k == 9 else '%s_%d' % ('IPT'[k // 3], k % 3)


MS_SUMS, MS_COEF, MS_TPB = 13, 6, 256
MS_NAMES = ['I_0', 'I_1', 'I_2', 'P_0', 'P_1', 'P_2', 'T_0', 'T_1', 'T_2', 'ce', 'tp', 'fp', 'fn']


def loss_nchunk(P, tpb):
    return min(64, -(-P // (tpb * 8)))


def n_add(P, tpb, double_chunks=False):
    """the longest chain of fp32 additions behind one per-sample sum (docstring)"""
    nchunk = loss_nchunk(P, tpb)
    trips = -(-P // (nchunk * tpb))
    return trips + tpb + (1 if double_chunks else nchunk // 4 + nchunk % 4 + 2)


def nxt(i, ND, wrap=True):
    return (1 if wrap else 0) if i == ND - 1 else i + 1


def prv(i, ND, wrap=True):
    return (ND - 1 if wrap else 0) if i == 1 else i - 1


def ws_layout(entry, B, P, ND=9):
    """offsets in floats of the workspace's parts, as dam_loss_impl (partial | coef | sums | pad | single) and cdnet_mask_loss
    (partial | coef | pad) and the val sums (partial) lay them out, and the total"""
    if entry == 'dam':
        Y = LossLay(ND)
        nchunk = loss_nchunk(P, Y.TPB)
        lay = dict(nchunk=nchunk, partial=0, coef=B * nchunk * Y.SUMS)
        lay['sums'] = lay['coef'] + B * Y.COEF
        lay['pad'] = lay['sums'] + B * Y.SUMS
        lay['single'] = lay['pad'] + 16
        lay['total'] = lay['single'] + B
    elif entry == 'mask':
        nchunk = loss_nchunk(P, MS_TPB)
        lay = dict(nchunk=nchunk, partial=0, coef=B * nchunk * MS_SUMS)
        lay['pad'] = lay['coef'] + B * MS_COEF
        lay['total'] = lay['pad'] + 16
    else:
        Y = ValLay(ND)
        nchunk = loss_nchunk(P, Y.TPB)
        lay = dict(nchunk=nchunk, partial=0, total=B * nchunk * Y.SUMS)
    return lay


# ----------------------------------------------------------------------------------------------------------------------------------
# rows
# ----------------------------------------------------------------------------------------------------------------------------------
S1, S2, S3, S4, S5 = (1, 3, 5), (2, 24, 20), (3, 33, 31), (2, 96, 112), (64, 6, 8)
CAP9, CAP17 = (1, 384, 352), (1, 264, 256)


@dataclasses.dataclass(frozen=True)
class Row:
    entry: str                 # 'dam' | 'mask' | 'val'
    fam: str                   # 'L' | 'T' | 'R'
    shape: tuple
    ND: int = 9
    quirk: int = 1
    terms: int = FULL
    mis: bool = False          # label and direction pointers one byte into larger buffers
    spec: str = ''             # 'bg0': sample 0 has no foreground;  val rows: 'rank' | 'perm'
    seed: int = 0

    @property
    def id(self):
        s = '%s-%s-%dx%dx%d%s' % (self.entry, self.fam, *self.shape, 'm' if self.mis else '')
        if self.entry != 'mask':
            s += '-nd%d' % self.ND
        if self.entry == 'dam':
            s += '-q%d' % self.quirk
        if self.entry != 'val':
            s += '-t%d' % self.terms
        return s + ('-' + self.spec if self.spec else '')

    @property
    def P(self):
        return self.shape[1] * self.shape[2]


def _rows():
    rows = []
    small = [(S1, False), (S2, False), (S2, True), (S3, False), (S4, False), (S5, False)]
    for ni, ND in enumerate((5, 9, 17)):
        for si, (shape, mis) in enumerate(small):
            k = si + ni
            rows.append(Row('dam', 'LTR'[k % 3], shape, ND, k % 2, DAM_WORDS[(si + 2 * ni) % 4], mis))
        rows.append(Row('dam', 'R', CAP17 if ND == 17 else CAP9, ND, ni % 2, FULL))
    # what the cycle above leaves out: (ND, word), (ND, quirk), (family, ND) pairs, the full word for cdnet_dam_loss, no foreground in sample 0
    rows += [Row('dam', 'R', S2, 9, 1, FULL), Row('dam', 'R', S3, 9, 0, FULL), Row('dam', 'L', S2, 9, 1, FULL), Row('dam', 'T', S2, 9, 0, FULL),
             Row('dam', 'R', S2, 5, 1, FULL), Row('dam', 'R', S2, 17, 1, FULL), Row('dam', 'R', S3, 17, 0, DICE), Row('dam', 'R', S3, 5, 0, CE | DICE),
             Row('dam', 'R', S3, 9, 1, WMAP | DICE),
             Row('dam', 'R', S3, 9, 1, FULL, spec='bg0'), Row('dam', 'T', S2, 17, 1, FULL, spec='bg0'), Row('dam', 'L', S3, 5, 1, FULL, spec='bg0')]
    for si, (shape, mis) in enumerate(small):
        rows.append(Row('mask', 'LTR'[si % 3], shape, terms=si + 2, mis=mis))
    rows += [Row('mask', 'R', CAP9, terms=FULL), Row('mask', 'R', S2, terms=0), Row('mask', 'R', S3, terms=1), Row('mask', 'R', S2, terms=FULL),
             Row('mask', 'T', S3, terms=DICE), Row('mask', 'L', S4, terms=CE), Row('mask', 'R', S4, terms=WMAP | CE)]
    for ni, ND in enumerate((5, 9, 17)):
        for si, (shape, mis) in enumerate(small):
            k = si + ni + 1
            if (si + ni) % 2 == 0 or shape in (S4, S5):
                rows.append(Row('val', 'LTR'[k % 3], shape, ND, mis=mis, spec=('rank', 'perm')[k % 2]))
        rows.append(Row('val', 'R', CAP17 if ND == 17 else CAP9, ND, spec='perm'))
    rows.append(Row('val', 'R', S2, 9, spec='rank'))
    return [dataclasses.replace(r, seed=1000 + 7 * i) for i, r in enumerate(rows)]


ROWS = _rows()
ROW_BY_ID = {r.id: r for r in ROWS}
assert len(ROW_BY_ID) == len(ROWS), 'row ids collide'


def check_coverage():
    """every pair the tests rely on appears in at least one row"""
    dam = [r for r in ROWS if r.entry == 'dam']
    val = [r for r in ROWS if r.entry == 'val']
    mask = [r for r in ROWS if r.entry == 'mask']
    small = [(S1, False), (S2, False), (S2, True), (S3, False), (S4, False), (S5, False)]
    for ND in (5, 9, 17):
        cap = (CAP17 if ND == 17 else CAP9, False)
        assert {(r.shape, r.mis) for r in dam if r.ND == ND} >= set(small + [cap]), ND
        assert {(r.shape, r.mis) for r in val if r.ND == ND} >= {(S4, False), (S5, False), cap}, ND
        for rs in (dam, val):
            assert {r.fam for r in rs if r.ND == ND} == set('LTR'), ND
        assert {r.quirk for r in dam if r.ND == ND} == {0, 1}
        assert {r.terms for r in dam if r.ND == ND} == set(DAM_WORDS)
        assert {r.spec for r in val if r.ND == ND} == {'rank', 'perm'}
    assert {(r.shape, r.mis) for r in val} >= set(small)
    assert {(r.shape, r.mis) for r in mask} >= set(small + [(CAP9, False)])
    assert {r.terms for r in mask} == set(range(8)) and {r.fam for r in mask} == set('LTR')
    assert any(r.spec == 'bg0' and r.quirk for r in dam)
    assert any(r.terms == FULL and r.ND == 9 for r in dam)
    for r in ROWS:
        assert r.fam == 'R' or r.P <= 43690, r.id                       # 128 * 3 * P < 2^24
        assert r.shape[0] <= 64
    assert len(ROWS) <= 70, len(ROWS)


# ----------------------------------------------------------------------------------------------------------------------------------
# data
# ----------------------------------------------------------------------------------------------------------------------------------
def _saturated(rng, win, NC):
    """logits [B, NC, P]: 0 at channel win[b, p], -128 elsewhere"""
    l = np.full(win.shape[:1] + (NC,) + win.shape[1:], -128.0, f32)
    np.put_along_axis(l, win[:, None, :], 0.0, axis=1)
    return l


def _ties(rng, B, NC, P, counts):
    """logits in {0, -128}: per pixel n zeros at random channels, n drawn from `counts`"""
    n = rng.choice(counts, size=(B, 1, P))
    order = np.argsort(rng.random((B, NC, P)), axis=1)
    return np.where(order < n, 0.0, -128.0).astype(f32)


@functools.lru_cache(maxsize=None)
def make_data(row):
    """dict of numpy arrays: lm f32 [B,3,P], lp f32 [B,P], ld f32 [B,ND,P], lab / dl / wt u8 [B,P], pt f16 [B,P], lut int [ND] (val);
    built once per row and never modified"""
    rng = np.random.default_rng(row.seed)
    (B, H, W), ND, P = row.shape, row.ND, row.P
    lab = rng.integers(0, 3, (B, P)).astype(np.uint8)
    dl = rng.integers(0, ND, (B, P)).astype(np.uint8)
    if row.spec == 'bg0':
        lab[0] = 0
    if row.entry != 'mask':
        if B >= 2:
            dl[B - 1] = ND - 1                                          # constant at a non-zero class
        if B >= 3:
            lab[B - 2] = 0                                              # no foreground at all
    lut = None
    if row.entry == 'val':
        if row.spec == 'rank':
            dl[dl == 2] = 3
            present = np.unique(dl)
            lut = np.full(ND, -1, np.int32)
            lut[present] = np.arange(len(present))
        else:
            lut = rng.permutation(ND).astype(np.int32)
            lut[int(dl[0, 0])] = -1                                     # a class that occurs in sample 0
    if row.fam == 'R':
        lm = (rng.standard_normal((B, 3, P)) * 2).astype(f32)
        ld = (rng.standard_normal((B, ND, P)) * 2).astype(f32)
        lp = rng.standard_normal((B, P)).astype(f32)
        wt = rng.integers(0, 256, (B, P)).astype(np.uint8)
        pt = (rng.random((B, P)) * (255 if row.entry == 'val' else 1)).astype(np.float16)
    else:
        wt = (rng.integers(1, 4, (B, P)) * 20).astype(np.uint8)
        lp = (rng.integers(-8, 9, (B, P)) / 4).astype(f32)
        pt = (rng.integers(-8, 9, (B, P)) / 4).astype(np.float16)
        if row.fam == 'L':
            lm = _saturated(rng, np.where(rng.random((B, P)) < 0.5, lab, rng.integers(0, 3, (B, P))).astype(np.int64), 3)
            t = dl.astype(np.int64)
            kind = rng.integers(0, 4, (B, P))
            nx = np.where(t == ND - 1, 1, t + 1)
            pv = np.where(t == 1, ND - 1, t - 1)
            win = np.select([kind == 0, kind == 1, kind == 2], [t, np.where(t >= 1, nx, t), np.where(t >= 1, pv, t)], rng.integers(0, ND, (B, P)))
            ld = _saturated(rng, win, ND)
        else:
            lm = _ties(rng, B, 3, P, [1, 2])
            ld = _ties(rng, B, ND, P, [1, 2, 4])
    d = dict(lm=lm, lp=lp, ld=ld, lab=lab, dl=dl, wt=wt, pt=pt, lut=lut)
    for v in d.values():
        if v is not None:
            v.setflags(write=False)
    return d


# ----------------------------------------------------------------------------------------------------------------------------------
# reference (plain float64)
# ----------------------------------------------------------------------------------------------------------------------------------
VARIANTS = {1: 'dnext / dprev without the cyclic wrap', 2: 'a_next and a_prev exchanged', 3: "quirk on using the sample's own label",
            4: "quirk off using sample 0's label", 5: 'the single flag ignored', 6: 'class 0 not doubled in the weighted dice',
            7: 'w / ND dropped from the direction dice gradient', 8: 'CE gradient without w', 9: 'last-maximum arg-max',
            10: "val_sums without q'_0 *= p_0", 11: "val_sums foreground from the sample's own label",
            12: "val_sums treating an absent class's -1 rank as channel 0"}


def _softmax64(l):
    x = l.astype(f64)
    a = x - x.max(1, keepdims=True)
    e = np.where(a <= -104, 0.0, np.exp(a))                           # below half the smallest fp32 denormal: 0 in fp32 (2.6e-56 at -128)
    s = e.sum(1, keepdims=True)
    return e / s, a - np.log(s)


def _argmax(l, last=False):
    return l.shape[1] - 1 - np.argmax(l[:, ::-1], axis=1) if last else np.argmax(l, axis=1)


def _onehot(idx, n):
    """[B, n, P] float64 one-hot of idx [B, P]; idx < 0 gives zeros"""
    return (idx[:, None, :] == np.arange(n)[None, :, None]).astype(f64)


def _pick(a, idx):
    return np.take_along_axis(a, idx[:, None, :].astype(np.int64), axis=1)[:, 0]


def _tpfpfn(pred1, true1):
    return [(pred1 & true1).sum(1).astype(f64), (pred1 & ~true1).sum(1).astype(f64), (~pred1 & true1).sum(1).astype(f64)]


def pixel_metrics64(tp, fp, fn, P):
    tn = P - tp - fp - fn
    pr, rc = tp / (tp + fp + 1e-10), tp / (tp + fn + 1e-10)
    m = np.stack([(tp + tn) / (tp + fp + tn + fn + 1e-10), tp / (tp + fp + fn + 1e-10), rc, pr, 2 * pr * rc / (pr + rc + 1e-10)])
    return m.sum(1) / len(tp)


def _mask_part(d, w, B, P, on_ce, on_dice, variant):
    """the mask terms both losses share: sums I, P, T, ce; alpha, beta; ce, dice; dmask"""
    p3, lp3 = _softmax64(d['lm'])
    lab = d['lab'].astype(np.int64)
    oh = _onehot(lab, 3)
    I, Pc, T = (p3 * oh).sum(2), p3.sum(2), oh.sum(2)
    ce_s = (-_pick(lp3, lab) * w).sum(1)
    U = Pc + T
    alpha, beta = -2 / (B * (U + 1)), 2 * (I + 1) / (B * (U + 1) ** 2)
    ce = ce_s.sum() / (B * P)
    dice = sum(1 - (2 * (I[:, c] + 1) / (U[:, c] + 1)).sum() / B for c in range(3))
    g = (beta[:, :, None] + oh * alpha[:, :, None]) * (1.0 if on_dice else 0.0)
    dm = p3 * (g - (p3 * g).sum(1, keepdims=True))
    if on_ce:
        dm = dm + (np.ones_like(w) if variant == 8 else w)[:, None, :] * (p3 - oh) / (B * P)
    return dict(I=I, P=Pc, T=T, ce_s=ce_s, alpha=alpha, beta=beta, ce=ce, dice=dice, dmask=dm)


def reference(row, d, variant=0):
    """everything the entry reports, float64; `variant` switches one of VARIANTS on (0: the true reference)"""
    (B, _, _), P, ND = row.shape, row.P, row.ND
    if row.entry == 'val':
        return _reference_val(row, d, variant)
    wmap = bool(row.terms & WMAP)
    w = d['wt'].astype(f64) / 20 if wmap else np.ones((B, P))
    if row.entry == 'mask':
        m = _mask_part(d, w, B, P, bool(row.terms & CE), bool(row.terms & DICE), variant)
        am = _argmax(d['lm'], last=variant == 9)
        cnt = _tpfpfn(am == 1, d['lab'] == 1)
        sums = np.concatenate([m['I'], m['P'], m['T'], m['ce_s'][:, None], np.stack(cnt, 1)], 1)
        total = (m['ce'] if row.terms & CE else 0.0) + (m['dice'] if row.terms & DICE else 0.0)
        losses = np.concatenate([[total, m['ce'], m['dice']], pixel_metrics64(*cnt, P)])
        return dict(sums=sums, coef=np.concatenate([m['alpha'], m['beta']], 1), losses=losses, dmask=m['dmask'])
    Y = LossLay(ND)
    wrap = variant != 1
    NX, PV = [nxt(j, ND, wrap) for j in range(ND)], [prv(j, ND, wrap) for j in range(ND)]
    m = _mask_part(d, w, B, P, bool(row.terms & CE), True, variant)
    q, lq = _softmax64(d['ld'])
    lab, dl = d['lab'].astype(np.int64), d['dl'].astype(np.int64)
    single = (dl.min(1) == dl.max(1)).astype(np.int64)
    quirk = row.quirk if variant not in (3, 4) else 1 - row.quirk
    fg = np.broadcast_to(lab[0] != 0, (B, P)) if quirk else lab != 0
    t = np.where(fg, dl, -1)
    if variant != 5:
        t[single == 1] = 0
    oht = _onehot(t, ND)
    Pw, Tw = (w[:, None] * q).sum(2), (w[:, None] * oht).sum(2)
    SS = (w[:, None] * q * oht).sum(2)
    SN, SP = np.zeros((B, ND)), np.zeros((B, ND))
    for j in range(1, ND):
        SN[:, j] = (w * q[:, NX[j]] * oht[:, j]).sum(1)
        SP[:, j] = (w * q[:, PV[j]] * oht[:, j]).sum(1)
    dce_s = (-_pick(lq, dl) * w).sum(1)
    dpt = d['lp'].astype(f64) - d['pt'].astype(f64)
    mse_s = (dpt * dpt).sum(1)
    cnt = _tpfpfn(_argmax(d['ld'], last=variant == 9) == 1, dl == 1)
    sums = np.concatenate([m['I'], m['P'], m['T'], Pw, Tw, SS, SN, SP, np.stack([m['ce_s'], dce_s, mse_s] + cnt, 1)], 1)
    # coefficients and the dice value
    plain = not wmap
    m0 = 1.0 if plain or variant == 6 else 2.0
    ratio = lambda S_, U_: 2 * (S_ + 1) / (U_ + 1)
    al = lambda U_: -2 / (B * (U_ + 1))
    be = lambda S_, U_: 2 * (S_ + 1) / (B * (U_ + 1) ** 2)
    bsum, a_self, a_next, a_prev = np.zeros((B, ND)), np.zeros((B, ND)), np.zeros((B, ND)), np.zeros((B, ND))
    terms_ii = np.zeros(ND)
    wd = 0.0
    for j in range(ND):
        mm = m0 if j == 0 else 1.0
        U_ = Pw[:, j] + Tw[:, j]
        a_self[:, j] = mm * al(U_)
        bsum[:, j] += mm * be(SS[:, j], U_)
        terms_ii[j] = 1 - ratio(SS[:, j], U_).sum() / B
        if not plain and j >= 1:
            i_n, i_p = NX[j], PV[j]
            Un, Up = Pw[:, i_n] + Tw[:, j], Pw[:, i_p] + Tw[:, j]
            a_next[:, j], a_prev[:, j] = al(Un), al(Up)
            bsum[:, i_n] += be(SN[:, j], Un)
            bsum[:, i_p] += be(SP[:, j], Up)
            # loss.py:252-258: d_i - (1 - d(i, prev(i))) - (1 - d(i, next(i))): the pair (row next(j), target j) is d(i, prev(i)) of i = next(j)
            wd -= ratio(SN[:, j], Un).sum() / B + ratio(SP[:, j], Up).sum() / B
    if plain:
        wd = terms_ii.sum()
    else:
        wd = (m0 * terms_ii[0] + terms_ii[1:].sum() + wd) / ND
    if variant == 2:
        a_next, a_prev = a_prev, a_next
    coef = np.concatenate([m['alpha'], m['beta'], bsum, a_self, a_next, a_prev], 1)
    n = B * P
    dce, mse = dce_s.sum() / n, mse_s.sum() / n
    total = (m['ce'] if row.terms & CE else 0.0) + m['dice'] + dce + wd + mse
    losses = np.concatenate([[total, dce, wd, mse, m['ce'], m['dice']], pixel_metrics64(*cnt, P)])
    # direction gradient
    h = np.repeat(bsum[:, :, None], P, axis=2)
    for j in range(ND):
        sel = t == j
        for c, a in ((j, a_self), ) + (((NX[j], a_next), (PV[j], a_prev)) if j >= 1 else ()):
            h[:, c] += np.where(sel, a[:, j:j + 1], 0.0)
    if wmap and variant != 7:
        h = h * (w / ND)[:, None]
    ddir = q * (h - (q * h).sum(1, keepdims=True)) + (np.ones_like(w) if variant == 8 else w)[:, None] * (q - _onehot(dl, ND)) / n
    return dict(single=single, sums=sums, coef=coef, losses=losses, dmask=m['dmask'], ddir=ddir, dpoint=2 * dpt / n)


def _reference_val(row, d, variant=0):
    (B, _, _), P, ND = row.shape, row.P, row.ND
    p3, lp3 = _softmax64(d['lm'])
    q, lq = _softmax64(d['ld'])
    lab, dl = d['lab'].astype(np.int64), d['dl'].astype(np.int64)
    oh = _onehot(lab, 3)
    w = d['wt'].astype(f64) / 20
    qq = q.copy()
    if variant != 10:
        qq[:, 0] *= p3[:, 0]
    fg = np.broadcast_to(lab[0] != 0, (B, P)) if variant != 11 else lab != 0
    ch = d['lut'].astype(np.int64)[dl]
    if variant == 12:
        ch = np.maximum(ch, 0)
    oht = _onehot(np.where(fg, ch, -1), ND)
    dpt = d['lp'].astype(f64) - d['pt'].astype(f64) / 255
    cnt = _tpfpfn(_argmax(d['lm'], last=variant == 9) == 1, lab == 1)
    sums = np.concatenate([(p3 * oh).sum(2), p3.sum(2), oh.sum(2), (-_pick(lp3, lab)).sum(1)[:, None], (qq * oht).sum(2), qq.sum(2), oht.sum(2),
                           np.stack([(-w * _pick(lq, dl)).sum(1), (dpt * dpt).sum(1)] + cnt, 1)], 1)
    return dict(sums=sums)


# ----------------------------------------------------------------------------------------------------------------------------------
# the two arithmetics of the kernel model
# ----------------------------------------------------------------------------------------------------------------------------------
def _repr32(v):
    with np.errstate(over='ignore'):
        return v.astype(f32).astype(f64) == v


class V:
    """float64 value with a first-order bound of the fp32 computation's error (docstring: Bounds)"""
    __slots__ = ('v', 'e')

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, f64)
        self.e = np.zeros_like(self.v) + e

    @staticmethod
    def lift(x):
        return x if isinstance(x, V) else V(x)

    @property
    def exact(self):
        return self.e == 0

    def _rounded(self, v, ein, k=1.0, keep=None):
        e = ein + np.where((ein == 0) & _repr32(v), 0.0, k * U32 * np.abs(v))
        if keep is not None:
            for cond, ek in keep:
                e = np.where(cond, ek + 0 * v, e)
        return V(v, e)

    def __getitem__(self, i):
        return V(self.v[i], self.e[i])

    def __neg__(self):
        return V(-self.v, self.e)

    def __add__(self, o):
        o = V.lift(o)
        return self._rounded(self.v + o.v, self.e + o.e, keep=[(o.exact & (o.v == 0), self.e), (self.exact & (self.v == 0), o.e)])

    __radd__ = __add__

    def __sub__(self, o):
        return self + (-V.lift(o))

    def __rsub__(self, o):
        return V.lift(o) + (-self)

    def _mul(self, o, rounded=True):
        v = self.v * o.v
        ein = np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e
        if not rounded:
            return V(v, ein)
        unit = lambda x: x.exact & ((x.v == 0) | (np.abs(x.v) == 1))
        return self._rounded(v, ein, keep=[(unit(self) | unit(o), ein)])

    def __mul__(self, o):
        return self._mul(V.lift(o))

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = V.lift(o)
        v = self.v / o.v
        ein = (self.e + np.abs(v) * o.e) / (np.abs(o.v) - o.e)
        return self._rounded(v, ein, k=2 * ULP_DIV)

    def __rtruediv__(self, o):
        return V.lift(o) / self


class VOps:
    name = 'bound'
    lift = staticmethod(V.lift)

    @staticmethod
    def exp(a):
        v = np.exp(a.v)
        exact = a.exact & ((a.v == 0) | (a.v <= -104))
        v = np.where(a.exact & (a.v <= -104), 0.0, v)
        return V(v, np.where(exact, 0.0, v * np.expm1(a.e) + 2 * ULP_EXP * U32 * v))

    @staticmethod
    def log(s):
        v = np.log(s.v)
        return V(v, np.where(s.exact & (s.v == 1), 0.0, s.e / (s.v - s.e) + 2 * ULP_LOG * U32 * np.abs(v)))

    @staticmethod
    def fma(a, b, c):
        a, b, c = V.lift(a), V.lift(b), V.lift(c)
        pr = a._mul(b, rounded=False)
        zero = (a.exact & (a.v == 0)) | (b.exact & (b.v == 0))
        return c._rounded(pr.v + c.v, pr.e + c.e, keep=[(zero, c.e)])

    @staticmethod
    def where(m, a, b):
        a, b = V.lift(a), V.lift(b)
        return V(np.where(m, a.v, b.v), np.where(m, a.e, b.e))

    @staticmethod
    def scale2(x, k):
        return V(x.v * k, x.e * abs(k))

    @staticmethod
    def const(x):
        """a compile-time constant: the correctly rounded fp32 of x"""
        return V(x, 0.0 if f64(f32(x)) == x else U32 * abs(x))

    @staticmethod
    def from_double(x):
        x = np.asarray(x, f64)
        return V(x, np.where(_repr32(x), 0.0, U32 * np.abs(x)))

    @staticmethod
    def stack(xs, axis=0):
        return V(np.stack([x.v for x in xs], axis), np.stack([x.e for x in xs], axis))

    @staticmethod
    def val(x):
        return x.v

    @staticmethod
    def psum(t, tpb, double_chunks=False, fma=None):
        """per-sample sum over the pixels of terms [B, P] (fma = (a, b): the term a * b enters through one fused multiply-add)"""
        if fma is not None:
            t = V.lift(fma[0])._mul(V.lift(fma[1]), rounded=False)
        P = t.v.shape[1]
        absum, esum = np.abs(t.v).sum(1), t.e.sum(1)
        exact = esum == 0
        ok = np.zeros_like(exact)
        for k in range(5):                                              # quantum 2^-k
            ok |= (np.mod(t.v * 2.0 ** k, 1.0) == 0).all(1) & (absum * 2.0 ** k < 2.0 ** 24)
        return V(t.v.sum(1), np.where(exact & ok, 0.0, n_add(P, tpb, double_chunks) * U32 * absum + esum))


class F32Ops:
    """the kernels' arithmetic in numpy fp32, in their summation order (libm's expf / logf / division stand in for the device's)"""
    name = 'f32'
    lift = staticmethod(lambda x: np.asarray(x, f32))
    exp = staticmethod(np.exp)
    log = staticmethod(np.log)
    where = staticmethod(np.where)
    const = staticmethod(f32)
    from_double = staticmethod(lambda x: np.asarray(x, f64).astype(f32))
    stack = staticmethod(lambda xs, axis=0: np.stack(xs, axis))
    val = staticmethod(lambda x: np.asarray(x, f64))

    @staticmethod
    def fma(a, b, c):
        return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)

    @staticmethod
    def scale2(x, k):
        return x * f32(k)

    @staticmethod
    def psum(t, tpb, double_chunks=False, fma=None):
        a, b = (np.asarray(fma[0], f32), np.asarray(fma[1], f32)) if fma is not None else (np.asarray(t, f32), None)
        B, P = a.shape
        nchunk = loss_nchunk(P, tpb)
        stride = nchunk * tpb
        trips = -(-P // stride)
        pad = lambda x: np.concatenate([x, np.zeros((B, trips * stride - P), f32)], 1).reshape(B, trips, nchunk, tpb)
        a = pad(a)
        b = pad(b) if b is not None else None
        acc = np.zeros((B, nchunk, tpb), f32)
        for k in range(trips):
            acc = F32Ops.fma(a[:, k], b[:, k], acc) if b is not None else acc + a[:, k]
        part = np.zeros((B, nchunk), f32)
        for lane in range(tpb):
            part = part + acc[:, :, lane]
        if double_chunks:
            s = np.zeros(B, f64)
            for ch in range(nchunk):
                s = s + part[:, ch].astype(f64)
            return s.astype(f32)
        s = [np.zeros(B, f32) for _ in range(4)]
        ch = 0
        while ch + 3 < nchunk:
            for k in range(4):
                s[k] = s[k] + part[:, ch + k]
            ch += 4
        while ch < nchunk:
            s[0] = s[0] + part[:, ch]
            ch += 1
        return (s[0] + s[1]) + (s[2] + s[3])


# ----------------------------------------------------------------------------------------------------------------------------------
# the kernels, once, over either arithmetic
# ----------------------------------------------------------------------------------------------------------------------------------
def _softmax(ops, l):
    """softmax3 / softmax_n over the channel list l (raw f32 arrays [B, P]) -> lists p, logp"""
    m = ops.lift(np.max(np.stack(l), 0))
    e = [ops.exp(ops.lift(x) - m) for x in l]
    s = e[0]
    for x in e[1:]:
        s = s + x
    ls = ops.log(s)
    return [x / s for x in e], [ops.lift(x) - m - ls for x in l]


def _choose(ops, idx, xs):
    out = xs[0]
    for c in range(1, len(xs)):
        out = ops.where(idx == c, xs[c], out)
    return out


def _first_argmax(l):
    return np.argmax(np.stack(l, 1), axis=1)


def _seq(xs):
    s = xs[0]
    for x in xs[1:]:
        s = s + x
    return s


def _dice_terms(ops, S, B, triples):
    """dice_term for each (num, da, db): 1 - (sum_b 2 (S[num] + 1) / (S[da] + S[db] + 1)) / fB, vectorised over the triples"""
    num, da, db = [list(k) for k in zip(*triples)]
    Sm = ops.stack(S, 1)                                                # [B, NS]
    r = ops.scale2(Sm[:, num] + 1.0, 2.0) / (Sm[:, da] + Sm[:, db] + 1.0)
    acc = _seq([r[b] for b in range(B)])
    return 1.0 - acc / ops.lift(float(B))


def _mask_coef(ops, S, fB):
    """mask_dice_coef: alpha[3] + beta[3] as six [B] vectors"""
    al, be = [], []
    for c in range(3):
        I, U = S[c], S[3 + c] + S[6 + c]
        al.append(ops.lift(-2.0) / (fB * (U + 1.0)))
        be.append(ops.scale2(I + 1.0, 2.0) / (fB * (U + 1.0) * (U + 1.0)))
    return al + be


def _metrics(ops, S, tp0, B, P):
    tp, fp, fn = [ops.val(S[tp0 + k]) for k in range(3)]
    return [ops.from_double(x) for x in pixel_metrics64(tp, fp, fn, P)]


def _col(x):
    return x[:, None]


def _mask_grad_parts(ops, p3, lab, cf, w, inv_n):
    """(gd[c], gc[c]): p (g - dot) and w inv_n (p - onehot) of the three mask classes; cf = six [B] vectors or None (dice off)"""
    zero = ops.lift(0.0)
    gp = [(_col(cf[3 + c]) + ops.where(lab == c, _col(cf[c]), zero)) if cf is not None else zero for c in range(3)]
    dot = zero
    for c in range(3):
        dot = ops.fma(p3[c], gp[c], dot)
    gd = [p3[c] * (gp[c] - dot) for c in range(3)]
    gc = [w * inv_n * (p3[c] - ops.lift((lab == c).astype(f32))) for c in range(3)]
    return gd, gc


def _weights(ops, d, wmap):
    return ops.lift(d['wt'].astype(f32)) / ops.lift(20.0) if wmap else ops.lift(np.ones(d['lab'].shape, f32))


def model_mask(row, d, ops):
    (B, _, _), P = row.shape, row.P
    wmap, on_ce, on_dice = bool(row.terms & WMAP), bool(row.terms & CE), bool(row.terms & DICE)
    lab = d['lab'].astype(np.int64)
    l3 = [d['lm'][:, c] for c in range(3)]
    p3, lp3 = _softmax(ops, l3)
    w = _weights(ops, d, wmap)
    zero = ops.lift(0.0)
    ps = lambda t: ops.psum(t, MS_TPB)
    S = [ps(ops.where(lab == c, p3[c], zero)) for c in range(3)] + [ps(p3[c]) for c in range(3)] + \
        [ps(ops.lift((lab == c).astype(f32))) for c in range(3)]
    lpl = _choose(ops, lab, lp3)
    S.append(ps(-(lpl * w) if wmap else -lpl))
    am = _first_argmax(l3)
    pi, ti = am == 1, lab == 1
    S += [ps(ops.lift(x.astype(f32))) for x in (pi & ti, pi & ~ti, ~pi & ti)]
    fB = ops.lift(float(B))
    cf = _mask_coef(ops, S, fB)
    term = _dice_terms(ops, S, B, [(c, 3 + c, 6 + c) for c in range(3)])
    ce = _seq([S[9][b] for b in range(B)]) / ops.lift(float(B) * float(P))
    dice = _seq([term[c] for c in range(3)])
    total = ce + dice if on_ce and on_dice else ce if on_ce else dice if on_dice else zero
    losses = [total, ce, dice] + _metrics(ops, S, 10, B, P)
    inv_n = ops.lift(1.0) / ops.lift(float(B) * float(P))
    if not on_ce and not on_dice:
        dmask = [ops.lift(np.zeros((B, P), f32))] * 3
    else:
        gd, gc = _mask_grad_parts(ops, p3, lab, cf if on_dice else None, w, inv_n)
        dmask = [gd[c] + gc[c] if on_ce and on_dice else gd[c] if on_dice else gc[c] for c in range(3)]
    return dict(sums=ops.stack(S, 1), coef=ops.stack(cf, 1), losses=ops.stack(losses), dmask=ops.stack(dmask, 1))


def model_dam(row, d, ops):
    (B, _, _), P, ND = row.shape, row.P, row.ND
    Y = LossLay(ND)
    wmap, on_ce = bool(row.terms & WMAP), bool(row.terms & CE)
    plain = not wmap
    lab, dl = d['lab'].astype(np.int64), d['dl'].astype(np.int64)
    single = (dl.min(1) == dl.max(1))
    l3, l9 = [d['lm'][:, c] for c in range(3)], [d['ld'][:, c] for c in range(ND)]
    p3, lp3 = _softmax(ops, l3)
    p9, lp9 = _softmax(ops, l9)
    w = _weights(ops, d, wmap)
    zero = ops.lift(0.0)
    fg = np.broadcast_to(lab[0] != 0, (B, P)) if row.quirk else lab != 0
    t = np.where(single[:, None], 0, np.where(fg, dl, -1))
    NX, PV = [nxt(j, ND) for j in range(ND)], [prv(j, ND) for j in range(ND)]
    ps = lambda x: ops.psum(x, Y.TPB)
    pf = lambda a, b: ops.psum(None, Y.TPB, fma=(a, b))
    S = [ps(ops.where(lab == c, p3[c], zero)) for c in range(3)] + [ps(p3[c]) for c in range(3)] + \
        [ps(ops.lift((lab == c).astype(f32))) for c in range(3)]
    S += [pf(w, p9[c]) for c in range(ND)]
    S += [ps(ops.where(t == j, w, zero)) for j in range(ND)]
    S += [pf(ops.where(t == j, w, zero), p9[j]) for j in range(ND)]
    S += [pf(ops.where(t == j, w, zero), p9[NX[j]]) if j >= 1 else ps(ops.lift(np.zeros((B, P), f32))) for j in range(ND)]
    S += [pf(ops.where(t == j, w, zero), p9[PV[j]]) if j >= 1 else ps(ops.lift(np.zeros((B, P), f32))) for j in range(ND)]
    S.append(ps(-(_choose(ops, lab, lp3) * w)))
    S.append(ps(-(_choose(ops, dl, lp9) * w)))
    dpt = ops.lift(d['lp']) - ops.lift(d['pt'].astype(f32))
    S.append(pf(dpt, dpt))
    am = _first_argmax(l9)
    pi, ti = am == 1, dl == 1
    S += [ps(ops.lift(x.astype(f32))) for x in (pi & ti, pi & ~ti, ~pi & ti)]
    # loss_finalize_kernel
    fB = ops.lift(float(B))
    cf = _mask_coef(ops, S, fB)
    bsum = [zero] * ND
    a_self, a_next, a_prev = [None] * ND, [ops.lift(np.zeros(B, f32))] * ND, [ops.lift(np.zeros(B, f32))] * ND
    for j in range(ND):
        U, Sij, m = S[Y.PW + j] + S[Y.TW + j], S[Y.SS + j], 2.0 if j == 0 and not plain else 1.0
        a_self[j] = ops.lift(m * -2.0) / (fB * (U + 1.0))
        bsum[j] = bsum[j] + ops.scale2(Sij + 1.0, m * 2.0) / (fB * (U + 1.0) * (U + 1.0))
        if not plain and j >= 1:
            for i, base, dst in ((NX[j], Y.SN, a_next), (PV[j], Y.SP, a_prev)):
                U, Sij = S[Y.PW + i] + S[Y.TW + j], S[base + j]
                dst[j] = ops.lift(-2.0) / (fB * (U + 1.0))
                bsum[i] = bsum[i] + ops.scale2(Sij + 1.0, 2.0) / (fB * (U + 1.0) * (U + 1.0))
    cf = cf + bsum + a_self + a_next + a_prev
    T_PREV, T_NEXT = 3 + ND, 3 + ND + ND - 1
    tr = [(c, 3 + c, 6 + c) for c in range(3)] + [(Y.SS + i, Y.PW + i, Y.TW + i) for i in range(ND)] + \
         [(Y.SN + PV[i], Y.PW + i, Y.TW + PV[i]) for i in range(1, ND)] + [(Y.SP + NX[i], Y.PW + i, Y.TW + NX[i]) for i in range(1, ND)]
    term = _dice_terms(ops, S, B, tr)
    n = ops.lift(float(B) * float(P))
    ce, dce, mse = [_seq([S[Y.SC + k][b] for b in range(B)]) / n for k in range(3)]
    dice = _seq([term[c] for c in range(3)])
    if plain:
        wd = _seq([term[3 + i] for i in range(ND)])
    else:
        wd = ops.scale2(term[3], 2.0)
        for i in range(1, ND):
            wd = wd + (term[3 + i] - (1.0 - term[T_PREV + i - 1]) - (1.0 - term[T_NEXT + i - 1]))
        wd = wd / ops.lift(float(ND))
    total = ce + dice + dce + wd + mse if on_ce else dice + dce + wd + mse
    losses = [total, dce, wd, mse, ce, dice] + _metrics(ops, S, Y.SC + 3, B, P)
    # loss_grad_kernel
    inv_n = ops.lift(1.0) / (ops.lift(float(B)) * ops.lift(float(P)))
    gd, gc = _mask_grad_parts(ops, p3, lab, cf, w, inv_n)
    dmask = [gd[c] + gc[c] if on_ce else gd[c] for c in range(3)]
    gq = []
    for c in range(ND):
        a = zero
        a = ops.where(t == c, _col(a_self[c]), a)
        if c >= 1:
            for j in range(1, ND):                                      # the else-if chain: self, then next, then prev
                if NX[j] == c and j != c:
                    a = ops.where(t == j, _col(a_next[j]), a)
            for j in range(1, ND):
                if PV[j] == c and j != c and NX[j] != c:
                    a = ops.where(t == j, _col(a_prev[j]), a)
        gq.append(_col(bsum[c]) + a)
    if wmap:
        k = w * ops.const(1.0 / ND)
        gq = [g * k for g in gq]
    dotq = zero
    for c in range(ND):
        dotq = ops.fma(p9[c], gq[c], dotq)
    ddir = [p9[c] * (gq[c] - dotq) + w * inv_n * (p9[c] - ops.lift((dl == c).astype(f32))) for c in range(ND)]
    dpoint = ops.scale2(inv_n, 2.0) * dpt
    return dict(single=single.astype(np.int64), sums=ops.stack(S, 1), coef=ops.stack(cf, 1), losses=ops.stack(losses),
                dmask=ops.stack(dmask, 1), ddir=ops.stack(ddir, 1), dpoint=dpoint)


def model_val(row, d, ops):
    (B, _, _), P, ND = row.shape, row.P, row.ND
    Y = ValLay(ND)
    lab, dl = d['lab'].astype(np.int64), d['dl'].astype(np.int64)
    l3, l9 = [d['lm'][:, c] for c in range(3)], [d['ld'][:, c] for c in range(ND)]
    p3, lp3 = _softmax(ops, l3)
    p9, lp9 = _softmax(ops, l9)
    w = _weights(ops, d, True)
    zero = ops.lift(0.0)
    ps = lambda x: ops.psum(x, Y.TPB, True)
    S = [ps(ops.where(lab == c, p3[c], zero)) for c in range(3)] + [ps(p3[c]) for c in range(3)] + \
        [ps(ops.lift((lab == c).astype(f32))) for c in range(3)]
    S.append(ps(-_choose(ops, lab, lp3)))
    p9 = [p9[0] * p3[0]] + p9[1:]
    ch = d['lut'].astype(np.int64)[dl]
    tch = np.where(np.broadcast_to(lab[0] != 0, (B, P)) & (ch >= 0), ch, -1)
    S += [ps(ops.where(tch == c, p9[c], zero)) for c in range(ND)]
    S += [ps(p9[c]) for c in range(ND)]
    S += [ps(ops.lift((tch == c).astype(f32))) for c in range(ND)]
    S.append(ps(-(w * _choose(ops, dl, lp9))))
    dpt = ops.lift(d['lp']) - ops.lift(d['pt'].astype(f32)) / ops.lift(255.0)
    S.append(ops.psum(None, Y.TPB, True, fma=(dpt, dpt)))
    am = _first_argmax(l3)
    pi, ti = am == 1, lab == 1
    S += [ps(ops.lift(x.astype(f32))) for x in (pi & ti, pi & ~ti, ~pi & ti)]
    return dict(sums=ops.stack(S, 1))


MODELS = dict(dam=model_dam, mask=model_mask, val=model_val)
QUANTITIES = ('sums', 'coef', 'losses', 'dmask', 'ddir', 'dpoint')


@functools.lru_cache(maxsize=4)
def bounds(row):
    """{quantity: bound array} from the V model; its values must agree with the reference (they are the same closed forms)"""
    d = make_data(row)
    ref = reference(row, d)
    mv = MODELS[row.entry](row, d, VOps)
    out = {}
    for k, x in mv.items():
        if k == 'single':
            assert np.array_equal(x, ref['single'])
            continue
        scale = max(1.0, float(np.abs(ref[k]).max()))
        assert np.abs(x.v - ref[k]).max() <= 1e-9 * scale, '%s: the kernel model and the reference disagree on %s' % (row.id, k)
        out[k] = x.e * HI
    return out


def emulate(row):
    """the fp32 emulation's outputs as float64 arrays"""
    return {k: np.asarray(v, f64) for k, v in MODELS[row.entry](row, make_data(row), F32Ops).items()}


def layout(row):
    return ValLay(row.ND) if row.entry == 'val' else LossLay(row.ND) if row.entry == 'dam' else None


def sum_name(row, k):
    return MS_NAMES[k] if row.entry == 'mask' else layout(row).name(k)


def exact_columns(row):
    """the columns of `sums` the family makes exact (compared with ==): all on L, all but the cross-entropies on T"""
    if row.fam == 'R':
        names = ('T_', 'tp', 'fp', 'fn', 'Tq_')
        n = MS_SUMS if row.entry == 'mask' else layout(row).SUMS
        return [k for k in range(n) if sum_name(row, k).startswith(names)]
    n = MS_SUMS if row.entry == 'mask' else layout(row).SUMS
    inexact = ('mse',) if row.entry == 'val' else ()                    # target / 255
    return [k for k in range(n) if sum_name(row, k) not in inexact + (('ce', 'dce') if row.fam == 'T' else ())]


def guard(row):
    """before any GPU call: the family's exactness holds on the row's own data (the bound of every exact column is 0, which `V.psum`
    grants only to terms that are multiples of a quantum with less than 2^24 quanta in all), the label content is in range, the data
    has what the row is there for, and every bound is finite"""
    d = make_data(row)
    ref = reference(row, d)
    bd = bounds(row)
    (B, _, _), P, ND = row.shape, row.P, row.ND
    assert d['lab'].max() <= 2 and d['dl'].max() <= ND - 1
    for k, b in bd.items():
        assert np.isfinite(b).all() and (b >= 0).all(), (row.id, k)
    ex = exact_columns(row)
    assert (bd['sums'][:, ex] == 0).all(), '%s: columns %s are not exact' % (row.id, [sum_name(row, k) for k in ex if (bd['sums'][:, k] != 0).any()])
    assert (ref['sums'][:, ex] < 2.0 ** 24).all()
    if row.fam == 'L':
        assert (np.mod(ref['sums'][:, ex] * 16, 1) == 0).all(), row.id
    if row.entry == 'dam':
        if B >= 2:
            assert ref['single'][B - 1] == 1 and d['dl'][B - 1, 0] == ND - 1
        assert ref['single'][0] == (1 if P == 1 else 0)
        if P >= 400 and row.spec != 'bg0':
            pairs = {(int(a), int(b)) for a, b in zip(d['lab'][0], d['dl'][0])}
            assert pairs == {(a, b) for a in range(3) for b in range(ND)}, row.id
            if B >= 2 and not row.quirk:
                assert ((d['dl'][1] != 0) & (d['lab'][1] == 0)).any()
            Y = LossLay(ND)
            if row.fam != 'T' and (row.terms & WMAP):
                assert (ref['sums'][0, Y.SN + 1:Y.SN + ND] > 0).all() and (ref['sums'][0, Y.SP + 1:Y.SP + ND] > 0).all(), row.id
    if row.entry == 'val':
        assert (d['lut'] == -1).sum() >= 1
        if row.spec == 'perm':
            assert (d['lut'][d['dl'][0].astype(np.int64)] == -1).any()
    return ref, bd


# ----------------------------------------------------------------------------------------------------------------------------------
# comparison
# ----------------------------------------------------------------------------------------------------------------------------------
def worst(err, bound):
    """(largest err / bound, its index); a zero bound with a zero error counts 0, with a non-zero error inf"""
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(err == 0, 0.0, err / bound)
    q = np.where(np.isnan(q), np.inf, q)
    i = np.unravel_index(int(np.argmax(q)), q.shape)
    return float(q[i]), tuple(int(k) for k in i)


LOSS_NAMES = dict(dam='total dce wdice mse ce dice accuracy iou recall precision f1'.split(),
                  mask='total ce dice accuracy iou recall precision f1'.split())


def describe(row, name, got, want, i, bound=None):
    """quantity, sample, class, pixel, got and want of element i"""
    if name == 'sums':
        where = 'sample %d, %s' % (i[0], sum_name(row, i[1]))
    elif name == 'coef':
        k = i[1]
        nm = ('alpha_%d' % k if k < 3 else 'beta_%d' % (k - 3)) if k < 6 else '%s_%d' % (('bsum', 'a_self', 'a_next', 'a_prev')[(k - 6) // row.ND], (k - 6) % row.ND)
        where = 'sample %d, %s' % (i[0], nm)
    elif name == 'losses':
        where = LOSS_NAMES[row.entry][i[0]]
    elif name == 'dpoint':
        where = 'sample %d, pixel %d' % i
    else:
        where = 'sample %d, class %d, pixel %d' % i
    s = '%s: %s [%s]: got %r want %r' % (row.id, name, where, float(got[i]), float(want[i]))
    return s if bound is None else s + ' bound %.3g' % float(bound[i])


def compare(row, got, ref, bd, report=None, what=QUANTITIES):
    """every element of every quantity in `got` against the reference: == where the bound is 0, err <= bound elsewhere.  Returns
    {quantity: worst err / bound}."""
    report = {} if report is None else report
    if 'single' in got:
        assert np.array_equal(got['single'], ref['single']), '%s: single flags: got %s want %s' % (row.id, got['single'].tolist(), ref['single'].tolist())
    for name in what:
        if name not in got:
            continue
        g, w_, b = np.asarray(got[name], f64), ref[name], bd[name]
        assert g.shape == w_.shape, (row.id, name, g.shape, w_.shape)
        q, i = worst(np.abs(g - w_), b)
        report[name] = max(report.get(name, 0.0), q)
        assert q <= 1.0, 'err / bound = %.3g; ' % q + describe(row, name, g, w_, i, b)
    return report


# ----------------------------------------------------------------------------------------------------------------------------------
# device side (imported lazily: the CPU tests use everything above)
# ----------------------------------------------------------------------------------------------------------------------------------
class OutBuffer:
    """a sentinel-filled float tensor inside a sentinel-filled allocation with SLACK elements on both ends"""

    def __init__(self, shape, fill=SENTINEL):
        import torch
        n = int(np.prod(shape))
        self.full = torch.full((n + 2 * SLACK,), fill, dtype=torch.float32, device='cuda')
        self.t = self.full[SLACK:SLACK + n].view(*shape)
        self.sent = float(torch.full((1,), fill, dtype=torch.float32)[0])
        self.bits = self.full.view(torch.int32).cpu().numpy().copy()

    def ptr(self):
        return C.c_void_p(self.t.data_ptr())

    def read(self):
        """(the tensor as float64 numpy, the slack still holds its bits)"""
        import torch
        raw = self.full.view(torch.int32).cpu().numpy()
        f = self.full.double().cpu().numpy()
        n = f.size - 2 * SLACK
        ok = bool((raw[:SLACK] == self.bits[:SLACK]).all() and (raw[SLACK + n:] == self.bits[SLACK + n:]).all())
        return f[SLACK:SLACK + n].reshape(tuple(self.t.shape)), ok

    def untouched(self):
        import torch
        return bool((self.full.view(torch.int32).cpu().numpy() == self.bits).all())


class DeviceCase:
    """the row's inputs on the device; `mis` puts the label and the direction map one byte into larger buffers"""

    def __init__(self, row, d, lab=None, dl=None):
        import torch
        self.row = row
        dev = lambda a: torch.from_numpy(np.array(a)).cuda()
        self.lm, self.lp, self.ld = dev(d['lm']), dev(d['lp']), dev(d['ld'])
        self.pt, self.wt = dev(d['pt']), dev(d['wt'])

        def u8(a):
            a = np.array(a).reshape(-1)
            if not row.mis:
                return dev(a)
            big = torch.full((a.size + 32,), 255, dtype=torch.uint8, device='cuda')
            assert big.data_ptr() % 16 == 0
            big[1:1 + a.size] = torch.from_numpy(a).cuda()
            return big[1:1 + a.size]
        self.lab, self.dl = u8(d['lab'] if lab is None else lab), u8(d['dl'] if dl is None else dl)
        if row.mis:
            assert self.lab.data_ptr() % 16 == 1 and self.dl.data_ptr() % 16 == 1


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def query(row):
    from cdnet_amd import _lib
    lib = _lib.load()
    B, P = row.shape[0], row.P
    if row.entry == 'dam':
        return lib.cdnet_dam_loss_classes_workspace_floats(B, P, row.ND)
    if row.entry == 'mask':
        return lib.cdnet_mask_loss_workspace_floats(B, P)
    return lib.cdnet_dam_val_sums_classes_workspace_floats(B, P, row.ND)


class Run:
    """one call of an entry on a row: sentinel-filled outputs, a NaN-filled workspace with SLACK NaN floats behind the part the library
    asked for.  `entry`: 'terms' | 'classes' | 'plain' (cdnet_dam_loss) | 'mask' | 'val'."""

    def __init__(self, row, dc, entry, grads=True, B=None, ws_floats=None, only=None):
        import torch
        from cdnet_amd import _lib
        lib = _lib.load()
        (Bt, H, W), P, ND = row.shape, row.P, row.ND
        self.row, self.lay = row, ws_layout(row.entry, Bt, P, ND)
        need = query(row)
        assert need == self.lay['total'], '%s: ws_layout says %d floats, the library %d' % (row.id, self.lay['total'], need)
        self.ws = OutBuffer((need,), float('nan'))
        self.losses = OutBuffer((11 if row.entry == 'dam' else 8,)) if row.entry != 'val' else None
        self.dmask = OutBuffer((Bt, 3, P)) if row.entry != 'val' else None
        self.ddir = OutBuffer((Bt, ND, P)) if row.entry == 'dam' else None
        self.dpoint = OutBuffer((Bt, P)) if row.entry == 'dam' else None
        self.sums = OutBuffer((Bt, ValLay(ND).SUMS)) if row.entry == 'val' else None
        B = Bt if B is None else B
        wsf = need if ws_floats is None else ws_floats
        g = lambda name, buf: buf.ptr() if grads and (only is None or name in only) else None
        st = _lib.stream_ptr()
        wt = _p(dc.wt) if row.entry == 'val' or row.terms & WMAP else None
        if row.entry == 'dam':
            head = [_p(dc.lm), _p(dc.lp), _p(dc.ld), _p(dc.lab), _p(dc.dl), _p(dc.pt)]
            tail = [self.ws.ptr(), wsf, self.losses.ptr(), g('dmask', self.dmask), g('dpoint', self.dpoint), g('ddir', self.ddir), st]
            if entry == 'terms':
                self.rc = lib.cdnet_dam_loss_terms(*head, wt, B, H, W, ND, row.quirk, *tail, row.terms)
            elif entry == 'classes':
                self.rc = lib.cdnet_dam_loss_classes(*head, wt, B, H, W, ND, row.quirk, *tail)
            else:
                self.rc = lib.cdnet_dam_loss(*head, wt, B, H, W, row.quirk, *tail)
        elif row.entry == 'mask':
            self.rc = lib.cdnet_mask_loss(_p(dc.lm), _p(dc.lab), wt, B, H, W, row.terms, self.ws.ptr(), wsf, self.losses.ptr(),
                                          g('dmask', self.dmask), st)
        else:
            self.lut = (C.c_int * ND)(*[int(k) for k in make_data(row)['lut']])
            self.rc = lib.cdnet_dam_val_sums_classes(_p(dc.lm), _p(dc.lp), _p(dc.ld), _p(dc.lab), _p(dc.dl), _p(dc.pt), _p(dc.wt), self.lut,
                                                     ND, B, H, W, self.ws.ptr(), wsf, self.sums.ptr(), st)
        torch.cuda.synchronize()
        self.err = lib.cdnet_last_error().decode(errors='replace') if self.rc else ''

    def outputs(self):
        return {k: b for k, b in (('ws', self.ws), ('losses', self.losses), ('dmask', self.dmask), ('ddir', self.ddir),
                                  ('dpoint', self.dpoint), ('sums', self.sums)) if b is not None}

    def untouched(self):
        """the name of an output the call wrote, or None"""
        for k, b in self.outputs().items():
            if not b.untouched():
                return k
        return None

    def read(self, grads=True):
        """{quantity: float64 array} of everything the call reported, after the sentinel checks: the slack around every output holds,
        every element of every output was written, `sums`, `coef` and `single` come out of the workspace through ws_layout"""
        import torch
        row, lay = self.row, self.lay
        (B, _, _), ND = row.shape, row.ND
        got = {}
        for k, b in self.outputs().items():
            x, ok = b.read()
            assert ok, '%s: the call wrote outside %s' % (row.id, k)
            if k == 'ws':
                ws = x
            elif k in ('losses', 'sums') or grads:
                un = x == b.sent
                assert not un.any(), '%s: %d elements of %s were not written, the first at %s' % (row.id, int(un.sum()), k, [int(a[0]) for a in np.nonzero(un)])
                got[k] = x
            else:
                assert b.untouched(), '%s: a call without gradient pointers wrote %s' % (row.id, k)
        nchunk = lay['nchunk']
        if row.entry == 'dam':
            Y = LossLay(ND)
            part = ws[:lay['coef']].reshape(B, nchunk, Y.SUMS)
            got['coef'] = ws[lay['coef']:lay['sums']].reshape(B, Y.COEF)
            got['sums'] = ws[lay['sums']:lay['pad']].reshape(B, Y.SUMS)
            ints = self.ws.t.view(torch.int32).cpu().numpy()
            got['single'] = ints[lay['single']:lay['total']].astype(np.int64)
            assert ints[lay['pad']] == 0, row.id + ': error flag raised'
            assert np.isnan(ws[lay['pad'] + 1:lay['single']]).all(), row.id + ': the pad behind the error flag was written'
        elif row.entry == 'mask':
            part = ws[:lay['coef']].reshape(B, nchunk, MS_SUMS)
            got['coef'] = ws[lay['coef']:lay['pad']].reshape(B, MS_COEF)
            got['sums'] = part.sum(1)                                    # the kernel keeps no summed rows: the partial rows, added in double
            ints = self.ws.t.view(torch.int32).cpu().numpy()
            assert ints[lay['pad']] == 0, row.id + ': error flag raised'
            assert np.isnan(ws[lay['pad'] + 1:]).all(), row.id + ': the pad behind the error flag was written'
        else:
            part = ws.reshape(B, nchunk, ValLay(ND).SUMS)
        assert not np.isnan(part).any(), row.id + ': partial rows not fully written'
        got['partial'] = part
        return got
