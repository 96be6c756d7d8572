"""Real-valued tests of cdnet_conv_backward_weight with a derived per-element bound: one row per kernel family and source transform,
random data (rounded to the storage type), non-lattice scale and shift.

Reference: float64 (tests/_wgrad_cases.py: the source transform with the kernels' rounding points, then the float64 sum).  Bound per
element, S = sum |a * g| over the element's terms, c = chain_length(family, shape, ksplit):
  16-bit path   c * 2^-24 * S                    (products of bf16 values are exact in fp32: only the additions round)
  fp32 path     (2^-16 + c * 2^-24) * S          (2^-16: the split-bf16 x 3 product, see test_gpu_fp32_kernels.py)
c = the longest chain of fp32 additions behind an element, read from the kernels: pixels per tile (x 3 MFMAs per k-step on the fp32
path) x tiles per slice + 3 (folds across waves) + ceil(ksplit / 4) + 5 (the reduce).  ASSUMPTION: the accumulation order inside one
MFMA is not documented; each MFMA is counted as its k-depth (16) of sequential roundings, the worst case.
A reference-side tie from double rounding (float64 fma, then fp32) has probability about 2^-29 per input element; at most one dW
element per case may exceed the bound for it, and the case prints it.
Measured worst err / bound per family: DESIGN.md, "Weight-gradient error bound"."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _wgrad_cases as wc  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS = ['c2-3x3-plain-sweep', 'c2-3x3-fast-res', 'c2-3x3-gen-affine', 'c2-3x3-fast-ragged', 'c1-3x3-kq-fast', 'c1-3x3-fast-res',
        'c2-3x3-pool-ceil', 'c4-3x3-gen-res', 'c4-3x3-plain-sweep', 'c2-3x3-concat', 'c1-T4-plain', 'c2-s2-plain', 'c2-qm-conv3-32x32-xf0',
        'c2-qm-conv1-64x32-xf1', 'c2-qm-conv3-32x64-xf2', 'c2-qm-convT4-64x32', 'c2-qm-convT2-32x32', 'c4-T4']
_RUNS = [(cid, p) for cid in ROWS for p in ('16', '32') if (wc.CASE_BY_ID[cid].form16 if p == '16' else wc.CASE_BY_ID[cid].form32)]


@pytest.mark.parametrize('cid,prec', _RUNS, ids=['%s-%s' % r for r in _RUNS])
def test_wgrad_within_derived_bound(cid, prec):
    import torch
    case = wc.CASE_BY_ID[cid]
    data = wc.make_data(case, 'real')
    dw, sabs = wc.ref_dw(case, data, prec)
    want, sabs = wc.real_dw(case, dw), wc.real_dw(case, sabs)
    srcs, g = wc.device_sources(case, data, prec)
    forms = case.form16 if prec == '16' else case.form32
    sent = torch.full(want.shape, wc.SENTINEL, dtype=torch.float32)
    for ksplit in case.ksplits:
        for i in range(len(srcs)):
            buf = wc.DwBuffer(want.shape)
            f, _, _ = wc.launch(case, srcs, g, i, ksplit, buf)
            got, slack_ok = buf.read()
            assert f == forms[i], (wc.form_str(f), wc.form_str(forms[i]))
            own = wc.owned(case, i)
            assert slack_ok and torch.equal(got[~own], sent[~own]), 'wrote elements of dW the call does not own'
            bnd = wc.bound(f & 15, case.shape, ksplit, sabs)
            err = (got.double() - want).abs()
            ratio = torch.where(own & (bnd > 0), err / bnd.clamp_min(1e-300), torch.zeros_like(err))
            assert bool(torch.isfinite(got[own]).all())
            assert bool((err[own & (bnd == 0)] == 0).all())
            print('WGRAD_BOUND %s prec %s ksplit %d source %d %s c %d worst err/bound %.4f' % (
                cid, prec, ksplit, i, wc.form_str(f), wc.chain_length(f & 15, case.shape, ksplit), float(ratio.max())))
            over = torch.nonzero(ratio > 1.0)
            for ix in over[:4]:
                ix = tuple(ix.tolist())
                print('  over the bound at %s: got %r want %r bound %r' % (ix, float(got[ix]), float(want[ix]), float(bnd[ix])))
            assert len(over) <= 1, '%d elements over the bound, worst ratio %.3f' % (len(over), float(ratio.max()))
