"""Exact per-element tests of cdnet_conv_backward_weight (csrc/wgrad.hip): every dispatch form, both precisions, bit equality.

The inputs sit on the lattices of tests/_wgrad_cases.py, so every partial sum is exactly representable in fp32 and the result must EQUAL
the float64 reference whatever the summation order, the split factor or the kernel form: nothing here carries a tolerance.  dW starts
from a sentinel inside a larger buffer (elements the call does not own - other sources' channels, padded channels, the slack on both ends
- must still hold it), the slab starts from NaN (a slice without tiles must write zeros), and every launch asserts the kernel
instantiation it took (cdnet_conv_backward_weight_last_form)."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _wgrad_cases as wc  # noqa: E402

pytestmark = pytest.mark.gpu

_RUNS = wc.runs()
_IDS = ['%s-%s-%s' % (c.id, p, lat) for c, p, lat in _RUNS]


def _prepared(run):
    """(expected dW fp32, device sources, device gradient) of a run: computed once per run, shared by its split factors and sources,
    never modified"""
    import torch
    case, prec, lat = run
    data = wc.make_data(case, lat)
    dw, sabs = wc.ref_dw(case, data, prec)
    wc.guard(case, data, prec, dw, sabs)                           # before any GPU call
    srcs, g = wc.device_sources(case, data, prec)
    return wc.real_dw(case, dw).to(torch.float32), srcs, g


def _diff(case, got, exp):
    import torch
    bad = torch.nonzero(got != exp)
    rows = ['%s: got %r want %r' % (tuple(i.tolist()), float(got[tuple(i)]), float(exp[tuple(i)])) for i in bad[:8]]
    return '%s: %d of %d elements differ\n  ' % (case.id, len(bad), got.numel()) + '\n  '.join(rows)


@pytest.mark.parametrize('run', _RUNS, ids=_IDS)
def test_wgrad_exact(run):
    import torch
    case, prec, lat = run
    want, srcs, g = _prepared(run)
    forms = case.form16 if prec == '16' else case.form32
    sent = torch.full(want.shape, wc.SENTINEL, dtype=torch.float32)
    for ksplit in case.ksplits:
        for i in range(len(srcs)):
            buf = wc.DwBuffer(want.shape)
            f, slab, _ = wc.launch(case, srcs, g, i, ksplit, buf)
            got, slack_ok = buf.read()
            assert f == forms[i], '%s ksplit %d source %d: ran %s, the row expects %s' % (case.id, ksplit, i, wc.form_str(f), wc.form_str(forms[i]))
            exp = torch.where(wc.owned(case, i), want, sent)
            assert slack_ok, '%s ksplit %d source %d: wrote outside dW' % (case.id, ksplit, i)
            assert torch.equal(got, exp), 'ksplit %d source %d (%s) ' % (ksplit, i, wc.form_str(f)) + _diff(case, got, exp)


_CHUNK = 13
_CHUNKS = [_RUNS[i:i + _CHUNK] for i in range(0, len(_RUNS), _CHUNK)]


@pytest.mark.parametrize('chunk', _CHUNKS, ids=['%s..%s' % (_IDS[i], _IDS[min(i + _CHUNK, len(_IDS)) - 1]) for i in range(0, len(_RUNS), _CHUNK)])
def test_wgrad_exact_deferred_reduce(chunk):
    """the same rows with CDNET_WGRAD_DEFER_REDUCE: the calls leave dW alone, then ONE cdnet_wgrad_reduce_batch over all their slabs
    (every source of every row of the chunk: descriptors of unequal block counts) gives the reference"""
    import torch
    jobs, args, keep = [], [], []
    for n, run in enumerate(chunk):
        case, prec, lat = run
        want, srcs, g = _prepared(run)
        ksplit = case.ksplits[n % len(case.ksplits)]
        buf = wc.DwBuffer(want.shape)
        forms = case.form16 if prec == '16' else case.form32
        for i in range(len(srcs)):
            f, slab, a = wc.launch(case, srcs, g, i, ksplit, buf, defer=True)
            assert f == forms[i], (case.id, wc.form_str(f), wc.form_str(forms[i]))
            args.append(a)
            keep.append((slab, srcs, g))
        got, slack_ok = buf.read()
        assert slack_ok and torch.equal(got, torch.full(want.shape, wc.SENTINEL, dtype=torch.float32)), case.id + ': the deferred call wrote dW'
        jobs.append((case, buf, want))
    wc.reduce_batch(args)
    for case, buf, want in jobs:
        got, slack_ok = buf.read()
        assert slack_ok, case.id
        assert torch.equal(got, want), _diff(case, got, want)


def test_refused_sources():
    """fp32 pooled sources and pooled sources with a residual branch are refused before any launch"""
    import torch
    from cdnet_amd import _lib, engine
    lib = _lib.load()
    N, H, W, Cc, Cout = 1, 8, 16, 32, 32
    slab = torch.zeros((lib.cdnet_conv_wgrad_slab_floats(Cc, Cout, 9, 1, 2, 1),), dtype=torch.float32, device='cuda')
    dw = torch.full((Cout, Cc, 3, 3), wc.SENTINEL, dtype=torch.float32, device='cuda')
    for dt, res, word in ((torch.float32, False, b'fp32 pooled'), (torch.bfloat16, True, b'residual'), (torch.float32, True, b'pooled')):
        x = torch.zeros((N, 2 * H, 2 * W, Cc), dtype=dt, device='cuda')
        g = torch.zeros((N, H, W, Cout), dtype=dt, device='cuda')
        s = engine.Src(x, pool=1, res=x.clone() if res else None)
        cs = engine.ConvSrc()
        s.fill(cs)
        rc = lib.cdnet_conv_backward_weight(C.byref(cs), 0, Cc, Cc, _lib.ptr(g), Cout, N, H, W, 9, 1, 1, 2, 1, _lib.ptr(slab), _lib.ptr(dw), 0,
                                            _lib.stream_ptr())
        assert rc != 0 and word in lib.cdnet_last_error(), (rc, lib.cdnet_last_error())
    torch.cuda.synchronize()
    assert torch.equal(dw.cpu(), torch.full((Cout, Cc, 3, 3), wc.SENTINEL, dtype=torch.float32))
