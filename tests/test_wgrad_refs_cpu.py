"""CPU-side checks of tests/_wgrad_cases.py (no GPU): the float64 weight-gradient reference equals PyTorch autograd for every layer kind
and source form of the table, every lattice row stays in the exact regime, the numpy restatement of the split-K reduce maps every mode
onto the PyTorch weight layout, and the table reaches every kernel instantiation the dispatch can."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _wgrad_cases as wc  # noqa: E402


def _autograd_dw(case, A, G):
    """dW of the layer through autograd of the forward op (A: logical input, float64)"""
    shape = wc.dw_shape(case) if case.kind == 'conv3s2' else None
    if case.kind in ('conv3', 'conv1'):
        k = 3 if case.kind == 'conv3' else 1
        w = torch.zeros((case.Cout, A.shape[1], k, k), dtype=torch.float64, requires_grad=True)
        F.conv2d(A, w, None, padding=k // 2).backward(G)
    elif case.kind == 'conv3s2':
        w = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
        F.conv2d(A, w, None, stride=2, padding=1).backward(G)
    elif case.kind == 'convT4':
        w = torch.zeros((A.shape[1], case.Cout, 4, 4), dtype=torch.float64, requires_grad=True)
        F.conv_transpose2d(A, w, None, stride=2, padding=1).backward(G)
    else:
        w = torch.zeros((A.shape[1], case.Cout, 2, 2), dtype=torch.float64, requires_grad=True)
        F.conv_transpose2d(A, w, None, stride=2).backward(G)
    return w.grad


def _torch_input(case, data, prec):
    """the layer's logical input rebuilt with PyTorch ops in the forward order (affine, residual add, ReLU, storage rounding, max-pool,
    F.pad, torch.cat) - independent of _wgrad_cases.logical_input's placement code"""
    N, H, W = case.shape
    r = wc.rounded(data, case, prec)
    parts = []
    for s, d in zip(case.srcs, r['src']):
        t = d['x']
        if d['scale'] is not None:
            t = t * d['scale'].view(1, -1, 1, 1) + d['shift'].view(1, -1, 1, 1)
        if d['res'] is not None:
            t = t + d['res']
        if s.relu:
            t = F.relu(t)
        if prec == '16':
            t = t.bfloat16().double()
        if s.pool:
            t = F.max_pool2d(t, 2, ceil_mode=s.pool == 2)
        if case.kind != 'conv3s2':
            oy, ox = s.off
            t = F.pad(t, (ox, W - ox - t.shape[3], oy, H - oy - t.shape[2]))      # (negative pads crop)
        parts.append(t)
    return torch.cat(parts, 1), r['g']


_RUNS = wc.runs()


@pytest.mark.parametrize('run', _RUNS, ids=['%s-%s-%s' % (c.id, p, lat) for c, p, lat in _RUNS])
def test_reference_equals_autograd_and_stays_exact(run):
    """lattice data: the float64 reference EQUALS autograd's float64 dW (both exact), and the exactness guard holds"""
    case, prec, lat = run
    data = wc.make_data(case, lat)
    dw, sabs = wc.ref_dw(case, data, prec)
    wc.guard(case, data, prec, dw, sabs)
    A, G = _torch_input(case, data, prec)
    want = _autograd_dw(case, A, G)
    assert torch.equal(dw, want)
    assert float(dw.abs().max()) > 0
    assert tuple(wc.real_dw(case, dw).shape) == tuple(wc.dw_shape(case))
    own = sum(wc.owned(case, i).long() for i in range(len(wc.layer_channels(case)[0])))
    assert int(own.min()) == 1 and int(own.max()) == 1          # the sources' calls partition dW


@pytest.mark.parametrize('cid', ['c2-3x3-concat', 'c2-3x3-concat-pool', 'c1-T4-kq-fast', 'c2-qm-convT2-64x32', 'c1-s2-kq', 'c4-3x3-pool-ceil'])
def test_real_valued_reference_close_to_autograd(cid):
    """real-valued data: the reference (with the kernels' rounding points) agrees with autograd over the same rounded input to float64
    rounding, and with autograd over the unrounded transform to the rounding of the path (bf16: 2^-8 per term)"""
    case = wc.CASE_BY_ID[cid]
    for prec in ('16', '32'):
        if (case.form16 if prec == '16' else case.form32) is None:
            continue
        data = wc.make_data(case, 'real')
        dw, sabs = wc.ref_dw(case, data, prec)
        A = wc.logical_input(case, wc.rounded(data, case, prec), prec)
        want = _autograd_dw(case, A, wc.rounded(data, case, prec)['g'])
        assert float(((dw - want).abs() / (sabs + 1e-300)).max()) < 2.0 ** -40
        A2, G2 = _torch_input(case, data, prec)                  # fp32 intermediate roundings left out: within 2^-8 (2^-22) per term
        want2 = _autograd_dw(case, A2, G2)
        eps = 2.0 ** -8 if prec == '16' else 2.0 ** -21
        assert float(((dw - want2).abs() - eps * sabs).max()) <= 0


def test_guard_rejects_a_row_outside_the_exact_regime():
    case = wc.CASE_BY_ID['c2-3x3-plain-sweep']
    data = wc.make_data(case, 'L0')
    data['g'] = data['g'] * 2.0 ** 16
    dw, sabs = wc.ref_dw(case, data, '32')
    with pytest.raises(AssertionError):
        wc.guard(case, data, '32', dw, sabs)
    data = wc.make_data(case, 'L0')
    data['src'][0]['x'] = data['src'][0]['x'] + 0.25            # off the lattice
    dw, sabs = wc.ref_dw(case, data, '32')
    with pytest.raises(AssertionError):
        wc.guard(case, data, '32', dw, sabs)


def _view_inputs(case, A):
    """the two row-parity space-to-depth views of the stride-2 form: view a, channel b * Cp + c, pixel (y, x) = input (c, 2y + a, 2x + b)"""
    return [torch.cat([A[:, :, a::2, b::2] for b in (0, 1)], 1) for a in (0, 1)]


@pytest.mark.parametrize('cid,ci_t', [('c2-3x3-concat', 2), ('c2-3x3-stem', 1), ('c1-1x1-plain', 4), ('c1-T4-plain', 2), ('c1-T4-kq-fast', 1),
                                      ('c1-T2-plain', 4), ('c2-qm-convT2-40x40', 2), ('c1-s2-kq', 1), ('c2-s2-plain', 2), ('c4-s2', 4)])
def test_reduce_restatement_maps_every_mode_onto_the_pytorch_layout(cid, ci_t):
    """slab built from the kernels' definition (emulate_slab), split into slices, summed and scattered by the numpy restatement ==
    autograd's dW; elements no source owns stay untouched; no dW element is written twice"""
    case = wc.CASE_BY_ID[cid]
    data = wc.make_data(case, 'L0')
    dw, _ = wc.ref_dw(case, data, '16')
    want = wc.real_dw(case, dw)
    r = wc.rounded(data, case, '16')
    A = wc.logical_input(case, r, '16')
    taps, npar, ostride, mode = wc.KINDS[case.kind]
    Cs, coffs, real, cin_real = wc.layer_channels(case)
    CI, CO = ci_t * 32, (4 // ci_t) * 32
    inputs = _view_inputs(case, A) if case.kind == 'conv3s2' else list(torch.split(A, Cs, 1))
    flat = np.full(int(np.prod(wc.dw_shape(case))), np.float32(wc.SENTINEL), dtype=np.float32)
    rng = np.random.default_rng(1)
    for i, Ai in enumerate(inputs):
        slab = wc.emulate_slab(case.kind, Ai, r['g'], CI, CO).numpy()
        parts = rng.integers(-4, 5, size=(3, slab.size)).astype(np.float64)          # three slices that sum to the slab
        parts[2] = slab - parts[0] - parts[1]
        idx = wc.scatter_index(mode, npar, -(-Cs[i] // CI), -(-case.Cout // CO), taps, CI, CO, real[i], cin_real, coffs[i], case.Cout)
        live = idx[idx >= 0]
        assert len(np.unique(live)) == len(live)
        mask = np.zeros(flat.size, dtype=bool)
        mask[live] = True
        assert np.array_equal(mask, wc.owned(case, i).numpy().reshape(-1))           # exactly the elements the call owns
        flat = wc.reduce_ref(parts.astype(np.float32), idx, flat)
    assert np.array_equal(flat.reshape(wc.dw_shape(case)), want.numpy().astype(np.float32))


def test_table_reaches_every_reachable_form():
    """the expected forms of the table rows, with the documented exceptions, are every instantiation the dispatch can take"""
    table = wc.table_forms()
    missing = sorted(wc.REACHABLE - table - set(wc.NOT_COVERED))
    assert not missing, [wc.form_str(f) for f in missing]
    stale = sorted(set(wc.NOT_COVERED) & table)
    assert not stale, [wc.form_str(f) for f in stale]
    assert table <= wc.REACHABLE, [wc.form_str(f) for f in sorted(table - wc.REACHABLE)]
    assert set(wc.NOT_COVERED) <= wc.REACHABLE
    # every kind x ci_tiles x precision, every split regime of the prefetch pipelines
    for kind in wc.KINDS:
        for ci_t in (1, 2, 4):
            rows = [c for c in wc.CASES if c.kind == kind and c.ci_t == ci_t]
            assert any(c.form16 for c in rows) and any(c.form32 for c in rows), (kind, ci_t)
    for fam in (wc.GEN, wc.WS, wc.F32K, wc.WS32):
        th = 4 if fam == wc.WS32 else 8
        seen = set()
        for c in wc.CASES:
            for fs in (c.form16, c.form32):
                if fs and fs[0] & 15 == fam:
                    N, H, W = c.shape
                    nt = N * -(-H // th) * -(-W // 16)
                    for k in c.ksplits:
                        seen |= {min(6, (nt - ks + k - 1) // k if ks < nt else 0) for ks in range(k)}
        assert seen >= {0, 1, 2, 3, 4, 6}, (fam, seen)


def test_chain_length_counts():
    assert wc.chain_length(wc.WS, (1, 8, 16), 1) == 128 + 3 + 1 + 5
    assert wc.chain_length(wc.WS32, (3, 17, 33), 7) == 3 * 64 * 7 + 3 + 2 + 5
