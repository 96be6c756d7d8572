"""Exact per-element tests of csrc/dam_loss.hip, csrc/mask_loss.hip and csrc/loss_util.h against the float64 reference of
tests/_loss_exact_cases.py (its docstring has the reference, the data families and the derivation of every bound).

Per row: the entry runs into sentinel-filled outputs and a NaN-filled workspace (every element written, the slack around every buffer and
behind the workspace untouched); the `single` flags, the per-sample sums and the coefficient block are read out of the workspace through
ws_layout and, with the 11 / 8 losses and every gradient element, held to the reference: == where the family makes the value exact, err <=
the derived bound elsewhere.  A row with every term on runs cdnet_dam_loss_classes (and cdnet_dam_loss for 9 classes) as well, each against
the reference, not against the other entry.  The call without gradient pointers gives the same `losses` bits and leaves the gradient
buffers alone.  Then the argument and label edges."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _loss_exact_cases as lx  # noqa: E402

pytestmark = pytest.mark.gpu

_WORST = {}


def _run_and_compare(row, dc, entry, ref, bd, report):
    from cdnet_amd import _lib
    run = lx.Run(row, dc, entry)
    assert run.rc == 0, '%s (%s): refused: %s' % (row.id, entry, run.err)
    got = run.read()
    lx.compare(row, got, ref, bd, report)
    if row.entry == 'dam':                                             # the partial rows add up to the summed rows, within the sums' bound
        q, i = lx.worst(np.abs(got['partial'].sum(1) - ref['sums']), bd['sums'])
        assert q <= 1.0, lx.describe(row, 'sums', got['partial'].sum(1), ref['sums'], i, bd['sums']) + ' (partial rows)'
    if row.entry == 'val':
        return
    # value-only call: the same bits in `losses`, the gradient buffers' sentinels intact
    again = lx.Run(row, dc, entry, grads=False)
    assert again.rc == 0, _lib.load().cdnet_last_error()
    got2 = again.read(grads=False)
    assert np.array_equal(got2['losses'].astype(np.float32).view(np.int32), got['losses'].astype(np.float32).view(np.int32)), \
        '%s (%s): losses without gradient pointers %s, with %s' % (row.id, entry, got2['losses'].tolist(), got['losses'].tolist())


@pytest.mark.parametrize('row', lx.ROWS, ids=[r.id for r in lx.ROWS])
def test_row(row):
    ref, bd = lx.guard(row)                                           # before any GPU call
    dc = lx.DeviceCase(row, lx.make_data(row))
    report = {}
    entries = {'mask': ['mask'], 'val': ['val']}.get(row.entry) or \
        ['terms'] + (['classes'] + (['plain'] if row.ND == 9 else []) if row.terms == lx.FULL else [])
    for entry in entries:
        _run_and_compare(row, dc, entry, ref, bd, report)
    _WORST[row.id] = report
    print('\n%s [%s]: worst err / bound: %s' % (row.id, ', '.join(entries), ', '.join('%s %.3g' % kv for kv in sorted(report.items()))))


def test_worst_ratios():
    """the largest err / bound per entry and quantity over the rows that ran (the figures DESIGN.md quotes)"""
    worst = {}
    for rid, rep in _WORST.items():
        for k, q in rep.items():
            key = (lx.ROW_BY_ID[rid].entry, k)
            if q >= worst.get(key, (-1, ''))[0]:
                worst[key] = (q, rid)
    for key in sorted(worst):
        print('%s %s: %.3g (%s)' % (key + worst[key]))
    assert all(q <= 1.0 for q, _ in worst.values())


# ----------------------------------------------------------------------------------------------------------------------------------
# argument edges: the argument error, no output touched
# ----------------------------------------------------------------------------------------------------------------------------------
_EDGE_ROWS = dict(dam=lx.ROW_BY_ID['dam-R-2x24x20-nd9-q1-t7'], mask=lx.ROW_BY_ID['mask-R-2x24x20-t7'], val=lx.ROW_BY_ID['val-R-2x24x20-nd9-rank'])
_ENTRY = dict(dam='classes', mask='mask', val='val')


_EDGES = [(k, e) for k in ('dam', 'mask', 'val') for e in ('B=65', 'workspace one float short')] + \
         [('dam', 'only dmask'), ('dam', 'only dpoint'), ('dam', 'only ddir')]


@pytest.mark.parametrize('kind,edge', _EDGES, ids=['%s: %s' % e for e in _EDGES])
def test_argument_edges(kind, edge):
    row = _EDGE_ROWS[kind]
    dc = lx.DeviceCase(row, lx.make_data(row))
    if edge == 'B=65':
        run = lx.Run(row, dc, _ENTRY[kind], B=65)                      # (refused before anything is read: the buffers hold 2 samples)
    elif edge.startswith('workspace'):
        run = lx.Run(row, dc, _ENTRY[kind], ws_floats=lx.query(row) - 1)
    else:
        run = lx.Run(row, dc, _ENTRY[kind], only={edge.split()[1]})
    assert run.rc in (1, 2) and run.err, (kind, edge, run.rc, run.err)
    assert run.rc == 1 or edge.startswith('workspace'), (kind, edge, run.rc)
    assert run.untouched() is None, '%s, %s: the refused call wrote %s' % (kind, edge, run.untouched())


# ----------------------------------------------------------------------------------------------------------------------------------
# label edges: out-of-range content poisons every reported value; the flag is clear again on the next valid call
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,what', [('dam', 'label'), ('dam', 'direction'), ('mask', 'label')])
def test_label_edges(kind, what):
    import torch
    from cdnet_amd import _lib
    row = _EDGE_ROWS[kind]
    d = lx.make_data(row)
    ref, bd = lx.guard(row)
    lab, dl = d['lab'].copy(), d['dl'].copy()
    if what == 'label':
        lab[1, 77] = 3
    else:
        dl[0, 123] = row.ND
    bad, good = lx.DeviceCase(row, d, lab=lab, dl=dl), lx.DeviceCase(row, d)
    run = lx.Run(row, bad, _ENTRY[kind])
    assert run.rc == 0, run.err
    losses, ok = run.losses.read()
    assert ok and np.isnan(losses).all(), '%s with a %s out of range: losses %s' % (kind, what, losses.tolist())
    for k, b in run.outputs().items():                                 # indices are clamped: everything is written in bounds
        if k not in ('ws', 'losses'):
            x, ok = b.read()
            assert ok and not (x == b.sent).any() and np.isfinite(x).all(), k
    assert run.ws.read()[1]
    # the same workspace, valid labels: the flag is cleared by the call itself and every value is back inside its bound
    lib = _lib.load()
    (B, H, W), ND = row.shape, row.ND
    out = lx.Run(row, good, _ENTRY[kind])                              # (fresh outputs to compare against)
    st, p = _lib.stream_ptr(), lx._p
    losses2 = lx.OutBuffer((11 if kind == 'dam' else 8,))
    if kind == 'dam':
        rc = lib.cdnet_dam_loss_classes(p(good.lm), p(good.lp), p(good.ld), p(good.lab), p(good.dl), p(good.pt), p(good.wt), B, H, W, ND, row.quirk,
                                        run.ws.ptr(), lx.query(row), losses2.ptr(), None, None, None, st)
    else:
        rc = lib.cdnet_mask_loss(p(good.lm), p(good.lab), p(good.wt), B, H, W, row.terms, run.ws.ptr(), lx.query(row), losses2.ptr(), None, st)
    torch.cuda.synchronize()
    assert rc == 0, lib.cdnet_last_error()
    got, ok = losses2.read()
    assert ok and np.array_equal(got, out.losses.read()[0]), (got.tolist(), out.losses.read()[0].tolist())
    lx.compare(row, dict(losses=got), ref, bd)
    ints = run.ws.t.view(torch.int32).cpu().numpy()
    assert ints[run.lay['pad']] == 0
