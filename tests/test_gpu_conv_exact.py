"""Exact per-element tests of cdnet_conv_forward (csrc/conv.hip, conv16ws.hip, conv32.hip, conv32ws.hip): every dispatch form, both
precisions, forward, transposed and backward-data, bit equality.

The data sit on the lattices of tests/_conv_cases.py, so every product and partial sum is exactly representable in fp32 and the stored
output must EQUAL the float64 reference (rounded once to the output's type) whatever the tile, the chunk order, the hi / lo split or the
kernel form: nothing here carries a tolerance.  The output starts from a sentinel inside a larger buffer (channels outside the slice
and the slack on both ends must still hold it), the statistics rows start from NaN, and every launch asserts the kernel instantiation
it took (cdnet_conv_forward_last_form)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _conv_cases as cc  # noqa: E402

pytestmark = pytest.mark.gpu

_RUNS = cc.runs()
_IDS = ['%s-%s' % (r.id, lat) for r, lat in _RUNS]
_PREPARED = {}


def _prepared(run):
    """(reference, device arguments) of a run: computed once, shared by the tests that need it, never modified"""
    row, lat = run
    key = (row.id, lat)
    if key not in _PREPARED:
        data = cc.make_data(row, lat)
        ref = cc.reference(row, data)
        cc.guard(row, data, ref)                                     # before any GPU call
        _PREPARED.clear()                                            # (one run's tensors at a time)
        _PREPARED[key] = (ref, cc.device_args(row, data))
    return _PREPARED[key]


def _diff(row, got, exp):
    import torch
    bad = torch.nonzero(got != exp)
    rows = ['%s: got %r want %r' % (tuple(i.tolist()), float(got[tuple(i)]), float(exp[tuple(i)])) for i in bad[:8]]
    return '%s: %d of %d elements differ ([n][y][x][c])\n  ' % (row.id, len(bad), got.numel()) + '\n  '.join(rows)


def _check(row, ref, res, what):
    import torch
    assert res['form'] == row.form, '%s %s: ran %s, the row expects %s' % (row.id, what, cc.form_str(res['form']), cc.form_str(row.form))
    got, slack_ok = res['out'].read()
    assert slack_ok, '%s %s: wrote outside the output tensor' % (row.id, what)
    exp = torch.full(got.shape, cc.SENTINEL, dtype=got.dtype)
    exp[..., row.coff:row.coff + row.Cout] = ref['out']
    assert torch.equal(got, exp), '%s (%s) ' % (what, cc.form_str(res['form'])) + _diff(row, got, exp)
    if row.pool_out:
        gp, slack_ok = res['pool'].read()
        assert slack_ok, '%s %s: wrote outside the pooled output' % (row.id, what)
        assert torch.equal(gp, ref['pool']), '%s pool_out ' % what + _diff(row, gp, ref['pool'])
    if row.stats:
        st = res['stats'].double().cpu()
        assert not torch.isnan(st).any(), '%s %s: %d statistics entries were not written' % (row.id, what, int(torch.isnan(st).sum()))
        cols = st.sum(0)
        assert torch.equal(cols[0], ref['ssum']), '%s %s: sum acc: got %r want %r' % (row.id, what, cols[0].tolist(), ref['ssum'].tolist())
        assert torch.equal(cols[1], ref['ssq']), '%s %s: sum acc^2: got %r want %r' % (row.id, what, cols[1].tolist(), ref['ssq'].tolist())


@pytest.mark.parametrize('run', _RUNS, ids=_IDS)
def test_conv_exact(run):
    row, lat = run
    ref, dargs = _prepared(run)
    res = cc.launch(row, dargs, row.debug | (row.cap << 8 if row.persistent else 0))
    _check(row, ref, res, 'cap %d' % row.cap if row.persistent else 'launch')


_PERSISTENT = [(r, lat) for r, lat in _RUNS if r.persistent and lat == r.lattices[0]]


@pytest.mark.parametrize('run', _PERSISTENT, ids=['%s-%s' % (r.id, lat) for r, lat in _PERSISTENT])
def test_conv_exact_grid_caps(run):
    """every row of the persistent kernels with one and two workgroups per output-channel tile (all tiles in one run; two runs whose odd /
    even tile_step pairs and serial last epilogues differ) and with the default grid: equal bits among them and with the reference"""
    import torch
    row, lat = run
    ref, dargs = _prepared(run)
    outs = []
    for cap in (1, 2, 0):
        res = cc.launch(row, dargs, row.debug | (cap << 8))
        _check(row, ref, res, 'cap %d' % cap)
        outs.append(res['out'].read()[0])
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_refusals():
    """launches no kernel serves: each returns non-zero with its message, leaves the sentinel-filled output untouched and the form record as it was"""
    import torch
    from cdnet_amd import _lib, engine
    lib = _lib.load()
    cases = [
        # a one-tap second source where no producer / consumer kernel is eligible (the one-tile kernels only)
        ('ws16-bn64-xf0-pair-mix', dict(debug=cc.ONE_TILE), 'one-tap second source'),
        ('ws32-mix-bn64-xf0', dict(debug=cc.ONE_TILE), 'one-tap second source'),
        # pool_out off the out-image form (an odd chunk count: direct stores) and off conv_ws32_kernel
        ('ws16-pool-out-pair', dict(debug=cc.ONE_TILE), 'max-pool'),
        ('ws16-bn32-xf0-direct', dict(pool_out=True, orelu=True), 'max-pool'),
        ('ws32-pool', dict(debug=cc.ONE_TILE), 'max-pool'),
        # a padding chunk on the one-tile kernel
        ('ws16-pad-chunk-pair', dict(debug=cc.ONE_TILE), 'padding chunk'),
        # Cout not a multiple of 8
        ('fwd-conv3-t16-ck16-bn32', dict(Cout=12), 'multiple of 8'),
    ]
    import dataclasses
    for rid, change, word in cases:
        row = dataclasses.replace(cc.ROW_BY_ID[rid], **{k: v for k, v in change.items() if k != 'Cout'})
        data = cc.make_data(row, row.lattices[0])
        dargs = cc.device_args(row, data)
        if 'Cout' in change:                                         # (the pack and the vectors keep the row's size: nothing is read)
            row = dataclasses.replace(row, Cout=change['Cout'], cstride=16)
        before = lib.cdnet_conv_forward_last_form()
        bufs = cc.make_buffers(row)
        with pytest.raises(_lib.CdnetHipError) as e:
            cc.launch(row, dargs, row.debug, bufs)
        assert word in str(e.value), (rid, str(e.value))
        assert lib.cdnet_conv_forward_last_form() == before, rid
        torch.cuda.synchronize()
        for o in (bufs['out'], bufs['pool']):
            if o is not None:
                got, slack_ok = o.read()
                assert slack_ok and torch.equal(got, torch.full(got.shape, cc.SENTINEL, dtype=got.dtype)), rid + ': a refused launch wrote its output'
    # an fp32 pooled source (must be materialised first)
    x = torch.zeros((1, 32, 32, 16), dtype=torch.float32, device='cuda')
    wp = engine.pack_weights(torch.zeros((16, 16, 3, 3), dtype=torch.float32, device='cuda'), (16, 16, 32), 0, split=True)
    out = cc.OutBuffer((1, 16, 16, 16), torch.float32)
    with pytest.raises(_lib.CdnetHipError) as e:
        engine.conv_forward([engine.Src(x, pool=1)], wp, 16, (16, 16, 32), out=out.t, H=16, W=16)
    assert 'pooled' in str(e.value)
    torch.cuda.synchronize()
    got, slack_ok = out.read()
    assert slack_ok and torch.equal(got, torch.full(got.shape, cc.SENTINEL, dtype=torch.float32))
