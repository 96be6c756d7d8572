"""Exact per-element tests of csrc/bn_bwd.hip: every instantiation its launch plan can produce, both passes, against the float64
reference of tests/_bn_exact_cases.py (its docstring has the definition, the lattices and the derivation of every bound).

Per row: the plan record of both passes (cdnet_bn_backward_last_plan / _last_sums_plan), sentinels (every element of dRaw and dz written,
the slack around them, the workspace behind the nb partial rows and the coefficients untouched, NaN wherever a correct kernel does not
read a gradient source), then dz, dbeta, dgamma, the partial rows' column sums and k1 .. k3 with == on the lattice rows and dRaw within
the derived bound; the random rows bound the sums.  The split entries are checked against the same reference, not against the fused call."""
import ctypes as C
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bn_exact_cases as bx  # noqa: E402

pytestmark = pytest.mark.gpu

_REACHED = {}


@pytest.mark.parametrize('row', bx.ROWS, ids=[r.id for r in bx.ROWS])
def test_row(row):
    from cdnet_amd import _lib
    d = bx.make_data(row)
    ref = bx.reference(row, d)
    bx.guard(row, d, ref)                                            # before any GPU call
    report = bx.check_row(row, d, ref)
    lib = _lib.load()
    _REACHED[row.id] = [p for p in ((lib.cdnet_bn_backward_last_sums_plan() if row.bn else None), lib.cdnet_bn_backward_last_plan()) if p]
    print('\n%s: %s; worst err / bound: %s' % (row.id, ' | '.join(bx.plan_str(p) for p in _REACHED[row.id]),
                                             ', '.join('%s %.3g' % kv for kv in sorted(report.items()))))
    if row.shape == bx.K:
        assert all(bx.plan_decode(p)['nb'] == 512 for p in _REACHED[row.id]), row.id


def test_every_instantiation_reached():
    """the rows above and the child process below between them ran all 40 instantiations of `launch` (when the whole file ran)"""
    reached = {bx.instantiation(p) for ps in _REACHED.values() for p in ps}
    assert reached <= bx.all_instantiations()
    if len(_REACHED) == len(bx.ROWS):
        missing = bx.all_instantiations() - reached
        assert missing == {('flat', f, n, 1, 1) for f in (0, 1) for n in (1, 2, 3)}, sorted(missing)


def test_flat_residual_apply_without_dz_reuse():
    """CDNET_BN_DZ_REUSE=0 is read once per process: a child runs the flat rows with a residual of the small shapes; their apply pass
    then reads the sources and the mask again (bn_bwd_flat_kernel<NG, true, true>, the six instantiations no other row reaches)"""
    rows = [r.id for r in bx.ROWS if r.reuse and r.shape != bx.K]
    env = dict(os.environ, CDNET_BN_DZ_REUSE='0')
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), '_bn_exact_worker.py')] + rows,
                       env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    plans = json.loads(p.stdout.strip().splitlines()[-1])
    assert {bx.instantiation(v) for v in plans.values()} == {('flat', f, n, 1, 1) for f in (0, 1) for n in (1, 2, 3)}


# ----------------------------------------------------------------------------------------------------------------------------------
# the split entries against the reference
# ----------------------------------------------------------------------------------------------------------------------------------
def _ktab(Cc):
    import torch
    return bx.OutBuffer((7, Cc), torch.float32)


def _stats(dc, b, ktab, ws_floats=None):
    import torch
    from cdnet_amd import _lib
    rc = _lib.load().cdnet_bn_backward_stats(C.byref(dc.A), dc.gamma_ptr(), b['dgamma'].ptr(), b['dbeta'].ptr(), b['ws'].ptr(),
                                             bx.ws_floats(dc.row.C) if ws_floats is None else ws_floats, ktab.ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _apply(dc, b, ktab):
    import torch
    from cdnet_amd import _lib
    rc = _lib.load().cdnet_bn_backward_apply(C.byref(dc.A), ktab.ptr(), b['draw'].ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _finalize(dc, b, partial, nb, ktab):
    import torch
    from cdnet_amd import _lib
    rc = _lib.load().cdnet_bn_backward_finalize(C.byref(dc.A), dc.gamma_ptr(), b['dgamma'].ptr(), b['dbeta'].ptr(),
                                                C.c_void_p(partial.data_ptr()), nb, ktab.ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _check_draw(row, b, ref):
    got, ok = b['draw'].read()
    assert ok and not (got == b['draw'].sent).any(), row.id + ': dRaw not fully written / written outside'
    q, i = bx.worst(np.abs(got - ref['draw']), bx.draw_bound(row, ref))
    assert q <= 1.0, '%s: err / bound = %.3g; %s' % (row.id, q, bx.describe('draw', got, ref['draw'], i))
    return q


@pytest.mark.parametrize('rid', ['A-flat-f16-ng1-res0', 'A-flat-bf16-ng1-res0', 'K-flat-f16'])
def test_stats_then_apply(rid):
    """cdnet_bn_backward_stats + cdnet_bn_backward_apply: ktab rows 0-3 are the copied vectors, k1 exact, k2 and k3 the correctly
    rounded quotients, dbeta / dgamma exact, dRaw within the bound - all against the float64 reference"""
    from cdnet_amd import _lib
    lib = _lib.load()
    row = bx.ROW_BY_ID[rid]
    d = bx.make_data(row)
    ref = bx.reference(row, d)
    dc, b, ktab = bx.DeviceCase(row, d), bx.make_buffers(row), _ktab(row.C)
    assert _stats(dc, b, ktab) == 0, lib.cdnet_last_error()
    want_sums, want_apply = row.plans()
    assert lib.cdnet_bn_backward_last_plan() == want_sums == lib.cdnet_bn_backward_last_sums_plan(), bx.plan_str(lib.cdnet_bn_backward_last_plan())
    kt, ok = ktab.read()
    assert ok
    for k, name in enumerate(('scale', 'shift', 'mean', 'invstd')):
        assert np.array_equal(kt[k], d[name]), name
    assert np.array_equal(kt[4], ref['k1'])
    assert np.array_equal(kt[5], bx.round_quot(ref['dbeta'], row.M).astype(np.float64))
    assert np.array_equal(kt[6], bx.round_quot(ref['dgamma'], row.M).astype(np.float64))
    for name in ('dbeta', 'dgamma'):
        got, ok = b[name].read()
        assert ok and np.array_equal(got, ref[name]), name
    ws, ok = b['ws'].read()
    assert ok and not (ws[:row.nb * 2 * row.C] == b['ws'].sent).any() and (ws[row.nb * 2 * row.C:] == b['ws'].sent).all()
    got, ok = b['draw'].read()
    assert ok and (got == b['draw'].sent).all(), 'the stats entry wrote dRaw'
    assert _apply(dc, b, ktab) == 0, lib.cdnet_last_error()
    assert lib.cdnet_bn_backward_last_plan() == want_apply and lib.cdnet_bn_backward_last_sums_plan() == want_sums
    print('\n%s stats + apply: worst err / bound draw %.3g' % (rid, _check_draw(row, b, ref)))


@pytest.mark.parametrize('Cc', [8, 48])
@pytest.mark.parametrize('nb', [1, 255, 256, 257, 512, 2048])
def test_finalize_alone(nb, Cc):
    """integer partial rows (|.| < 1000: every sum below 2^24): dbeta and dgamma exact, k2 and k3 the fp32 rounding of the float64
    quotient, rows 0-3 of ktab untouched; 257 and 512 rows take the second trip of the finalize kernel's row loop, 2048 the eighth"""
    import torch
    from cdnet_amd import _lib
    row = bx.Row('finalize', 'f16', bx.B, Cc, ('same',), bx.PATH_FLAT, seed=900 + Cc)
    d = bx.make_data(row)
    dc, b, ktab = bx.DeviceCase(row, d), bx.make_buffers(row), _ktab(Cc)
    rng = np.random.default_rng(nb * 100 + Cc)
    part = rng.integers(-999, 1000, (nb, 2, Cc)).astype(np.float64)
    dev = torch.from_numpy(part.astype(np.float32)).cuda()
    plan = _lib.load().cdnet_bn_backward_last_plan()
    assert _finalize(dc, b, dev, nb, ktab) == 0, _lib.load().cdnet_last_error()
    assert _lib.load().cdnet_bn_backward_last_plan() == plan               # (finalize launches none of the planned kernels)
    s1, s2 = part[:, 0].sum(0), part[:, 1].sum(0)
    kt, ok = ktab.read()
    assert ok and (kt[:4] == ktab.sent).all(), 'rows 0-3 of ktab were written'
    assert np.array_equal(kt[4], d['gamma'] * d['invstd'])
    assert np.array_equal(kt[5], bx.round_quot(s1, row.M).astype(np.float64)) and np.array_equal(kt[6], bx.round_quot(s2, row.M).astype(np.float64))
    got, ok = b['dbeta'].read()
    assert ok and np.array_equal(got, s1)
    got, ok = b['dgamma'].read()
    assert ok and np.array_equal(got, s2)
    assert bx.buffers_untouched(dict(draw=b['draw'], ws=b['ws'])) is None


@pytest.mark.parametrize('rid', ['A-flat-f16-ng1-relu0', 'A-flat-f32-ng1-relu0'])
def test_apply_masked_source(rid):
    """cdnet_bn_backward_apply with relu = 0 (the source went through the ReLU already) over a ktab made from the reference"""
    import torch
    from cdnet_amd import _lib
    row = bx.ROW_BY_ID[rid]
    d = bx.make_data(row)
    ref = bx.reference(row, d)
    dc, b, ktab = bx.DeviceCase(row, d), bx.make_buffers(row), _ktab(row.C)
    kt = np.stack([d['scale'], d['shift'], d['mean'], d['invstd'], ref['k1'], bx.round_quot(ref['dbeta'], row.M), bx.round_quot(ref['dgamma'], row.M)])
    ktab.t.copy_(torch.from_numpy(kt.astype(np.float32)))
    assert _apply(dc, b, ktab) == 0, _lib.load().cdnet_last_error()
    assert _lib.load().cdnet_bn_backward_last_plan() == row.plans()[1]
    print('\n%s apply alone: worst err / bound draw %.3g' % (rid, _check_draw(row, b, ref)))
    assert bx.buffers_untouched(dict(ws=b['ws'], dgamma=b['dgamma'], dbeta=b['dbeta'])) is None


# ----------------------------------------------------------------------------------------------------------------------------------
# refusals
# ----------------------------------------------------------------------------------------------------------------------------------
def _set(**fields):
    def f(dc):
        for k, v in fields.items():
            setattr(dc.A, k, v)
    return f


def _set_gin(k, **fields):
    def f(dc):
        for n, v in fields.items():
            setattr(dc.A.gin[k], n, v)
    return f


_WIDE = bx.Row('wide', 'f16', (1, 2, 2), 2064, ('same',), bx.PATH_FLAT, seed=901)
_WIDE32 = bx.Row('wide32', 'f32', bx.B, 1032, ('same',), bx.PATH_GENERIC, seed=902)
_C16 = bx.Row('c16', 'f16', bx.B, 16, ('same',), bx.PATH_FLAT, seed=903)

# (name, row, entry, change to the filled arguments or to the call, a word of the message)
REFUSALS = [
    ('C=12', _C16, 'fused', _set(C=12), 'unsupported'),
    ('C=2056', _WIDE, 'fused', _set(C=2056), 'unsupported'),
    ('ngin=0', 'A-flat-f16-ng3-res0', 'fused', _set(ngin=0), 'ngin'),
    ('ngin=4', 'A-flat-f16-ng3-res0', 'fused', _set(ngin=4), 'ngin'),
    ('null source', 'A-flat-f32-ng3-res0', 'fused', _set_gin(1, g=None), 'null gradient'),
    ('relu=2 without res', 'A-flat-f16-ng1-res0', 'fused', _set(relu=2), 'relu = 2'),
    ('relu=2 shifted source', 'A-generic-f16-pad+same-res', 'fused', _set(relu=2), 'relu = 2'),
    ('relu=2 shifted source f32', 'A-generic-f32-pad+same-res', 'fused', _set(relu=2), 'relu = 2'),
    ('workspace short', 'A-flat-f16-ng1-res0', 'fused', 'ws', 'workspace'),
    ('workspace short window32', 'A-window-f32-pool2-nf1-kp0-L0', 'fused', 'ws', 'workspace'),
    ('no gamma', 'A-flat-f16-ng1-res0', 'fused', 'gamma', 'gamma'),
    ('empty source window', 'A-window-f16-pool2-nf1-kp0-L0', 'fused', _set_gin(0, Hg=0, pooled=1), 'empty gradient'),
    ('empty source window32', 'A-window-f32-pool2-nf0-kp0-L0', 'fused', _set_gin(0, Wg=0, pooled=1), 'empty gradient'),
    ('apply f32 C=1032', _WIDE32, 'apply', None, '1024'),
    ('stats f32', 'A-flat-f32-ng1-res0', 'stats', None, 'plain'),
]
for _entry in ('stats', 'finalize', 'apply'):
    REFUSALS += [('%s with a residual' % _entry, 'A-flat-f16-ng1-res1', _entry, None, 'plain'),
                 ('%s with a pooled source' % _entry, 'A-window-f16-pool2-nf0-kp0-L0', _entry, None, 'plain'),
                 ('%s with a channel slice' % _entry, 'A-flat-f16-ng3-res0', _entry, _set(ngin=1), 'plain')]


@pytest.mark.parametrize('case', REFUSALS, ids=[c[0] for c in REFUSALS])
def test_refusals(case):
    """calls no kernel serves: a non-zero status with its message, every sentinel-filled buffer untouched, the plan records as they were.
    Every buffer is as large as a launch with the refused arguments would need."""
    import torch
    from cdnet_amd import _lib
    lib = _lib.load()
    name, row, entry, change, word = case
    row = bx.ROW_BY_ID[row] if isinstance(row, str) else row
    d = bx.make_data(row)
    dc, b, ktab = bx.DeviceCase(row, d), bx.make_buffers(row, with_dz=True), _ktab(row.C)
    if not row.res:
        b['dz'] = None                                                   # (dz_out goes with a residual)
    if callable(change):
        change(dc)
    before = (lib.cdnet_bn_backward_last_plan(), lib.cdnet_bn_backward_last_sums_plan())
    if entry == 'fused':
        short = row.nb * 2 * row.C + 3 * row.C - 1 if change == 'ws' else None           # one float less than the plan needs
        rc = bx.run_fused(dc, b, ws_floats_arg=short, gamma=change != 'gamma')
    elif entry == 'stats':
        rc = _stats(dc, b, ktab)
    elif entry == 'apply':
        kt = torch.zeros((7, row.C), dtype=torch.float32)
        kt[4] = 1.0
        ktab2 = _ktab(row.C)
        ktab2.t.copy_(kt)
        rc = _apply(dc, b, ktab2)
    else:
        part = torch.zeros((4, 2, row.C), dtype=torch.float32, device='cuda')
        rc = _finalize(dc, b, part, 4, ktab)
    msg = lib.cdnet_last_error().decode(errors='replace')
    assert rc != 0 and word in msg, (name, rc, msg)
    assert (lib.cdnet_bn_backward_last_plan(), lib.cdnet_bn_backward_last_sums_plan()) == before, name
    b['ktab'] = ktab
    assert bx.buffers_untouched(b) is None, '%s: the refused call wrote %s' % (name, bx.buffers_untouched(b))
