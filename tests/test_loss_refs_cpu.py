"""CPU-side checks of tests/_loss_exact_cases.py: the float64 reference of the loss kernels against float64 autograd of the oracle
(oracle.train.dam_losses on rows whose weights are exact in fp32, the term-word restatement of test_gpu_dam_loss_terms.py /
test_gpu_mask_loss.py elsewhere) and against a float64 transcription of validate()'s loss mix; the guard of every row and the coverage
of the row list; an fp32 numpy emulation of the kernels' summation order inside every bound; and the power of the rows: twelve wrong
variants of the reference, each further from the true one than the bound on a named row.  No GPU.

Worst err / bound of the fp32 emulation over EMULATED (libm's expf / logf, correctly rounded division): see test_emulation_inside_bounds."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _loss_exact_cases as lx  # noqa: E402

WMAP, CE, DICE = lx.WMAP, lx.CE, lx.DICE


def _t(a, row, ch=None):
    import torch
    B, H, W = row.shape
    x = torch.from_numpy(np.array(a))
    return x.reshape((B, H, W) if ch is None else (B, ch, H, W))


def _close(got, want, name, row):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = max(float(np.abs(want).max()), 1e-300)
    err = float(np.abs(got - want).max())
    # (1e-40: the reference takes exp(x <= -104) as 0, as fp32 does; float64 autograd keeps 2.6e-56 at -128)
    assert err <= 1e-12 * scale + 1e-40, '%s: %s differs from autograd by %.3g of its largest element' % (row.id, name, err / scale)


def _restate_dam(row, d, use_dam_losses):
    """train_util_dam.py:167-276 for the row's term word in float64 autograd, composed from the oracle's pieces"""
    import torch
    import torch.nn.functional as F
    from oracle import train as ot
    lm, lp, ld = [_t(d[k], row, c).double().requires_grad_(True) for k, c in (('lm', 3), ('lp', 1), ('ld', row.ND))]
    lab, dirn, pt, wt = _t(d['lab'], row), _t(d['dl'], row), _t(d['pt'], row), _t(d['wt'], row)
    if use_dam_losses:
        with torch.no_grad():                  # (values only: its fp32 weight and target tensors do not differentiate against float64 logits)
            L = ot.dam_losses(lm, lp, ld, lab, dirn, pt, wt, bool(row.quirk))
        return [float(L[k]) for k in ('total', 'dce', 'wdice', 'mse', 'ce', 'dice')], None, None, None, None
    else:
        w = wt.double() / 20 if row.terms & WMAP else torch.ones(lab.shape, dtype=torch.float64)
        label, direction = lab.long(), dirn.long()
        ce = (F.nll_loss(F.log_softmax(lm, 1), label, reduction='none') * w).mean()
        dice = ot.multiclass_dice(F.softmax(lm, 1), F.one_hot(label, 3).permute(0, 3, 1, 2).double())
        dce = (F.nll_loss(F.log_softmax(ld, 1), direction, reduction='none') * w).mean()
        oh = ot.direction_onehot(direction, label, row.ND, bool(row.quirk)).double()
        ddice = ot.weight_multiclass_dice(F.softmax(ld, 1), oh, w) if row.terms & WMAP else ot.multiclass_dice(F.softmax(ld, 1), oh)
        mse = F.mse_loss(lp, pt.double().unsqueeze(1))
        total = dice + dce + ddice + mse
        if row.terms & CE:
            total = ce + total
        vals = [total, dce, ddice, mse, ce, dice]
    vals[0].backward()
    metrics = ot.pixel_metrics(ld.detach().argmax(1).numpy(), dirn.numpy())
    flat = lambda g: g.numpy().reshape(g.shape[0], g.shape[1], -1)
    return [float(v.detach()) for v in vals], metrics, flat(lm.grad), flat(lp.grad)[:, 0], flat(ld.grad)


_DAM = [r for r in lx.ROWS if r.entry == 'dam' and r.P <= 1023]


@pytest.mark.parametrize('row', _DAM, ids=[r.id for r in _DAM])
def test_dam_reference_matches_autograd(row):
    d = lx.make_data(row)
    ref = lx.reference(row, d)
    # oracle.train.dam_losses divides the weight byte in fp32: exact for the bytes of L and T, so there it is the reference itself
    for use in ([False, True] if row.terms == lx.FULL and row.fam != 'R' else [False]):
        vals, metrics, gm, gp, gd = _restate_dam(row, d, use)
        _close(ref['losses'][:6], vals, 'losses', row)
        if use:
            continue
        _close(ref['losses'][6:], metrics, 'metrics', row)
        _close(ref['dmask'], gm, 'dmask', row)
        _close(ref['dpoint'], gp, 'dpoint', row)
        _close(ref['ddir'], gd, 'ddir', row)


_MASK = [r for r in lx.ROWS if r.entry == 'mask' and r.P <= 10752]


@pytest.mark.parametrize('row', _MASK, ids=[r.id for r in _MASK])
def test_mask_reference_matches_autograd(row):
    import torch
    import torch.nn.functional as F
    from oracle import train as ot
    d = lx.make_data(row)
    ref = lx.reference(row, d)
    lm = _t(d['lm'], row, 3).double().requires_grad_(True)
    lab, wt = _t(d['lab'], row), _t(d['wt'], row)
    ce_map = F.nll_loss(F.log_softmax(lm, 1), lab.long(), reduction='none')
    if row.terms & WMAP:
        ce_map = ce_map * (wt.double() / 20)
    ce = ce_map.mean()
    dice = ot.multiclass_dice(F.softmax(lm, 1), F.one_hot(lab.long(), 3).permute(0, 3, 1, 2).double())
    total = (ce if row.terms & CE else 0) + (dice if row.terms & DICE else 0)
    _close(ref['losses'][:3], [float(total.detach()) if row.terms & (CE | DICE) else 0.0, float(ce.detach()), float(dice.detach())], 'losses', row)
    _close(ref['losses'][3:], ot.pixel_metrics(lm.detach().argmax(1).numpy(), lab.numpy()), 'metrics', row)
    if row.terms & (CE | DICE):
        total.backward()
        _close(ref['dmask'], lm.grad.numpy().reshape(row.shape[0], 3, -1), 'dmask', row)
    else:
        assert not ref['dmask'].any() and ref['losses'][0] == 0
    if row.terms == lx.FULL and row.fam != 'R':
        L = ot.unet_losses(_t(d['lm'], row, 3).double(), lab, wt)
        _close(ref['losses'][:3], [float(L['total']), float(L['ce']), float(L['dice'])], 'unet_losses', row)


_VAL = [r for r in lx.ROWS if r.entry == 'val' and r.P <= 10752]


@pytest.mark.parametrize('row', _VAL, ids=[r.id for r in _VAL])
def test_val_reference_matches_the_transcription(row):
    """train_util_dam.py:499-580 in float64 torch over the same inputs; the per-sample sums are combined the way validate() combines
    them.  With a 'rank' LUT channel k is the k-th value of torch.unique over the batch, as the reference has it."""
    import torch
    import torch.nn.functional as F
    from oracle import train as ot
    d = lx.make_data(row)
    S = lx.reference(row, d)['sums']
    Y, (B, _, _), P, ND = lx.ValLay(row.ND), row.shape, row.P, row.ND
    lm, lp, ld = _t(d['lm'], row, 3).double(), _t(d['lp'], row, 1).double(), _t(d['ld'], row, ND).double()
    lab, dirn, pt, wt = _t(d['lab'], row).long(), _t(d['dl'], row).long(), _t(d['pt'], row).double(), _t(d['wt'], row).double()
    lut = d['lut']
    uniq = torch.unique(dirn)
    if row.spec == 'rank':
        assert [int(lut[int(v)]) for v in uniq] == list(range(len(uniq)))
    ce = F.nll_loss(F.log_softmax(lm, 1), lab, reduction='none').mean()
    prob = F.softmax(lm, 1)
    dice = ot.multiclass_dice(prob, F.one_hot(lab, 3).permute(0, 3, 1, 2).double())
    dce = (F.nll_loss(F.log_softmax(ld, 1), dirn, reduction='none') * (wt / 20)).mean()
    fg0 = ((lab[0] == 1) | (lab[0] == 2)).double()
    oh = torch.zeros((B, ND) + tuple(dirn.shape[1:]), dtype=torch.float64)
    for v in range(ND):
        if lut[v] >= 0:
            oh[:, int(lut[v])] = (dirn == v).double() * fg0
    q = F.softmax(ld, 1).clone()
    q[:, 0] = q[:, 0] * prob[:, 0]
    ddice = ot.multiclass_dice(q, oh)
    mse = F.mse_loss(lp, pt.unsqueeze(1) / 255)
    ratio = lambda i, p, t: sum(1 - (2 * (S[:, i + c] + 1) / (S[:, p + c] + S[:, t + c] + 1)).sum() / B for c in range(t - p))
    got = [S[:, 9].sum() / (B * P), ratio(0, 3, 6), S[:, Y.VS].sum() / (B * P), ratio(Y.IQ, Y.PQ, Y.TQ), S[:, Y.VS + 1].sum() / (B * P)]
    _close(got, [float(ce), float(dice), float(dce), float(ddice), float(mse)], 'ce, dice, dce, ddice, mse', row)
    m = ot.pixel_metrics(lm.argmax(1).numpy(), lab.numpy())
    _close(lx.pixel_metrics64(S[:, Y.VS + 2], S[:, Y.VS + 3], S[:, Y.VS + 4], P), m, 'metrics', row)


@pytest.mark.parametrize('row', lx.ROWS, ids=[r.id for r in lx.ROWS])
def test_guard(row):
    lx.guard(row)


def test_coverage():
    lx.check_coverage()
    assert 55 <= len(lx.ROWS) <= 70


def test_ws_layout_adds_up():
    for r in lx.ROWS:
        lay = lx.ws_layout(r.entry, r.shape[0], r.P, r.ND)
        parts = sorted(v for k, v in lay.items() if k not in ('nchunk', 'total'))
        assert parts[0] == 0 and parts[-1] < lay['total']
    assert lx.ws_layout('dam', 2, 480, 9)['total'] == 2 * 1 * 60 + 2 * 42 + 2 * 60 + 16 + 2
    assert lx.loss_nchunk(135168, 256) == 64 and lx.loss_nchunk(131072, 256) == 64 and lx.loss_nchunk(67584, 128) == 64
    assert lx.n_add(135168, 256) == 9 + 256 + 16 + 0 + 2 and lx.n_add(10752, 256) == 7 + 256 + 1 + 2 + 2 and lx.n_add(10752, 128) == 8 + 128 + 2 + 3 + 2


# the two capped shapes (every thread takes 8 or 9 trips) and (2, 96, 112) (four chains and a tail), every entry
EMULATED = [r for r in lx.ROWS if r.fam == 'R' and r.shape in (lx.CAP9, lx.CAP17, lx.S4)] + \
           [lx.ROW_BY_ID[k] for k in ('dam-R-3x33x31-nd9-q1-t7-bg0', 'dam-R-64x6x8-nd5-q1-t6', 'mask-R-64x6x8-t7')]


@pytest.mark.parametrize('row', EMULATED, ids=[r.id for r in EMULATED])
def test_emulation_inside_bounds(row):
    """the kernels in numpy fp32, in their own order of additions, lie inside every bound: the bounds are not too tight.  Worst err / bound
    seen over these rows: sums 0.031, coef 0.029, dmask 0.41, ddir 0.41, dpoint 0.40, losses 0.996 - a pixel metric, whose bound is the one
    cast from double; the loss values proper stay below 0.2 (the sums' bounds are worst-case chains of ~280 additions, and they assume
    2 ulp for expf, logf and the division where libm and numpy give at most 1 ulp and a correctly rounded quotient)."""
    ref, bd = lx.guard(row)
    report = lx.compare(row, lx.emulate(row), ref, bd)
    print('\n%s: worst err / bound: %s' % (row.id, ', '.join('%s %.3g' % kv for kv in sorted(report.items()))))
    assert all(0 < q <= 1 for k, q in report.items() if not (row.entry == 'mask' and row.terms == 0 and k == 'dmask')), report


# variant -> the row that catches it (and the quantity, for the message)
CATCHERS = {1: 'dam-R-2x24x20m-nd5-q0-t5', 2: 'dam-R-2x24x20m-nd5-q0-t5', 3: 'dam-R-64x6x8-nd5-q1-t6', 4: 'dam-T-3x33x31-nd9-q0-t6',
            5: 'dam-R-2x24x20m-nd5-q0-t5', 6: 'dam-R-2x24x20m-nd5-q0-t5', 7: 'dam-R-1x3x5-nd17-q0-t7', 8: 'dam-L-1x3x5-nd5-q0-t7',
            9: 'dam-T-2x24x20-nd5-q1-t6', 10: 'val-L-2x24x20m-nd5-perm', 11: 'val-R-3x33x31-nd9-perm', 12: 'val-R-3x33x31-nd9-perm'}


def caught(row, variant):
    """(quantity, index, difference / bound) of the element where the wrong variant is furthest beyond the bound, or None"""
    d = lx.make_data(row)
    ref, bd = lx.reference(row, d), lx.bounds(row)
    wrong = lx.reference(row, d, variant)
    best = None
    if 'single' in ref and not np.array_equal(ref['single'], wrong['single']):
        return ('single', (0,), np.inf)
    for k in lx.QUANTITIES:
        if k in ref:
            q, i = lx.worst(np.abs(wrong[k] - ref[k]), bd[k])
            if q > 1 and (best is None or q > best[2]):
                best = (k, i, q)
    return best


@pytest.mark.parametrize('variant', sorted(lx.VARIANTS), ids=['%d' % v for v in sorted(lx.VARIANTS)])
def test_rows_catch_the_wrong_variant(variant):
    rid = CATCHERS[variant]
    hit = caught(lx.ROW_BY_ID[rid], variant)
    assert hit is not None, 'variant %d (%s) stays inside the bounds of %s' % (variant, lx.VARIANTS[variant], rid)
    print('\nvariant %d (%s): caught by %s at %s%s, difference / bound %.3g' % (variant, lx.VARIANTS[variant], rid, hit[0], list(hit[1]), hit[2]))
