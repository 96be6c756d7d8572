"""cdnet_dam_loss_terms: every term set equals cdnet_dam_loss_classes bit for bit; WMAP clear (unweighted CE maps, plain multi-class
dice on the direction branch), CE clear (mask CE out of total and gradient) and both against a torch restatement; DICE clear is an
argument error."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WMAP, CE, DICE = 1, 2, 4
# the last: P = 10 752, 6 chunks at 256 threads and 11 at the 17 classes' 128 - the chunk sum's four chains and its tail both run
SHAPES = [(2, 24, 20), (3, 40, 36), (1, 96, 112)]


def _rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-12))


@functools.lru_cache(maxsize=None)
def _case(shape, ND):
    """logits (mask, point, direction) and targets (label, direction, point, weight [B,1,H,W]) as CPU tensors, the last sample's direction
    map constant (train_util_dam.py:141); built once and never modified"""
    import torch
    from cdnet_amd import synth
    B, H, W = shape
    lab, dirn, point, weight = synth.train_targets(B, H, W, 11)
    dirn = synth.remap_direction(dirn, ND).copy()
    dirn[B - 1] = 0
    rs = np.random.RandomState(5 + ND)
    lm = torch.from_numpy((rs.randn(B, 3, H, W) * 2).astype(np.float32))
    ld = torch.from_numpy((rs.randn(B, ND, H, W) * 2).astype(np.float32))
    lp = torch.from_numpy(rs.randn(B, 1, H, W).astype(np.float32))
    return lm, lp, ld, torch.from_numpy(lab), torch.from_numpy(dirn), torch.from_numpy(point), torch.from_numpy(weight)


def _run(case, ND, quirk, terms=None, weight_null=False, raw=False):
    import torch
    from cdnet_amd import _lib
    lm, lp, ld, lab, dirn, point, weight = case
    B, _, H, W = lm.shape
    lib = _lib.load()
    ws = torch.empty((lib.cdnet_dam_loss_classes_workspace_floats(B, H * W, ND),), dtype=torch.float32, device='cuda')
    losses = torch.zeros(11, device='cuda')
    dm, dp, dd = torch.empty(lm.shape, device='cuda'), torch.empty(lp.shape, device='cuda'), torch.empty(ld.shape, device='cuda')
    keep = [lm.cuda(), lp.cuda(), ld.cuda(), lab.cuda(), dirn.cuda(), point.cuda(), None if weight_null else weight[:, 0].contiguous().cuda()]
    args = [_lib.ptr(t) for t in keep] + [B, H, W, ND, quirk, _lib.ptr(ws), ws.numel(), _lib.ptr(losses), _lib.ptr(dm), _lib.ptr(dp), _lib.ptr(dd),
                                          _lib.stream_ptr()]
    if raw:
        return lib.cdnet_dam_loss_terms(*args, terms)
    if terms is None:
        _lib.call('cdnet_dam_loss_classes', *args)
    else:
        _lib.call('cdnet_dam_loss_terms', *args, terms)
    return losses.cpu(), dm.cpu(), dp.cpu(), dd.cpu()


def _restate(case, ND, quirk, terms):
    """the loss of train_util_dam.py:167-276 for the term word, composed from the oracle's pieces; returns the six values in the order of
    `losses` and the three logit gradients"""
    import torch
    import torch.nn.functional as F
    from oracle import train as ot
    lm, lp, ld, lab, dirn, point, weight = case
    lm, lp, ld = [t.clone().requires_grad_(True) for t in (lm, lp, ld)]
    w = weight.float().div(20).squeeze(1) if terms & WMAP else torch.ones(lab.shape)
    label, direction = lab.long(), dirn.long()
    ce = (F.nll_loss(F.log_softmax(lm, 1), label, reduction='none') * w).mean()
    dice = ot.multiclass_dice(F.softmax(lm, 1), F.one_hot(label, 3).permute(0, 3, 1, 2).float())
    dce = (F.nll_loss(F.log_softmax(ld, 1), direction, reduction='none') * w).mean()
    oh = ot.direction_onehot(direction, label, ND, bool(quirk))
    if terms & WMAP:
        ddice = ot.weight_multiclass_dice(F.softmax(ld, 1), oh, w)
    else:
        ddice = ot.multiclass_dice(F.softmax(ld, 1), oh)                 # :241-244: criterion_dice, a sum over the classes
    mse = F.mse_loss(lp, point.float().unsqueeze(1))
    total = dice + dce + ddice + mse
    if terms & CE:
        total = ce + total
    total.backward()
    return [float(v) for v in (total, dce, ddice, mse, ce, dice)], lm.grad, lp.grad, ld.grad


@pytest.mark.parametrize('quirk', [0, 1])
@pytest.mark.parametrize('ND', [5, 9, 17])
@pytest.mark.parametrize('shape', SHAPES)
def test_terms(shape, ND, quirk):
    import torch
    case = _case(shape, ND)
    base = _run(case, ND, quirk)
    full = _run(case, ND, quirk, WMAP | CE | DICE)
    for a, b in zip(full, base):
        assert torch.equal(a, b)
    for terms in (CE | DICE, WMAP | DICE, DICE):
        want, gm, gp, gd = _restate(case, ND, quirk, terms)
        losses, dm, dp, dd = _run(case, ND, quirk, terms, weight_null=not terms & WMAP)
        print(shape, ND, quirk, terms, losses.tolist(), want)
        np.testing.assert_allclose(losses[:6].numpy(), want, rtol=2e-5, atol=2e-6)
        assert torch.equal(losses[6:], base[0][6:])                       # the metrics do not depend on the terms
        assert _rel(dm, gm) < 1e-4 and _rel(dp, gp) < 1e-4 and _rel(dd, gd) < 1e-4, (terms, _rel(dm, gm), _rel(dp, gp), _rel(dd, gd))
    for terms in (0, WMAP | CE, CE, WMAP):
        assert _run(case, ND, quirk, terms, raw=True) == 1                # CDNET_E_ARG: no DAM configuration without the dice terms
    assert _run(case, ND, quirk, WMAP | CE | DICE, weight_null=True, raw=True) == 1
