"""cdnet_mask_loss (mask_loss.hip): bit identity with the mask terms of cdnet_dam_loss_classes when every term is on, the other term
words against a torch restatement, the pixel metrics, and the argument / label errors."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WMAP, CE, DICE = 1, 2, 4
# (B, H, W): P < 256 (idle threads, one chunk) | plain | odd P | several chunks | P = 135 168 > the 64-chunk cap of 131 072: threads loop
# | P = 10 752: 6 chunks, the finalize kernel's chunk sum runs one round of its four chains and a tail of two
SHAPES = [(1, 7, 5), (2, 24, 20), (2, 33, 31), (3, 64, 64), (1, 384, 352), (1, 96, 112)]


def _rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-12))


@functools.lru_cache(maxsize=None)
def _case(shape):
    """(logits f32 [B,3,H,W], label u8 [B,H,W], weight u8 [B,H,W]) as CPU tensors; built once per shape and never modified"""
    import torch
    from cdnet_amd import synth
    B, H, W = shape
    rs = np.random.RandomState(100 + H)
    if H < 16 or W < 16:
        lab = rs.randint(0, 3, size=(B, H, W)).astype(np.uint8)                # seeded noise: train_targets needs room for a nucleus
        weight = rs.randint(1, 200, size=(B, H, W)).astype(np.uint8)
    else:
        lab, _, _, weight = synth.train_targets(B, H, W, 11)
        weight = np.ascontiguousarray(weight[:, 0])
        if B > 1:
            lab = lab.copy()
            lab[B - 1] = 0                         # a sample without foreground: tp = 0, the epsilon denominators decide
    lm = torch.from_numpy((rs.randn(B, 3, H, W) * 2).astype(np.float32))
    return lm, torch.from_numpy(lab), torch.from_numpy(weight)


def _mask_loss(lm, lab, weight, terms, grad=True):
    import torch
    from cdnet_amd import _lib
    B, _, H, W = lm.shape
    ws = torch.empty((_lib.load().cdnet_mask_loss_workspace_floats(B, H * W),), dtype=torch.float32, device='cuda')
    losses = torch.full((8,), 7.0, device='cuda')
    dm = torch.full(lm.shape, float('nan'), device='cuda') if grad else None
    keep = [lm.cuda(), lab.cuda(), None if weight is None else weight.cuda()]
    _lib.call('cdnet_mask_loss', *[_lib.ptr(t) for t in keep], B, H, W, terms, _lib.ptr(ws), ws.numel(), _lib.ptr(losses), _lib.ptr(dm),
              _lib.stream_ptr())
    return losses.cpu(), None if dm is None else dm.cpu()


def _dam_loss(lm, lab, weight):
    """the parent's route: the 9-class DAM loss over all-zero point / direction branches"""
    import torch
    from cdnet_amd import _lib
    B, _, H, W = lm.shape
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device='cuda')
    point, dirn, dirlab, pt = z((B, 1, H, W), torch.float32), z((B, 9, H, W), torch.float32), z((B, H, W), torch.uint8), z((B, H, W), torch.float16)
    ws = torch.empty((_lib.load().cdnet_dam_loss_classes_workspace_floats(B, H * W, 9),), dtype=torch.float32, device='cuda')
    losses = torch.zeros(11, device='cuda')
    dm, dp, dd = torch.empty(lm.shape, device='cuda'), torch.empty_like(point), torch.empty_like(dirn)
    keep = [lm.cuda(), point, dirn, lab.cuda(), dirlab, pt, weight.cuda()]
    _lib.call('cdnet_dam_loss_classes', *[_lib.ptr(t) for t in keep], B, H, W, 9, 1, _lib.ptr(ws), ws.numel(), _lib.ptr(losses), _lib.ptr(dm),
              _lib.ptr(dp), _lib.ptr(dd), _lib.stream_ptr())
    return losses.cpu(), dm.cpu()


@pytest.mark.parametrize('shape', SHAPES)
def test_all_terms_equal_the_dam_mask_terms_bit_for_bit(shape):
    import torch
    lm, lab, weight = _case(shape)
    want, want_dm = _dam_loss(lm, lab, weight)
    got, dm = _mask_loss(lm, lab, weight, WMAP | CE | DICE)
    assert torch.equal(got[1], want[4]), (float(got[1]), float(want[4]))          # ce
    assert torch.equal(got[2], want[5]), (float(got[2]), float(want[5]))          # dice
    assert torch.equal(dm, want_dm)
    assert torch.equal(got[0], got[1] + got[2])                                   # one fp32 add
    # the value-only call reports the same eight values
    assert torch.equal(_mask_loss(lm, lab, weight, WMAP | CE | DICE, grad=False)[0], got)


def _restate(lm, lab, weight, terms):
    """(total, ce, dice) of the term word in torch, composed from the oracle's dice and F.nll_loss (train_util.py:128-136, 183-190)"""
    import torch
    import torch.nn.functional as F
    from oracle import train as ot
    label = lab.long()
    ce_map = F.nll_loss(F.log_softmax(lm, 1), label, reduction='none')
    if terms & WMAP:
        ce_map = ce_map * weight.float().div(20)
    ce = ce_map.mean()
    dice = ot.multiclass_dice(F.softmax(lm, 1), F.one_hot(label, 3).permute(0, 3, 1, 2).float())
    total = (ce if terms & CE else 0) + (dice if terms & DICE else 0)
    return total, ce, dice


@pytest.mark.parametrize('terms', [0, WMAP, CE, WMAP | CE, DICE, WMAP | DICE, CE | DICE])
@pytest.mark.parametrize('shape', SHAPES)
def test_other_term_words_against_torch(shape, terms):
    import torch
    from oracle import train as ot
    lm, lab, weight = _case(shape)
    x = lm.clone().requires_grad_(True)
    total, ce, dice = _restate(x, lab, weight, terms)
    got, dm = _mask_loss(lm, lab, weight if terms & WMAP else None, terms)
    print(shape, terms, got.tolist(), float(total), float(ce), float(dice))
    np.testing.assert_allclose(got[:3].numpy(), [float(total), float(ce), float(dice)], rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(got[3:].numpy(), ot.pixel_metrics(lm.argmax(1).numpy(), lab.numpy()), rtol=1e-6)
    if terms & (CE | DICE):
        total.backward()
        assert _rel(dm, x.grad) < 1e-4, _rel(dm, x.grad)
    else:
        assert float(got[0]) == 0.0 and torch.equal(dm, torch.zeros_like(dm))


def test_label_out_of_range_poisons_every_value():
    lm, lab, weight = _case((2, 24, 20))
    bad = lab.clone()
    bad[1, 3, 4] = 3
    got, dm = _mask_loss(lm, bad, weight, WMAP | CE | DICE)
    assert np.isnan(got.numpy()).all()
    assert np.isfinite(dm.numpy()).all()                   # (indices are clamped: the gradient buffer is written in bounds)


def test_argument_errors_are_found_without_a_launch():
    """every pointer below is a host address or NULL: a launch or a memset on any of them would fault, an argument check does not"""
    from cdnet_amd import _lib
    lib = _lib.load()
    B, H, W = 2, 24, 20
    need = lib.cdnet_mask_loss_workspace_floats(B, H * W)
    assert need > 0
    host = (C.c_float * 16)()
    p = C.cast(host, C.c_void_p)

    def call(B=B, weight=p, terms=WMAP | CE | DICE, ws_floats=need):
        return lib.cdnet_mask_loss(p, p, weight, B, H, W, terms, p, ws_floats, p, None, None)

    assert call(weight=None) == 1 and b'weight' in lib.cdnet_last_error()             # CDNET_E_ARG
    assert call(ws_floats=need - 1) == 1 and b'workspace' in lib.cdnet_last_error()
    assert call(B=65) == 1 and b'65' in lib.cdnet_last_error()
    assert call(terms=8) == 1
