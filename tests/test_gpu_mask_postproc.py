"""GPU parity of the mask-only post-processing kernels (test.py:216-296): the one-launch view mean + class of whole images
(cdnet_mask_views_argmax), the two-launch tile chain (cdnet_tile_mask_postproc) and the label dilation alone (cdnet_dilate_labels)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def to_view(a, xf):
    """image frame [..., H, W] -> the stored frame of view `xf` (PIL rotate(90, expand) first, then the flips: test.py:228-254)"""
    if xf & 4:
        a = np.rot90(a, k=1, axes=(-2, -1))
    if xf & 1:
        a = np.flip(a, -1)
    if xf & 2:
        a = np.flip(a, -2)
    return np.ascontiguousarray(a)


def unflip(a, xf):
    """test.py:240-265: np.flip / np.rot90(k=3) back to the image frame"""
    if xf & 2:
        a = np.flip(a, -2)
    if xf & 1:
        a = np.flip(a, -1)
    if xf & 4:
        a = np.rot90(a, k=3, axes=(-2, -1))
    return np.ascontiguousarray(a)


def view_logits(K, H, W, seed):
    """eight views' logits [8, K, h_v*w_v] in their own frames: noise, exact ties of channels 0 and 1 on a band of image rows in every view,
    one NaN logit"""
    rs = np.random.RandomState(seed)
    out = []
    for xf in range(8):
        a = (2.0 * rs.randn(K, H, W)).astype(np.float32)
        if K >= 2:
            a[1, H // 3:H // 3 + 3] = a[0, H // 3:H // 3 + 3]
        if xf == 5:
            a[K - 1, H // 2, W // 2] = np.nan
        out.append(to_view(a, xf).reshape(K, -1))
    return np.stack(out)


def numpy_mean_class(views, K, H, W):
    """the reference's arithmetic on the kernel's own per-view probabilities (one call per view, V = 1, view code 0): un-flip, float32 sum in
    view order, / 8, np.argmax or `>= 0.5`"""
    import torch
    from cdnet_amd import postproc
    s = None
    for xf in range(8):
        hv, wv = (W, H) if xf & 4 else (H, W)
        t = torch.from_numpy(views[xf]).cuda().reshape(1, 1, K, hv * wv)
        p = postproc.mask_views_argmax(t, [0], hv, wv, want_prob=True)['prob_mean'][0].cpu().numpy()
        p = unflip(p, xf)
        s = p if s is None else s + p
    mean = s / 8
    pred = (mean[0] >= 0.5).astype(np.uint8) if K == 1 else np.argmax(mean, axis=0).astype(np.uint8)
    return mean, pred


def test_single_view_probabilities_are_probmaps():
    import torch
    from cdnet_amd import postproc
    H, W = 64, 80
    g = torch.Generator(device='cuda').manual_seed(3)
    ml = 3.0 * torch.randn((2, 3, H, W), device='cuda', generator=g)
    dl = torch.randn((2, 9, H, W), device='cuda', generator=g)
    prob, _ = postproc.probmaps(ml, dl)
    r = postproc.mask_views_argmax(ml, [0], H, W, want_prob=True)
    got = r['prob_mean'].cpu().numpy()
    assert np.array_equal(got.view(np.uint32), prob.cpu().numpy().view(np.uint32))
    np.testing.assert_allclose(got, torch.softmax(ml.cpu(), dim=1).numpy(), rtol=0, atol=3e-7)
    assert np.array_equal(r['pred'].cpu().numpy(), np.argmax(got, axis=1).astype(np.uint8))


@pytest.mark.parametrize('K', [1, 2, 3])
@pytest.mark.parametrize('shape', [(37, 53), (120, 152), (1000, 1000)])
def test_eight_views_mean_and_class_vs_numpy(K, shape):
    import torch
    from cdnet_amd import postproc
    H, W = shape
    views = view_logits(K, H, W, seed=K * 100 + H)
    r = postproc.mask_views_argmax(torch.from_numpy(views).cuda()[None], list(postproc.TTA_XFORMS), H, W, want_prob=True)
    mean, pred = numpy_mean_class(views, K, H, W)
    got_p, got_m = r['pred'][0].cpu().numpy(), r['prob_mean'][0].cpu().numpy()
    assert np.array_equal(got_m, mean, equal_nan=True)
    assert np.array_equal(got_p, pred)
    assert np.isnan(mean).any()                                  # (the NaN pixel reached the mean: its class is numpy's)
    if K >= 2:
        band = mean[0, H // 3:H // 3 + 3] == mean[1, H // 3:H // 3 + 3]
        assert band.all() and not (got_p[H // 3:H // 3 + 3] == 1).any()     # exact ties: the first maximum
    # the class plane alone (prob_mean not written) is the same
    r2 = postproc.mask_views_argmax(torch.from_numpy(views).cuda()[None], list(postproc.TTA_XFORMS), H, W)
    assert 'prob_mean' not in r2 and np.array_equal(r2['pred'][0].cpu().numpy(), pred)


def nuclei_logits(B, H, W, seed, K=3):
    """mask logits of rendered nuclei (ellipses: class 1 inside, class 2 on a ring, noise everywhere) as UNet would return them"""
    from cdnet_amd import synth
    rs = np.random.RandomState(seed)
    out = np.empty((B, K, H, W), np.float32)
    for b in range(B):
        inst = synth.ellipse_instances(H, W, max(2, H * W // 1100), rs, 5, 12, 4) if min(H, W) >= 32 else np.zeros((H, W), np.int32)
        inside = (inst > 0).astype(np.float32)
        out[b] = 1.5 * rs.randn(K, H, W)
        out[b, min(1, K - 1)] += 4.0 * inside - 2.0
        if K == 3:
            out[b, 2] += 1.0 * (synth.erode8(inst > 0) != (inst > 0))
    return out


CASES = [(64, 256, 256, 2, 3), (64, 256, 256, 0, 2), (2, 64, 64, 0, 3), (2, 64, 64, 1, 3), (2, 64, 64, 2, 1), (2, 64, 64, 5, 3),
         (3, 3, 64, 0, 3), (3, 3, 64, 1, 2), (3, 3, 64, 2, 3), (3, 3, 64, 5, 3), (2, 128, 512, 0, 3), (2, 128, 512, 1, 3),
         (2, 128, 512, 2, 2), (2, 128, 512, 5, 3)]


@pytest.mark.parametrize('B,H,W,radius,K', CASES)
def test_tile_chain_vs_per_step_and_oracle(B, H, W, radius, K):
    import torch
    from cdnet_amd import postproc
    from oracle import postproc as orc
    logits = torch.from_numpy(nuclei_logits(B, H, W, seed=H + W + radius, K=K)).cuda()
    assert postproc.tile_mask_postproc_eligible(B, K, H, W)
    f = postproc.tile_mask_postproc(logits, 20, radius, want_stages=True)
    m = postproc.mask_views_argmax(logits, [0], H, W, want_prob=True)
    s = postproc.cc_chain(m['pred'], 1, 20, radius, want_stages=True)
    torch.cuda.synchronize()
    assert np.array_equal(f['prob'].cpu().numpy().view(np.uint32), m['prob_mean'].cpu().numpy().view(np.uint32))
    assert np.array_equal(f['pred'].cpu().numpy(), m['pred'].cpu().numpy())
    for k in ('fill', 'small', 'label', 'final', 'counts'):
        assert np.array_equal(f[k].cpu().numpy(), s[k].cpu().numpy()), k
    pred = f['pred'].cpu().numpy()
    for b in range(min(B, 4)):
        w = orc.cc_chain(pred[b] == 1, 20, radius)
        assert np.array_equal(f['final'][b].cpu().numpy(), w['final']), b
        assert int(f['counts'][b]) == w['count']
    assert int(f['counts'].sum()) > 0 or H * W < 1024


def test_tile_chain_all_tiles_vs_oracle():
    """every tile of the 64 x 256^2 batch against the oracle's CC chain"""
    import torch
    from cdnet_amd import postproc
    from oracle import postproc as orc
    logits = torch.from_numpy(nuclei_logits(64, 256, 256, seed=11)).cuda()
    f = postproc.tile_mask_postproc(logits, 20, 2)
    pred, final, counts = f['pred'].cpu().numpy(), f['final'].cpu().numpy(), f['counts'].cpu().numpy()
    for b in range(64):
        w = orc.cc_chain(pred[b] == 1, 20, 2)
        assert np.array_equal(final[b], w['final']) and counts[b] == w['count'], b
    assert counts.min() > 5


@pytest.mark.parametrize('radius', list(range(9)))
def test_dilate_labels_vs_oracle(radius):
    import torch
    from cdnet_amd import postproc
    from oracle import postproc as orc
    rs = np.random.RandomState(radius)
    lab = np.zeros((2, 45, 70), np.int32)
    for n in range(2):
        for k in range(1, 25):
            y, x = rs.randint(0, 45), rs.randint(0, 70)
            lab[n, y:y + rs.randint(1, 6), x:x + rs.randint(1, 6)] = k
    t = torch.from_numpy(lab).cuda()
    got = postproc.dilate_labels(t, radius).cpu().numpy()
    assert np.array_equal(t.cpu().numpy(), lab)                 # (the input is left as it was)
    for n in range(2):
        assert np.array_equal(got[n], orc.dilate_disk(lab[n], radius)), n
    assert np.array_equal(postproc.dilate_labels(t[0], radius).cpu().numpy(), got[0])
