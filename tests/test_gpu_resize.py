"""GPU tests of csrc/resize.hip and cdnet_label8_dilate: every case bit-equal to Pillow (tests/golden/resize.npz) and to the numpy mirror,
in both forms."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _resize_cases as rc

IDS = lambda c: rc.mg.case_key(*c)


def _two_axes(case):
    H, W, oh, ow, _ = case
    return H != oh and W != ow


def _run(a, oh, ow, form):
    import torch
    from cdnet_amd import resize
    got = resize.resize_bilinear(torch.from_numpy(a).cuda(), (oh, ow), form=form)
    return got.cpu().numpy(), resize.last_form()


@pytest.mark.parametrize('case', rc.ALL, ids=IDS)
def test_both_forms_equal_golden_and_host_mirror(case):
    from cdnet_amd import _lib, resize
    H, W, oh, ow, C = case
    a = rc.mg.case_input(*case)
    host = resize.resize_bilinear_host(a, (oh, ow))
    identity, huge = (H, W) == (oh, ow), H == 2000
    # form 2 serves every case; an identity is a copy whatever the form
    got, ran = _run(a, oh, ow, 2)
    assert ran == (0 if identity else 2)
    assert np.array_equal(got, host)
    rc.assert_golden(case, got)
    # form 1 where it is accepted: both axes change and the tile's source rows fit the LDS
    if _two_axes(case) or identity:
        got, ran = _run(a, oh, ow, 1)
        assert ran == (0 if identity else 1)
        assert np.array_equal(got, host)
        rc.assert_golden(case, got)
    else:
        with pytest.raises(_lib.CdnetHipError, match='LDS' if huge else 'one axis'):
            _run(a, oh, ow, 1)
    # form 0 picks the LDS form whenever it is accepted
    got, ran = _run(a, oh, ow, 0)
    assert ran == (0 if identity else 1 if _two_axes(case) else 2)
    assert np.array_equal(got, host)


@pytest.mark.parametrize('C', [1, 3])
def test_auto_form_falls_back_to_two_launches_when_a_tile_does_not_fit(C):
    """1500 x 40 -> 9 x 23: both axes change and the 16 output rows of a tile read all 1500 source rows, more than the LDS holds, so
    form 0 takes the two-pass form through the workspace; form 1 is refused"""
    import torch
    from PIL import Image
    from cdnet_amd import _lib, resize
    a = rc.mg.noise_u8(1500 * 40 * C, 4242 + C).reshape((1500, 40) if C == 1 else (1500, 40, C))
    want = np.asarray(Image.fromarray(a).resize((23, 9), Image.BILINEAR))
    assert np.array_equal(resize.resize_bilinear_host(a, (9, 23)), want)
    assert _lib.load().cdnet_resize_workspace_bytes(1, 1500, 40, C, 9, 23, 0) == 1500 * 23 * C
    for form in (0, 2):
        got = resize.resize_bilinear(torch.from_numpy(a).cuda(), (9, 23), form=form)
        assert resize.last_form() == 2
        assert np.array_equal(got.cpu().numpy(), want), form
    with pytest.raises(_lib.CdnetHipError, match='LDS'):
        resize.resize_bilinear(torch.from_numpy(a).cuda(), (9, 23), form=1)
    assert resize.last_form() == 2                               # (a refused call leaves the last successful form)


@pytest.mark.parametrize('case', [c for c in rc.ALL if c[4] == 3], ids=IDS)
def test_rgb_from_a_view_one_byte_into_its_storage(case):
    import torch
    from cdnet_amd import resize
    H, W, oh, ow, C = case
    a = rc.mg.case_input(*case)
    n = a.size
    forms = (1, 2) if _two_axes(case) else (2,)
    for form in forms:
        src = torch.zeros(n + 1, dtype=torch.uint8, device='cuda')
        src[1:] = torch.from_numpy(a.reshape(-1)).cuda()
        view = src[1:].view(H, W, 3)
        assert view.data_ptr() % 2 == 1 and view.is_contiguous()
        got = resize.resize_bilinear(view, (oh, ow), form=form).cpu().numpy()
        rc.assert_golden(case, got)


def test_batch_of_two():
    import torch
    from cdnet_amd import resize
    case = (37, 53, 96, 137, 3)
    a = rc.mg.case_input(*case)
    b = np.ascontiguousarray(a[::-1, ::-1])
    batch = torch.from_numpy(np.stack([a, b])).cuda()
    for form in (1, 2):
        got = resize.resize_bilinear(batch, (96, 137), form=form).cpu().numpy()
        assert got.shape == (2, 96, 137, 3) and resize.last_form() == form
        rc.assert_golden(case, got[0])
        assert np.array_equal(got[1], resize.resize_bilinear_host(b, (96, 137)))


@pytest.mark.parametrize('case', rc.MASK_CASES, ids=lambda c: '{}x{}_{}x{}'.format(*c))
def test_mask_mode(case):
    import torch
    from PIL import Image
    from cdnet_amd import resize
    H, W, oh, ow = case
    m = rc.mg.mask_input(H, W)
    want = rc.golden_mask(case)
    live = (np.asarray(Image.fromarray(m * np.uint8(255)).resize((ow, oh), Image.BILINEAR)) > 127.5).astype(np.uint8)
    assert np.array_equal(want, live)
    for form in (0, 1, 2):
        got = resize.resize_mask(torch.from_numpy(m).cuda(), (oh, ow), form=form)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (oh, ow)
        assert resize.last_form() == (2 if form == 2 else 1)
        assert np.array_equal(got.cpu().numpy(), want), form
    # one axis at a time: the pass that runs both reads v * 255 and writes the threshold
    for size in ((H, ow), (oh, W), (H, W)):
        got = resize.resize_mask(torch.from_numpy(m).cuda(), size).cpu().numpy()
        live = (np.asarray(Image.fromarray(m * np.uint8(255)).resize((size[1], size[0]), Image.BILINEAR)) > 127.5).astype(np.uint8)
        assert np.array_equal(got, live), size
    # a batch [N, H, W]
    mm = np.stack([m, 1 - m])
    got = resize.resize_mask(torch.from_numpy(mm).cuda(), (oh, ow)).cpu().numpy()
    assert np.array_equal(got[0], want)
    assert np.array_equal(got[1], resize.resize_mask(torch.from_numpy(1 - m), (oh, ow)).numpy())


def _disk(r):
    y, x = np.mgrid[-r:r + 1, -r:r + 1]
    return (y * y + x * x) <= r * r


@pytest.mark.parametrize('radius', [0, 1, 2])
def test_label8_dilate_vs_scipy(radius):
    import torch
    from scipy import ndimage as ndi
    from cdnet_amd import postproc
    H, W = 45, 61
    m = np.zeros((H, W), np.uint8)
    m[5:12, 6:14] = 1
    m[8, 9] = 0                                   # a one-pixel hole: it must stay
    m[20:24, 20:24] = 1
    m[24:28, 24:28] = 1                           # touches the block above only diagonally: one component when 8-connected
    m[0:6, 50:61] = 1                             # on the border
    m[40:45, 0:3] = 1                             # on two borders
    m[30, 40] = 1                                 # a single pixel: no small-object removal here
    lab, n = ndi.label(m, structure=np.ones((3, 3), int))
    assert n == 5
    want = ndi.grey_dilation(lab, footprint=_disk(radius)) if radius else lab
    r = postproc.label8_dilate(torch.from_numpy(m).cuda(), radius, want_label=True)
    assert np.array_equal(r['label'].cpu().numpy(), lab)
    assert np.array_equal(r['final'].cpu().numpy(), want)
    assert int(r['counts'][0]) == n
    assert r['label'][8, 9].item() == 0
    if radius == 0:
        assert r['final'][8, 9].item() == 0
    # a batch, and a width the one-launch tile labelling serves (W a multiple of 64)
    big = np.zeros((2, 48, 64), np.uint8)
    big[0, :H, :W] = m
    big[1, 3:9, 3:9] = 1
    rb = postproc.label8_dilate(torch.from_numpy(big).cuda(), radius)
    for i in range(2):
        li, _ = ndi.label(big[i], structure=np.ones((3, 3), int))
        wi = ndi.grey_dilation(li, footprint=_disk(radius)) if radius else li
        assert np.array_equal(rb['final'][i].cpu().numpy(), wi), i
    assert rb['counts'].cpu().tolist() == [5, 1]


def test_restore_chain_small_stage_is_the_chains():
    """cdnet_fill_remove_small leaves the `small` stage of cdnet_cc_chain, bit for bit; restore_chain = that, resize_mask, label8_dilate"""
    import torch
    from cdnet_amd import postproc, resize
    m = np.stack([rc.mg.mask_input(61, 83, 7), rc.mg.mask_input(61, 83, 8)])
    m[0, 20:30, 20:30] = 1
    m[0, 24, 25] = 0                                  # a hole to fill
    m[1, 3, 70] = 1                                   # (whatever is smaller than min_area goes)
    pred = torch.from_numpy(m).cuda()
    chain = postproc.cc_chain(pred, 1, 20, 2, want_stages=True)
    r = postproc.restore_chain(pred, (120, 170), 1, 20, 2)
    assert np.array_equal(r['small'].cpu().numpy(), chain['small'].cpu().numpy())
    assert r['small'][0, 24, 25].item() == 1
    back = resize.resize_mask(chain['small'], (120, 170))
    assert np.array_equal(r['restored'].cpu().numpy(), back.cpu().numpy())
    tail = postproc.label8_dilate(back, 2)
    assert np.array_equal(r['final'].cpu().numpy(), tail['final'].cpu().numpy()) and tuple(r['final'].shape) == (2, 120, 170)
    assert r['counts'].cpu().tolist() == tail['counts'].cpu().tolist()
