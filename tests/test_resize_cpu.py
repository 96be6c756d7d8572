"""CPU tests of the 'scale' test transform: the numpy mirror of the resize kernels against the golden file and live Pillow, Scale's size
rule, the --scale option, and the argument checks of the new C entries (they return before any HIP call)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _resize_cases as rc


def _pillow(a, oh, ow):
    from PIL import Image
    return np.asarray(Image.fromarray(a).resize((ow, oh), Image.BILINEAR))


@pytest.mark.parametrize('case', rc.ALL, ids=lambda c: rc.mg.case_key(*c))
def test_host_mirror_equals_golden_and_live_pillow(case):
    from cdnet_amd import resize
    H, W, oh, ow, C = case
    a = rc.mg.case_input(*case)
    got = resize.resize_bilinear_host(a, (oh, ow))
    rc.assert_golden(case, got)
    assert np.array_equal(got, _pillow(a, oh, ow))


@pytest.mark.parametrize('case', rc.MASK_CASES, ids=lambda c: '{}x{}_{}x{}'.format(*c))
def test_host_mask_equals_golden_and_live_pillow(case):
    import torch
    from cdnet_amd import resize
    H, W, oh, ow = case
    m = rc.mg.mask_input(H, W)
    got = resize.resize_mask(torch.from_numpy(m), (oh, ow)).numpy()
    assert got.dtype == np.uint8 and np.array_equal(got, rc.golden_mask(case))
    assert np.array_equal(got, (_pillow(m * np.uint8(255), oh, ow) > 127.5).astype(np.uint8))


@pytest.mark.parametrize('mode', ['L', 'RGB', 'mask'])
def test_host_mirror_equals_pillow_on_random_sizes(mode):
    from cdnet_amd import resize
    rng = np.random.default_rng({'L': 1, 'RGB': 2, 'mask': 3}[mode])
    for _ in range(100):
        H, W = (int(v) for v in rng.integers(1, 91, 2))
        oh, ow = (int(v) for v in rng.integers(1, 141, 2))
        if mode == 'RGB':
            a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        elif mode == 'L':
            a = rng.integers(0, 256, (H, W), dtype=np.uint8)
        else:
            a = rng.integers(0, 2, (H, W), dtype=np.uint8) * np.uint8(255)
        assert np.array_equal(resize.resize_bilinear_host(a, (oh, ow)), _pillow(a, oh, ow)), (mode, H, W, oh, ow)


def test_tables_follow_the_stated_rule():
    from cdnet_amd import resize
    for (i, o) in ((200, 23), (53, 137), (2000, 8), (1, 7), (7, 1), (64, 64)):
        bounds, kk = resize.resize_tables(i, o)
        fs = max(i / o, 1.0)
        ksize = 2 * int(np.ceil(fs)) + 1
        assert bounds.dtype == np.int32 and kk.dtype == np.int32 and bounds.shape == (o, 2) and kk.shape == (o, ksize)
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds.sum(1) <= i).all() and (bounds[:, 1] <= ksize).all()
        assert (kk >= 0).all()                                            # (the bilinear filter has no negative lobe)
        assert (np.abs(kk.sum(1) - (1 << 22)) <= ksize).all()             # (each weight is rounded once)
        for r in range(o):
            assert (kk[r, bounds[r, 1]:] == 0).all()
        assert resize.resize_tables(i, o)[1] is kk                        # cached


def test_scaled_size_and_scale_class():
    from PIL import Image
    from cdnet_amd import resize
    from cdnet_amd.my_transforms_direction import Scale
    assert resize.scaled_size(53, 70, 96) == (96, 126)
    assert resize.scaled_size(70, 53, 96) == (126, 96)
    assert resize.scaled_size(64, 64, 96) == (96, 96)
    assert resize.scaled_size(96, 120, 96) is None and resize.scaled_size(120, 96, 96) is None
    assert resize.scaled_size(53, 70, (40, 30)) == (40, 30)
    rng = np.random.default_rng(0)
    tall = Image.fromarray(rng.integers(0, 256, (70, 53, 3), dtype=np.uint8))
    wide = Image.fromarray(rng.integers(0, 256, (53, 70, 3), dtype=np.uint8))
    square = Image.fromarray(rng.integers(0, 256, (64, 64, 3), dtype=np.uint8))
    a, b, c = Scale(96)((tall, wide, square))
    assert a.size == (96, 126) and b.size == (126, 96) and c.size == (96, 96)
    assert np.array_equal(np.asarray(a), np.asarray(tall.resize((96, 126), Image.BILINEAR)))
    assert np.array_equal(np.asarray(a), resize.resize_bilinear_host(np.asarray(tall), (126, 96)))
    same, = Scale(53)((tall,))
    assert same is tall
    same, = Scale(53)((wide,))
    assert same is wide
    pair, = Scale((40, 30))((tall,))
    assert pair.size == (40, 30)
    assert isinstance(Scale(96)((tall,)), tuple)


def test_scale_option():
    from cdnet_amd.options import Options
    assert 'scale' not in Options(isTrain=False).parse([]).transform['test']
    assert 'scale' not in Options(isTrain=False).parse(['--scale', '0']).transform['test']
    t = Options(isTrain=False).parse(['--scale', '96']).transform['test']
    assert list(t)[0] == 'scale' and t['scale'] == 96 and 'to_tensor' in t
    opt = Options(isTrain=False)
    opt.transform['test'] = {'scale': 64, 'to_tensor': 1}
    t = opt.parse([]).transform['test']
    assert list(t)[0] == 'scale' and t['scale'] == 64
    opt.transform['test']['scale'] = 80                                   # set after parsing, as the reference's users do
    assert opt.transform['test']['scale'] == 80


def test_mask_entry_rejects_scale_with_postproc_1():
    from cdnet_amd import test
    with pytest.raises(ValueError, match='postproc 1'):
        test.main(['--model-name', 'UNet', '--direction', '0', '--scale', '96', '--postproc', '1', '--img-dir', '/nonexistent'])


FAKE = 4096


def test_resize_entry_rejects_bad_arguments_without_a_gpu():
    from cdnet_amd import _lib
    lib = _lib.load()
    err = lambda: lib.cdnet_last_error().decode()

    def call(src=FAKE, N=1, H=40, W=64, C=3, oh=80, ow=100, hb=FAKE, hk=FAKE, hks=3, vb=FAKE, vk=FAKE, vks=3, mask=0, form=0, ws=FAKE,
             nws=1 << 20, out=FAKE + (1 << 20)):
        return lib.cdnet_resize_bilinear(src, N, H, W, C, oh, ow, hb, hk, hks, vb, vk, vks, mask, form, ws, nws, out, None)
    for kw in (dict(src=None), dict(out=None), dict(hb=None), dict(hk=None), dict(vb=None), dict(vk=None), dict(ws=None, form=2)):
        assert call(**kw) == 1 and 'null pointer' in err(), kw
    for kw in (dict(N=0), dict(H=0), dict(W=0), dict(oh=0), dict(ow=-1), dict(N=65536)):
        assert call(**kw) == 1 and 'bad size' in err(), kw
    for C in (0, 2, 4):
        assert call(C=C) == 1 and 'C=%d' % C in err()
    assert call(mask=1) == 1 and 'mask_mode' in err()                     # (mask mode is mode L)
    assert call(mask=2, C=1) == 1 and 'mask_mode' in err()
    assert call(form=3) == 1 and 'form=3' in err()
    assert call(hks=5) == 1 and 'hksize=5' in err() and 'ksize 3' in err()
    assert call(vks=1) == 1 and 'vksize=1' in err()
    assert call(H=200, W=150, oh=23, ow=17, hks=19, vks=21) == 1 and 'vksize=21' in err()         # (200 / 23 = 8.7: 2 * 9 + 1 = 19; 150 / 17: 19)
    assert call(H=200, W=150, oh=23, ow=17, hks=21, vks=19) == 1 and 'hksize=21' in err()
    assert call(out=FAKE + 100) == 1 and 'overlaps' in err()
    assert call(form=2, nws=40 * 100 * 3 - 1) == 2 and 'workspace' in err()
    # form 1: a tile whose source rows do not fit the LDS, and a one-axis resize
    assert call(H=2000, W=16, C=1, oh=8, ow=16, vks=501, form=1) == 1 and 'LDS' in err()
    assert call(H=2000, W=16, C=3, oh=8, ow=16, vks=501, form=1) == 1 and 'LDS' in err()
    assert call(oh=40, form=1) == 1 and 'one axis' in err()
    assert lib.cdnet_resize_workspace_bytes(1, 40, 64, 3, 80, 100, 2) == 40 * 100 * 3
    assert lib.cdnet_resize_workspace_bytes(1, 40, 64, 3, 80, 100, 0) == 0                        # (the LDS form takes it)
    assert lib.cdnet_resize_workspace_bytes(1, 40, 64, 3, 40, 100, 2) == 0
    assert lib.cdnet_resize_workspace_bytes(2, 3000, 64, 3, 10, 100, 0) == 2 * 3000 * 100 * 3     # (too many rows for the LDS)
    assert lib.cdnet_resize_workspace_bytes(0, 40, 64, 3, 80, 100, 0) == 0


def test_label8_dilate_rejects_bad_arguments_without_a_gpu():
    from cdnet_amd import _lib
    lib = _lib.load()
    err = lambda: lib.cdnet_last_error().decode()
    need = lib.cdnet_cc_workspace_bytes(1, 8, 8)

    def call(mask=FAKE, N=1, H=8, W=8, radius=2, ws=FAKE, nws=need, label=None, final=FAKE + 65536, counts=FAKE):
        return lib.cdnet_label8_dilate(mask, N, H, W, radius, ws, nws, label, final, counts, None)
    for kw in (dict(mask=None), dict(ws=None), dict(final=None), dict(counts=None)):
        assert call(**kw) == 1 and 'null pointer' in err(), kw
    for kw in (dict(N=0), dict(H=0), dict(W=-3)):
        assert call(**kw) == 1 and 'bad size' in err(), kw
    for r in (-1, 9):
        assert call(radius=r) == 1 and 'radius %d' % r in err()
    assert call(nws=need - 1) == 2 and 'workspace' in err()
    assert call(label=FAKE + 65536 + 16) == 1 and 'overlaps' in err()


def test_fill_remove_small_rejects_bad_arguments_without_a_gpu():
    from cdnet_amd import _lib
    lib = _lib.load()
    err = lambda: lib.cdnet_last_error().decode()
    need = lib.cdnet_cc_workspace_bytes(1, 8, 8)

    def call(pred=FAKE, N=1, H=8, W=8, ws=FAKE, nws=need, small=FAKE):
        return lib.cdnet_fill_remove_small(pred, 1, N, H, W, 20, ws, nws, small, None)
    for kw in (dict(pred=None), dict(ws=None), dict(small=None)):
        assert call(**kw) == 1 and 'null pointer' in err(), kw
    for kw in (dict(N=0), dict(H=-1), dict(W=0)):
        assert call(**kw) == 1 and 'bad size' in err(), kw
    assert call(H=40000, W=40000, nws=1 << 62) == 1 and 'too large' in err()
    assert call(nws=need - 1) == 2 and 'workspace' in err()


def test_build_lists_the_source():
    from cdnet_amd.csrc import build
    assert 'resize.hip' in build.SOURCES
    assert os.path.exists(os.path.join(build.HERE, 'resize.hip'))
