"""Host-side checks of the mask-only inference entry (cdnet_amd.test) and its C entries: argument handling, the result file's layout, and the
argument checks of the new library entries (which fail before any HIP call, so no GPU is needed)."""
import ctypes as C

import pytest


def test_main_rejects_xml_ground_truth_and_three_output_models(tmp_path):
    from cdnet_amd import test
    base = ['--img-dir', str(tmp_path), '--save-dir', str(tmp_path / 'out'), '--model-path', str(tmp_path / 'none.pth')]
    with pytest.raises(NotImplementedError, match='groundtruth 1'):
        test.main(['--model-name', 'UNet', '--groundtruth', '1'] + base)
    for name in ('UNet2RevA1_vgg16', 'model_unet_MandDandP', 'HRNet18_rev1'):
        with pytest.raises(ValueError, match='cdnet_amd.test_dam'):
            test.main(['--model-name', name] + base)
    with pytest.raises(SystemExit):
        test.main(['--model-name', 'UNet', '--no-such-flag'])
    from cdnet_amd.options import Options
    opt = Options(isTrain=False).parse(['--model-name', 'UNet', '--direction', '0', '--postproc', '1', '--all_img_test', '0',
                                        '--patch-size', '128', '--overlap', '24', '--min-area', '15', '--radius', '3', '--tta', '0'])
    assert opt.model['modelName'] == 'UNet' and opt.model['direction'] == 0 and opt.post == dict(postproc=1, min_area=15, radius=3)
    assert opt.all_img_test == 0 and opt.test['patch_size'] == 128 and opt.test['overlap'] == 24 and opt.test['tta'] is False


def test_save_results_layout(tmp_path):
    from cdnet_amd import test
    header = ['a', 'b', 'c']
    rows = {'im2': (0.5, 1.0, 0.25), 'im10': (1.0 / 3.0, 0.0, 2.0)}
    f = tmp_path / 'r.txt'
    test.save_results(header, [0.41666, 0.5, 1.125], rows, str(f))
    assert f.read_text() == ('Metrics:\ta\tb\tc\n'
                             'Average:\t0.4167\t0.5000\t1.1250\n'
                             '\n'
                             'im10:\t0.3333\t0.0000\t2.0000\n'
                             'im2:\t0.5000\t1.0000\t0.2500\n')
    test.save_results(header, [0, 0, 0], {}, str(f), mode='a+')
    assert f.read_text().endswith('im2:\t0.5000\t1.0000\t0.2500\nMetrics:\ta\tb\tc\nAverage:\t0.0000\t0.0000\t0.0000\n\n')
    with pytest.raises(AssertionError):
        test.save_results(header, [0, 0], rows, str(f))
    assert len(test.HEADER) == 22 and test.HEADER[11:14] == ['AJI', 'AJI_h', 'Dice_h'] and test.HEADER[-4:] == ['Ana_FP', 'Ana_FN', 'Ana_less', 'Ana_more']


def _lib():
    from cdnet_amd import _lib
    return _lib.load()


def _err(lib):
    return lib.cdnet_last_error().decode()


FAKE = C.c_void_p(4096)          # (never dereferenced: every call below fails its argument checks first)


def test_new_entries_reject_bad_arguments_without_a_gpu():
    lib = _lib()
    xf = (C.c_int * 8)(*range(8))
    xfp = C.cast(xf, C.c_void_p)
    assert lib.cdnet_mask_views_argmax(None, 1, 8, 3, xfp, 16, 16, None, FAKE, None) == 1 and 'null pointer' in _err(lib)
    assert lib.cdnet_mask_views_argmax(FAKE, 1, 8, 3, None, 16, 16, None, FAKE, None) == 1 and 'null pointer' in _err(lib)
    assert lib.cdnet_mask_views_argmax(FAKE, 1, 8, 4, xfp, 16, 16, None, FAKE, None) == 1 and 'K=4' in _err(lib)
    assert lib.cdnet_mask_views_argmax(FAKE, 1, 17, 3, xfp, 16, 16, None, FAKE, None) == 1 and 'bad size' in _err(lib)
    assert lib.cdnet_mask_views_argmax(FAKE, 1, 8, 3, xfp, 0, 16, None, FAKE, None) == 1 and 'bad size' in _err(lib)
    bad = (C.c_int * 8)(0, 1, 2, 3, 4, 5, 6, 8)
    assert lib.cdnet_mask_views_argmax(FAKE, 1, 8, 3, C.cast(bad, C.c_void_p), 16, 16, None, FAKE, None) == 1 and 'view_xform[7]=8' in _err(lib)

    args = lambda **kw: [kw.get('logits', FAKE), kw.get('B', 4), kw.get('K', 3), kw.get('H', 64), kw.get('W', 64), 20, kw.get('radius', 2),
                         kw.get('ws', FAKE), kw.get('wsb', 1 << 30), None, kw.get('pred', FAKE), None, None, None, kw.get('final', FAKE), FAKE, None]
    for kw, what in ((dict(logits=None), 'null pointer'), (dict(ws=None), 'null pointer'), (dict(pred=None), 'null pointer'),
                     (dict(final=None), 'null pointer'), (dict(K=0), 'K=0'), (dict(W=100), 'multiple of 64'), (dict(H=2048), 'multiple of 64'),
                     (dict(radius=9), 'radius 9')):
        assert lib.cdnet_tile_mask_postproc(*args(**kw)) == 1, kw
        assert what in _err(lib), (kw, _err(lib))
    assert lib.cdnet_tile_mask_postproc(*args(wsb=16)) == 2 and 'workspace' in _err(lib)

    assert lib.cdnet_dilate_labels(None, 1, 8, 8, 2, FAKE, None) == 1 and 'null pointer' in _err(lib)
    assert lib.cdnet_dilate_labels(FAKE, 1, 8, 8, 9, C.c_void_p(1 << 20), None) == 1 and 'radius 9' in _err(lib)
    assert lib.cdnet_dilate_labels(FAKE, 0, 8, 8, 2, C.c_void_p(1 << 20), None) == 1 and 'bad size' in _err(lib)
    assert lib.cdnet_dilate_labels(FAKE, 1, 8, 8, 2, C.c_void_p(4096 + 64), None) == 1 and 'overlaps' in _err(lib)


def test_tile_workspace_is_zero_for_shapes_not_served():
    lib = _lib()
    assert lib.cdnet_tile_mask_postproc_workspace_bytes(64, 3, 256, 256) >= 64 * 256 * 256 * 4 + 64 * 256 * 256 // 8
    for B, K, H, W in ((64, 2, 256, 256), (1, 1, 3, 64), (2, 3, 128, 512)):
        assert lib.cdnet_tile_mask_postproc_workspace_bytes(B, K, H, W) > 0
    for B, K, H, W in ((0, 3, 64, 64), (4, 0, 64, 64), (4, 4, 64, 64), (4, 3, 64, 100), (4, 3, 512, 256), (4, 3, 0, 64), (4, 3, 64, 0)):
        assert lib.cdnet_tile_mask_postproc_workspace_bytes(B, K, H, W) == 0, (B, K, H, W)
    from cdnet_amd import postproc
    assert postproc.tile_mask_postproc_eligible(64, 3, 256, 256) and not postproc.tile_mask_postproc_eligible(64, 3, 250, 250)
