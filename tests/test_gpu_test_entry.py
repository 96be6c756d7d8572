"""GPU tests of the mask-only inference entry (cdnet_amd.test, the reference's test.py): UNet.forward_packed, utils.split_forward,
pipeline.infer_image_mask against the reference's arithmetic and the CPU oracle, and test.main on image folders - one process, two ranks,
a failing rank, the ablation heads."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _unet(seed=1, K=3):
    import torch
    from cdnet_amd.models.unet import UNet
    torch.manual_seed(seed)
    return UNet(num_classes=K).cuda().eval()


def test_forward_packed_is_forward():
    import torch
    from cdnet_amd import runtime, synth
    m = _unet()
    x = torch.from_numpy(synth.det_input((2, 3, 64, 96), 3)).cuda()
    with torch.no_grad():
        want = m(x)
        got, = m.forward_packed(runtime.input_pack(x))
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32))


def restated_split_forward(forward, x, size, overlap, out_c):
    """the reference's loop (utils.py:610-654): zero padding, a forward per window, the kept region pasted"""
    import torch
    b, c, h0, w0 = x.shape
    if h0 - size > 0:
        x = torch.cat((x, torch.zeros((b, c, (size - overlap) - (h0 - size) % (size - overlap), w0))), dim=2)
    if w0 - size > 0:
        x = torch.cat((x, torch.zeros((b, c, x.shape[2], (size - overlap) - (w0 - size) % (size - overlap)))), dim=3)
    _, c, h, w = x.shape
    output = torch.zeros((b, out_c, h, w))
    for i in range(0, h - overlap, size - overlap):
        r_end = i + size if i + size < h else h
        ind1_s = i + overlap // 2 if i > 0 else 0
        ind1_e = i + size - overlap // 2 if i + size < h else h
        for j in range(0, w - overlap, size - overlap):
            c_end = j + size if j + size < w else w
            with torch.no_grad():
                patch = forward(x[:, :, i:r_end, j:c_end]).float().cpu()
            ind2_s = j + overlap // 2 if j > 0 else 0
            ind2_e = j + size - overlap // 2 if j + size < w else w
            output[:, :, ind1_s:ind1_e, ind2_s:ind2_e] = patch[:, :, ind1_s - i:ind1_e - i, ind2_s - j:ind2_e - j]
    return output[:, :, :h0, :w0]


def test_split_forward_vs_reference_loop_and_oracle():
    import torch
    from cdnet_amd import synth, utils
    from cdnet_amd.models.unet import UNet
    from oracle import models as om
    ref = om.det_fill(om.UNet(3)).eval()
    m = UNet(3)
    m.load_state_dict(ref.state_dict())
    m = m.cuda().eval()
    x = torch.from_numpy(synth.det_input((1, 3, 120, 152), 6, bf16_exact=True))
    got = utils.split_forward(m, x, 64, 16, None)
    assert tuple(got.shape) == (1, 3, 120, 152) and got.is_cuda
    got = got.cpu()
    want = restated_split_forward(lambda t: m(t.cuda()), x, 64, 16, 3)
    assert np.array_equal(got.numpy().view(np.uint32), want.numpy().view(np.uint32))
    orc = restated_split_forward(ref, x, 64, 16, 3)
    scale = orc.abs().max()
    err = (got - orc).abs()
    assert err.max() <= 8e-2 * scale and err.mean() <= 1e-2 * scale, (float(err.max()), float(err.mean()), float(scale))


def _per_view_reference(m, img, size, overlap):
    """per-view logits -> the kernel's probabilities of each view alone -> un-flipped, float32 mean in view order, arg-max (test.py:216-275)"""
    import torch
    from cdnet_amd import postproc, utils
    from test_gpu_mask_postproc import unflip
    _, H, W = img.shape
    views = utils.split_forward_views(m, img, size, overlap, postproc.TTA_XFORMS)
    s = None
    for xf, (mask,) in zip(postproc.TTA_XFORMS, views):
        K, hv, wv = mask.shape
        p = postproc.mask_views_argmax(mask.reshape(1, 1, K, hv * wv), [0], hv, wv, want_prob=True)['prob_mean'][0].cpu().numpy()
        p = unflip(p, xf)
        s = p if s is None else s + p
    mean = s / 8
    return mean, np.argmax(mean, axis=0).astype(np.uint8)


def test_infer_image_mask_tta_windows_vs_oracle():
    import torch
    from cdnet_amd import pipeline, synth
    from oracle import postproc as orc
    m = _unet(2)
    H, W = 120, 152
    img = torch.from_numpy(synth.det_input((3, H, W), 8)).cuda()
    r = pipeline.infer_image_mask(m, img, tta=True, all_img_test=0, patch_size=64, overlap=16, want_prob=True)
    mean, pred = _per_view_reference(m, img, 64, 16)
    assert np.array_equal(r['prob_mean'].cpu().numpy(), mean)
    assert np.array_equal(r['pred'].cpu().numpy(), pred)
    want = orc.cc_chain(pred == 1, 20, 2)
    assert np.array_equal(r['final'].cpu().numpy(), want['final'])
    assert r['count'] == want['count']
    # whole-image forward: the same chain on the whole-image views
    r1 = pipeline.infer_image_mask(m, img, tta=True, all_img_test=1)
    _, pred1 = _per_view_reference(m, img, max(H, W), 0)
    assert np.array_equal(r1['pred'].cpu().numpy(), pred1)
    assert np.array_equal(r1['final'].cpu().numpy(), orc.cc_chain(pred1 == 1, 20, 2)['final'])


def test_infer_image_mask_watershed_variant_vs_oracle():
    import torch
    from cdnet_amd import pipeline, synth
    from oracle import postproc as orc
    m = _unet(4)
    H, W = 96, 112
    img = torch.from_numpy(synth.det_input((3, H, W), 9)).cuda()
    r = pipeline.infer_image_mask(m, img, tta=True, all_img_test=0, patch_size=64, overlap=16, postproc=1, min_area=20, radius=2)
    _, pred = _per_view_reference(m, img, 64, 16)
    assert np.array_equal(r['pred'].cpu().numpy(), pred)
    lab = orc.watershed_process((pred == 1).astype(np.uint8) * 255, min_size=20)['labels']
    want = orc.dilate_disk(lab, 2)
    assert np.array_equal(r['final'].cpu().numpy(), want)
    assert r['count'] == len(np.unique(want[want > 0]))


def _trained_unet_checkpoint(tmp_path):
    import torch
    from cdnet_amd import checkpoint, synth, trainer
    m = _unet(0)
    m.train()
    tr = trainer.UNetTrainer(m)
    lab, _, _, weight = synth.train_targets(2, 64, 64, 31)
    x = torch.from_numpy(synth.det_input((2, 3, 64, 64), 12)).cuda()
    labd, wd = torch.from_numpy(lab).cuda(), torch.from_numpy(weight)[:, 0].contiguous().cuda()
    for _ in range(3):
        tr.train_step(x, labd, wd)
    return checkpoint.save_checkpoint(checkpoint.make_state(m, tr, 0), 0, True, str(tmp_path), 'Main', 0)


def _args(tmp_path, ck, extra=()):
    return ['--model-name', 'UNet', '--direction', '0', '--img-dir', str(tmp_path / 'images' / 'test1'),
            '--label-dir', str(tmp_path / 'labels' / 'test1'), '--model-path', ck] + list(extra)


def test_main_writes_results_and_rows_match_saved_maps(tmp_path):
    from PIL import Image
    from test_data_folder import make_dataset
    from cdnet_amd import test, test_dam
    make_dataset(tmp_path, n=3, size=(96, 112), seed=5, sub='test1')
    ck = _trained_unet_checkpoint(tmp_path)
    out = tmp_path / 'out'
    avg = test.main(_args(tmp_path, ck, ['--save-dir', str(out)]))
    assert avg is not None and list(avg) == test.HEADER and len(test.HEADER) == 22
    assert all(np.isfinite(v) for v in avg.values()), avg
    lines = open(out / 'test1_result.txt').read().split('\n')
    assert lines[0].split('\t') == ['Metrics:'] + test.HEADER and lines[1].startswith('Average:\t') and lines[2] == ''
    rows = {ln.split(':')[0]: [float(v) for v in ln.split('\t')[1:]] for ln in lines[3:] if ln}
    assert sorted(rows) == ['im0', 'im1', 'im2']
    for name, row in rows.items():
        assert len(row) == 22
        seg = np.asarray(Image.open(out / 'test1_segmentation' / ('b5_%s_seg.tiff' % name))).astype(np.int32)
        prob = np.asarray(Image.open(out / 'test1_prob_maps' / ('b5_%s_prob_inside.png' % name)))
        assert seg.shape == prob.shape == (96, 112) and prob.dtype == np.uint8
        gt = test_dam.ground_truth_instances(str(tmp_path / 'labels' / 'test1'), name)
        want, relab = test.image_metrics(seg, gt)
        assert np.array_equal(relab, seg)                           # (the saved map is the relabelled one, test.py:339, 379)
        assert np.allclose(row, [float('{:.4f}'.format(v)) for v in want], rtol=0, atol=1e-9), (name, row, want)
    means = np.mean([rows[k] for k in sorted(rows)], axis=0)
    assert np.allclose([float(v) for v in lines[1].split('\t')[1:]], means, atol=1.5e-4)


def _spawn_world2(tmp_path, args, two):
    import socket
    import subprocess
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), '_test_entry_world2_worker.py')
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK='0', WORLD_SIZE='2', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, worker, two] + args + ['--save-dir', two], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
    res = []
    for p in procs:
        try:
            o, e = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        res.append((p.returncode, o, e))
    return res


def test_main_two_ranks_and_a_failing_rank(tmp_path):
    import json
    from PIL import Image
    from test_data_folder import make_dataset
    from cdnet_amd import test
    make_dataset(tmp_path, n=5, size=(96, 112), seed=7, sub='test1')
    ck = _trained_unet_checkpoint(tmp_path)
    args = _args(tmp_path, ck)
    one = str(tmp_path / 'one')
    want = test.main(args + ['--save-dir', one])
    two = str(tmp_path / 'two')
    os.makedirs(two)
    for code, o, e in _spawn_world2(tmp_path, args, two):
        assert code == 0, o[-2000:] + '\n' + e[-4000:]
    got0, got1 = [json.load(open(os.path.join(two, 'rank%d.json' % r))) for r in range(2)]
    assert got1 is None and got0 == want
    for i in range(5):
        f = 'test1_segmentation/b5_im%d_seg.tiff' % i
        assert np.array_equal(np.asarray(Image.open(os.path.join(one, f))), np.asarray(Image.open(os.path.join(two, f)))), i
    assert open(os.path.join(one, 'test1_result.txt')).read() == open(os.path.join(two, 'test1_result.txt')).read()
    # rank 1's shard (im1, im3) gets an unreadable PNG: a host-side decode error - both ranks stop, non-zero, rank 0 names rank 1
    with open(tmp_path / 'images' / 'test1' / 'im1.png', 'wb') as fh:
        fh.write(b'not a png at all')
    bad = str(tmp_path / 'bad')
    os.makedirs(bad)
    (c0, o0, e0), (c1, o1, e1) = _spawn_world2(tmp_path, args, bad)
    assert c0 != 0 and c1 != 0, (c0, c1)
    assert 'rank 1 failed' in e0, e0[-3000:]
    assert not os.path.exists(os.path.join(bad, 'test1_result.txt'))


def test_ablation_head_runs_and_three_output_model_is_refused(tmp_path, monkeypatch):
    from test_data_folder import make_dataset
    from cdnet_amd import test
    make_dataset(tmp_path, n=2, size=(64, 80), seed=3, sub='test1')
    monkeypatch.setenv('CDNET_ALLOW_RANDOM_WEIGHTS', '1')
    base = ['--img-dir', str(tmp_path / 'images' / 'test1'), '--label-dir', str(tmp_path / 'labels' / 'test1'),
            '--model-path', str(tmp_path / 'missing.pth'), '--save-dir', str(tmp_path / 'out')]
    avg = test.main(['--model-name', 'model_unet_MandD'] + base)
    assert avg is not None and len(avg) == 22 and all(np.isfinite(v) for v in avg.values()), avg
    assert os.path.exists(tmp_path / 'out' / 'test1_segmentation' / 'b5_im1_seg.tiff')
    with pytest.raises(ValueError, match='test_dam'):
        test.main(['--model-name', 'UNet2RevA1_vgg16'] + base)
