"""The mask-only inference path (cdnet_amd.test, the reference's test.py) on the device; prints ONE JSON line.
    python3 tools/bench_mask_infer.py [steps]
    rocprofv3 --kernel-trace --stats -d <dir> -- python3 tools/bench_mask_infer.py      per-kernel durations
Legs (torch.cuda events around synchronised windows, after warm-up):
  tiles_*      plain UNet, B = 64 tiles of 256^2 incl. post-processing (on the side stream, as infer_tiles runs it), bf16 and fp32: tiles/s
  post64_*     the post-processing of 64 mask-only tiles alone: the two-launch chain (cdnet_tile_mask_postproc) vs the per-step one
               (cdnet_mask_views_argmax with one view + cdnet_cc_chain), ms per batch
  image_*      ms per 1000 x 1000 image with 8 TTA views: whole-image forward and 256/40 windows, with and without the post-processing
  kernels      algorithmic bytes and GB/s of the view-mean kernel: 8 views of 1000^2 (K = 3), and one view of 64 x 256^2 (the bytes of the
               tile class kernel, whose own duration is in the rocprofv3 summary)
  box          bench.box_calibration: what this box grants (copy GB/s, matrix clock)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch


def timed(fn, steps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    from cdnet_amd import _lib, pipeline, postproc, runtime, streams, synth
    from cdnet_amd.models.unet import UNet
    import bench
    dev = torch.device('cuda:0')
    torch.cuda.set_device(0)
    _lib.load()
    res = {'metric': 'mask_only_inference', 'steps': steps}
    res['box'] = bench.box_calibration(torch, dev)
    torch.manual_seed(0)
    m = UNet(num_classes=3).cuda().eval()

    # 1. plain-UNet tiles incl. post-processing on the side stream
    x = torch.from_numpy(synth.det_input((64, 3, 256, 256), 3)).to(dev)
    side = streams.side_stream()
    for prec in ('bf16', 'fp32'):
        runtime.set_precision(prec)
        m._rt = None                                               # (weights re-packed for the precision)
        ms = timed(lambda: pipeline.infer_tiles_mask(m, x, post_stream=side), steps)
        res['tiles_%s' % prec] = {'ms_per_batch': ms, 'tiles_per_s': 64 / ms * 1e3}
    runtime.set_precision('bf16')
    m._rt = None

    # 2. post-processing of 64 mask-only tiles alone
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from test_gpu_mask_postproc import nuclei_logits
    lg = torch.from_numpy(nuclei_logits(64, 256, 256, seed=11)).to(dev)
    fused = timed(lambda: postproc.tile_mask_postproc(lg, 20, 2), steps * 5)
    per_step = timed(lambda: postproc.cc_chain(postproc.mask_views_argmax(lg, [0], 256, 256)['pred'], 1, 20, 2), steps * 5)
    res['post64'] = {'two_launch_ms': fused, 'per_step_ms': per_step, 'launches_two_launch': 2}

    # 3. one 1000 x 1000 image, 8 views
    img = torch.from_numpy(synth.det_input((3, 1000, 1000), 4)).to(dev)
    from cdnet_amd import utils
    for name, aig in (('whole', 1), ('win256_40', 0)):
        full = timed(lambda: pipeline.infer_image_mask(m, img, all_img_test=aig, defer=True), max(2, steps // 2), warmup=2)
        buf = torch.empty((8, 3, 1000 * 1000), dtype=torch.float32, device=dev)
        size, ov = (1000, 0) if aig == 1 else (256, 40)
        fwd = timed(lambda: utils.split_forward_views(m, img, size, ov, postproc.TTA_XFORMS, out=(buf,)), max(2, steps // 2), warmup=2)
        res['image_' + name] = {'ms_with_post': full, 'ms_forward_only': fwd}
    buf = torch.empty((1, 8, 3, 1000 * 1000), dtype=torch.float32, device=dev).normal_()
    post = timed(lambda: postproc.cc_chain(postproc.mask_views_argmax(buf, postproc.TTA_XFORMS, 1000, 1000)['pred'], 1, 20, 2), steps * 5)
    res['image_post_ms'] = post

    # 4. the view-mean kernel alone
    kv = timed(lambda: postproc.mask_views_argmax(buf, postproc.TTA_XFORMS, 1000, 1000), steps * 10)
    bv = 8 * 3 * 4 * 1e6 + 1e6                                     # 96 B read + 1 B written per pixel
    # (tile_mask_pred_kernel has no entry of its own - its duration is in the rocprofv3 trace; here the view-mean kernel with ONE view on the
    #  same 64 tiles: the same bytes, 12 B read + 1 B written per pixel)
    kt = timed(lambda: postproc.mask_views_argmax(lg, [0], 256, 256), steps * 10)
    bt = 64 * 65536 * (12 + 1)
    res['kernels'] = {'mask_views_8x1000sq': {'ms': kv, 'bytes': bv, 'GBps': bv / kv / 1e6},
                      'mask_views_1view_64x256sq': {'ms': kt, 'bytes': bt, 'GBps': bt / kt / 1e6}}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
