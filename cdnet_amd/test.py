"""Mask-only inference entry point with the reference's names (test.py), for networks with ONE mask output.

  get_probmaps(input, model, opt, branch_value)                      test.py:609-636  -> numpy [K,H,W] softmax of the logits
  save_results(header, avg_results, all_results, filename, mode='w') test.py:639-664
  process_image(model, image, opt, ori_size=None)                    test.py:213-296 for one image -> dict(final, pred, count[, prob_inside])
  image_metrics(pred_labeled, gt_instances)                          test.py:316-371: the 22 numbers of one row of <img_dir>_result.txt
  main(argv=None)                                                    test.py:34-606 (command line; images from opt.test['img_dir'])

Models: UNet, UNet_vgg16 (models/model_unet.py), FullNet (inference on csrc/dilated.hip), and the model_unet_MandD / MandD4 / MandD16 ablation heads through output[0] of their (mask, direction) pair (:629-630).  A network
with three outputs (UNet2RevA1_vgg16, model_unet_MandDandP, HRNet18_rev1) is refused with a ValueError - cdnet_amd.test_dam evaluates those (the
reference's test.py fails on them too).

The 'scale' test transform (--scale N, or opt.transform['test']['scale'] set by hand; my_transforms_direction.py:38-65, :281-283) runs on the
device: the decoded bytes are uploaded, resized with Pillow's bilinear filter (csrc/resize.hip, bit-exact), converted and normalised there; the
cleaned mask is resized back to the original size before it is labelled and dilated.  Not with --postproc 1 (ValueError).

Not carried over: --groundtruth 1 (XML annotations: NotImplementedError, as in test_dam);
the experiments/*_logExl_*.csv bookkeeping (:80-92, :459-606); _seg_colored.png (random colours, :382-394); AJI_sklearn (:309-311, :400, :425:
only printed, and sklearn's jaccard_score with average='samples' on {0, 255} arrays does not run on current scikit-learn).
"""
import os
import sys
import traceback

import numpy as np
import torch

from . import checkpoint, pipeline, postproc, stats_utils, utils
from .options import Options
from .test_dam import _dist_env, evaluate_labels, gather_results, ground_truth_instances, shard_names

# networks whose forward has one mask output (or (mask, direction), read through output[0])
MASK_MODELS = ('UNet', 'model_unet_MandD', 'model_unet_MandD4', 'model_unet_MandD16', 'FullNet', 'UNet_vgg16')

# the 22 columns of <img_dir basename>_result.txt (test.py:442-455)
HEADER = ['pixel_acc', 'pixel_IoU', 'pixel_Recall', 'pixel_Precision', 'pixel_F1', 'recall', 'precision', 'F1', 'Dice', 'IoU', 'Hausdorff',
          'AJI', 'AJI_h', 'Dice_h', 'result_Dice2', 'dq_value', 'sq_value', 'pq_value', 'Ana_FP', 'Ana_FN', 'Ana_less', 'Ana_more']


def check_model_name(name):
    if name not in MASK_MODELS:
        raise ValueError("model '{}' does not have one mask output: cdnet_amd.test evaluates {} - use `python -m cdnet_amd.test_dam` for "
                         "networks with mask, point and direction outputs".format(name, ', '.join(MASK_MODELS)))


def get_probmaps(input, model, opt, branch_value=1):
    """input: float tensor [1,C,H,W].  Whole-image forward when opt.all_img_test == 1, else utils.split_forward with the test patch size and
    overlap; returns F.softmax(output, dim=0) as a numpy array [K,H,W] (cdnet_mask_views_argmax with one view)."""
    x = input[0].cuda().float()
    _, H, W = x.shape
    with torch.no_grad():
        if opt.all_img_test == 1:
            views = utils.split_forward_views(model, x, max(H, W), 0, (0,))
            mask = views[0][0]
        else:
            mask = utils.split_forward(model, input, opt.test['patch_size'], opt.test['overlap'], opt)[0]
        prob = postproc.mask_views_argmax(mask[None], [0], H, W, want_prob=True)['prob_mean']
    return prob[0].cpu().numpy()


def save_results(header, avg_results, all_results, filename, mode='w'):
    """ Save the result of metrics
        results: a list of numbers
    (test.py:639-664: a header row, the averages, a blank line, one row per image sorted by name)"""
    N = len(header)
    assert N == len(avg_results)
    with open(filename, mode) as file:
        file.write('Metrics:\t')
        for i in range(N - 1):
            file.write('{:s}\t'.format(header[i]))
        file.write('{:s}\n'.format(header[N - 1]))
        file.write('Average:\t')
        for i in range(N - 1):
            file.write('{:.4f}\t'.format(avg_results[i]))
        file.write('{:.4f}\n'.format(avg_results[N - 1]))
        file.write('\n')
        for key, values in sorted(all_results.items()):
            file.write('{:s}:'.format(key))
            for value in values:
                file.write('\t{:.4f}'.format(value))
            file.write('\n')


def process_image(model, image, opt, ori_size=None):
    """image: float tensor [3,H,W] (after the test transform).  Returns dict(final=np.int32 [H,W] (the dilated label map, :295), pred=np.uint8,
    count=int[, prob_inside=np.float32 [H,W] when opt.test['save_flag']]).
    With 'scale' in opt.transform['test'] (pipeline.scale_inputs): image is the uint8 image [ori_h,ori_w,3] before the transform (resized,
    converted and normalised on the device), the transformed float tensor at the original size (the Scale step then runs on the device), or
    the float tensor the caller scaled already together with ori_size=(ori_h, ori_w); `final` is at the original size (:281-295), `pred` and
    `prob_inside` at the scaled one."""
    want_prob = bool(opt.test.get('save_flag', True))
    x, restore = pipeline.scale_inputs(image, opt, ori_size)
    r = pipeline.infer_image_mask(model, x, opt, want_prob=want_prob, restore=restore)
    out = dict(final=r['final'].cpu().numpy(), pred=r['pred'].cpu().numpy(), count=r['count'])
    if want_prob:
        out['prob_inside'] = r['prob_mean'][min(1, r['prob_mean'].shape[0] - 1)].cpu().numpy()
    return out


def image_metrics(pred_labeled, gt_instances):
    """One row of the result file (test.py:316-371, branch 5): pixel accuracy / IoU / recall / precision / F1 of foreground vs foreground
    (test_dam.evaluate_labels' pixel part), utils.nuclei_accuracy_object_level, then - on utils.measure_label of both maps (:339-340) -
    stats_utils.get_fast_aji (AJI_h and the four Ana_*), get_dice_1 (Dice_h), result_Dice2 = 0 (as the reference sets it, :344) and
    get_fast_pq's DQ / SQ / PQ.  Returns (row: 22 floats in HEADER order, the relabelled prediction)."""
    pix = evaluate_labels(pred_labeled, gt_instances)
    obj = utils.nuclei_accuracy_object_level(pred_labeled, gt_instances)
    pl, gl = utils.measure_label(pred_labeled), utils.measure_label(gt_instances)
    aji, ana_fp, ana_fn, ana_less, ana_more = stats_utils.get_fast_aji(gl, pl)
    dice = stats_utils.get_dice_1(gl, pl)
    (dq, sq, pq), _ = stats_utils.get_fast_pq(gl, pl, match_iou=0.5)
    row = [pix['pixel_accu'], pix['pixel_iou'], pix['pixel_recall'], pix['pixel_precision'], pix['pixel_F1'], *obj, aji, dice, 0.0,
           dq, sq, pq, ana_fp, ana_fn, ana_less, ana_more]
    return [float(v) for v in row], pl


def _load_model(opt, trusted):
    """utils.chooseModel + the checkpoint, exactly as test_dam.main loads them (test.py:94-105)"""
    model = utils.chooseModel(opt).cuda()
    if os.path.exists(opt.test['model_path']):
        checkpoint.load_checkpoint(opt.test['model_path'], model, strict=False, trusted_pickle=trusted)      # DataParallel prefix (:101-102)
    elif os.environ.get('CDNET_ALLOW_RANDOM_WEIGHTS') == '1':
        print("=> no checkpoint at '{}': evaluating RANDOM weights (CDNET_ALLOW_RANDOM_WEIGHTS=1)".format(opt.test['model_path']))
    else:
        # the reference's torch.load raises here (:101); a mistyped path must not produce plausible-looking metrics
        raise FileNotFoundError("checkpoint '{}' not found (set CDNET_ALLOW_RANDOM_WEIGHTS=1 to evaluate an untrained model)"
                                .format(opt.test['model_path']))
    model.eval()
    return model


def _run_shard(opt, trusted, mine):
    """this rank's images: pipelined like test_dam.main - image i + 1's forward and post-processing are queued before image i's results are
    waited for (its device-to-host copy runs on a copy stream into pinned memory).  Returns {name: row}."""
    from PIL import Image
    model = _load_model(opt, trusted)
    img_dir, label_dir, save_dir = opt.test['img_dir'], opt.test['label_dir'], opt.test['save_dir']
    save_flag, branch = bool(opt.test.get('save_flag', True)), opt.test['branch']
    base = img_dir.rstrip('/').split('/')[-1]
    seg_folder = '{:s}/{:s}_segmentation'.format(save_dir, base)
    prob_folder = '{:s}/{:s}_prob_maps'.format(save_dir, base)
    if save_flag:
        os.makedirs(seg_folder, exist_ok=True)
        os.makedirs(prob_folder, exist_ok=True)
    dev = torch.device('cuda', torch.cuda.current_device())
    copy_stream = torch.cuda.Stream(device=dev)
    rows = {}
    in_c = opt.model.get('in_c', 3)                    # 1: a grey-scale dataset, read as mode L

    def launch(f):
        if 'scale' in opt.transform['test']:
            # the decoded bytes go up as they are; resize, conversion and normalisation run on the device (pipeline.scaled_input), and the
            # mask comes back at the original size (restore); the probability map stays at the scaled size, where the reference saves it
            raw = torch.from_numpy(np.array(Image.open(os.path.join(img_dir, f)).convert('L' if in_c == 1 else 'RGB'), dtype=np.uint8))
            x, restore = pipeline.scaled_input(raw, opt.transform['test'], dev)
            r = pipeline.infer_image_mask(model, x, opt, want_prob=save_flag, defer=True, restore=restore)
        else:
            x = pipeline.host_input(Image.open(os.path.join(img_dir, f)), opt.transform['test'], in_c)
            r = pipeline.infer_image_mask(model, x.pin_memory().to(dev, non_blocking=True), opt, want_prob=save_flag, defer=True)
        dev_out = {'final': r['final']}
        if save_flag:
            pm = r['prob_mean']
            dev_out['prob_inside'] = pm[min(1, pm.shape[0] - 1)]            # (plane 1, test.py:376; a one-channel model has plane 0 only)
        done = torch.cuda.Event()
        done.record()
        host = {k: torch.empty(v.shape, dtype=v.dtype).pin_memory() for k, v in dev_out.items()}
        copy_stream.wait_event(done)
        with torch.cuda.stream(copy_stream):
            for k, h in host.items():
                dev_out[k].record_stream(copy_stream)
                h.copy_(dev_out[k], non_blocking=True)
            copied = torch.cuda.Event()
            copied.record(copy_stream)
        return f, host, copied

    def finish(item):
        f, host, copied = item
        copied.synchronize()
        name = os.path.splitext(f)[0]
        pred_labeled = host['final'].numpy()
        print('{:s}: {:d} nuclei'.format(f, int(len(np.unique(pred_labeled[pred_labeled > 0])))))
        gt = ground_truth_instances(label_dir, name) if label_dir and os.path.isdir(label_dir) else None
        if gt is not None and gt.shape == pred_labeled.shape:
            row, pred_labeled = image_metrics(pred_labeled, gt)   # (the reference saves the relabelled map: :339 overwrites, :379 saves)
            rows[name] = row
            print('\timage {:s}, the pixel_iou = {:.4f}, pixel_F1 = {:.4f}, AJI_h = {:.4f}, PQ = {:.4f}'.format(f, row[1], row[4], row[12], row[17]))
        if save_flag:
            Image.fromarray((host['prob_inside'].numpy() * 255).astype(np.uint8)).save(
                '{:s}/b{:s}_{:s}_prob_inside.png'.format(prob_folder, str(branch), name))
            Image.fromarray(pred_labeled.astype(np.uint16)).save('{:s}/b{:s}_{:s}_seg.tiff'.format(seg_folder, str(branch), name))

    pending = None
    for f in mine:
        item = launch(f)
        if pending is not None:
            finish(pending)
        pending = item
    if pending is not None:
        finish(pending)
    return rows


def _gather_status(ok, error, rank, world):
    """(ok, error) of every rank, on every rank - so that all of them stop together when one has failed (a failing rank still reaches this
    collective: its exception was caught)"""
    if world <= 1:
        return [(ok, error)]
    import torch.distributed as dist
    parts = [None] * world
    dist.all_gather_object(parts, (ok, error))
    return parts


def main(argv=None):
    """The reference's test loop (test.py:34-606) sharded by image over the ranks of one node and pipelined inside a rank, as test_dam.main:
    rank r takes names[r::world].  Each rank reports (ok, error) to every other rank, then its metric rows are gathered on rank 0, which alone
    writes <save_dir>/<img_dir basename>_result.txt and returns the averages (the other ranks return None).  When a rank fails, no rank
    hangs: rank 0 names the failing rank(s) and every rank raises (a non-zero exit)."""
    argv = list(sys.argv[1:] if argv is None else argv)
    trusted = '--trusted-pickle' in argv                    # legacy checkpoints that need full unpickling (trusted source only)
    argv = [a for a in argv if a != '--trusted-pickle']
    opt = Options(isTrain=False).parse(argv)
    if opt.test.get('groundtruth', 0) == 1:
        # test.py:331-333: object metrics against the XML annotations (utils.nuclei_accuracy_annotation_object_level)
        raise NotImplementedError('--groundtruth 1 (XML annotation files) is outside the accelerated path: supply instance labels')
    check_model_name(opt.model['modelName'])
    if 'scale' in opt.transform['test'] and int(opt.post['postproc']) == 1:
        raise ValueError(postproc.SCALE_POSTPROC1)
    rank, world, made_group = _dist_env()
    if torch.cuda.device_count() > 1:
        torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', '0')) % torch.cuda.device_count())
    img_dir = opt.test['img_dir']
    names = sorted(f for f in os.listdir(img_dir) if f.endswith('png')) if os.path.isdir(img_dir) else []
    os.makedirs(opt.test['save_dir'], exist_ok=True)
    ok, error, rows = True, None, {}
    try:
        rows = _run_shard(opt, trusted, shard_names(names, rank, world))
    except Exception as e:                                  # (reported to every rank below instead of leaving them in the gather)
        if world <= 1:
            raise
        ok, error = False, '{}: {}'.format(type(e).__name__, e)
        traceback.print_exc()
    status = _gather_status(ok, error, rank, world)
    failed = [(r, s[1]) for r, s in enumerate(status) if not s[0]]
    merged = gather_results(rows, rank, world) if not failed else None
    if made_group:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    if failed:
        what = '; '.join('rank {:d} failed: {}'.format(r, e) for r, e in failed)
        if rank == 0:
            print('cdnet_amd.test: ' + what, file=sys.stderr)
        raise RuntimeError(what if rank == 0 or not ok else 'rank {:d} stops: {}'.format(rank, what))
    avg = None
    if rank == 0 and merged:
        meter = utils.AverageMeter(len(HEADER))                  # (test.py:122, 368-371; rows in name order: independent of the rank count)
        for k in sorted(merged):
            meter.update(merged[k])
        avg_results = meter.avg
        base = img_dir.rstrip('/').split('/')[-1]
        save_results(HEADER, avg_results, merged, '{:s}/{:s}_result.txt'.format(opt.test['save_dir'], base))
        avg = {k: float(v) for k, v in zip(HEADER, avg_results)}
        print('Average of {:d} images: '.format(len(merged)) + ', '.join('{:s} = {:.4f}'.format(k, v) for k, v in avg.items()))
    return avg


if __name__ == '__main__':
    main()
