"""`train` and `validate` of the plain UNet with the reference's signatures (train_util.py:58-259, :304-480).

`optimizer` is the object `cdnet_amd.utils.get_optimizer(opt, model)` returns for a UNet: the `UNetTrainer` that runs forward, the mask
loss (`cdnet_mask_loss`: cross-entropy x weight map, MulticlassDiceLoss, pixel metrics and the gradient in one entry), the optional
variance and boundary terms, backward and the optimiser step on the HIP kernels.  `criterion` is accepted and ignored.  A sample is
the reference's tuple (input f32 [B,3,H,W], weight_map u8 [B,1,H,W], target0 [B,1,H,W] with values {0,127/128,255} or [B,3,H,W]
one-hot colours); the five-tuples of the DAM loaders are taken too and their point / direction targets ignored.

The switches (options.py --weight-map, --dice, --alpha) act as in the reference:
  add_weightMap 0   the cross-entropy map is not weighted (:134-135)
  dice 0 / 1 / 2    no dice term / loss + loss_dice / loss = loss_dice alone (:183-190)
  alpha 0 / 1 / 2   no variance term / loss_CE + loss_var / 2 * loss_var instead of loss_CE (:138-155)
Two-class training (multi_class = False) and alpha = 3 (SSIM) raise ValueError."""
import numpy as np
import torch

from . import utils
from .train_util_dam import _label3


def _check_options(opt):
    """the option values this module serves -> the triple (dice, weight_map, alpha); ValueError otherwise"""
    if not opt.model.get('multi_class', True):
        raise ValueError('multi_class = False: two-class training is not built (the mask loss serves the three-class configuration)')
    dice, weight_map, alpha = opt.model.get('dice', 1), opt.model.get('add_weightMap', 1), opt.train.get('alpha', 0)
    utils.loss_terms(dice, weight_map, alpha)              # raises on dice 3, weight_map 2, alpha 3 (SSIM), ...
    return int(dice), int(weight_map), alpha


def epoch_scores(train_res, val_res=None):
    """(val_loss, val_iou, val_F1) of an epoch of the plain UNet as train.py:348-387 forms them: validate's [loss, accu, IoU, recall,
    precision, F1] when there is a validation result, else train's [loss, loss_CE, loss_var, accu, IoU, recall, precision, F1] standing
    in for it.  checkpoint_best follows val_iou and early stopping watches -val_F1 - val_iou, so neither may be a constant."""
    if val_res is not None:
        return float(val_res[0]), float(val_res[2]), float(val_res[5])
    return float(train_res[0]), float(train_res[4]), float(train_res[7])


def _unpack(sample, dev):
    input, weight_map, target0 = sample[0], sample[1], sample[2]
    label = _label3(target0.to(dev), 2).contiguous()
    w = weight_map.to(dev)
    w = (w[:, 0] if w.dim() == 4 else w).to(torch.uint8).contiguous()        # / 20 on the device (:109)
    return input.to(dev).float(), label, w


def train(train_loader, model, optimizer, criterion, epoch, opt, logger, get_process_worktime=1, get_process_detail=1, accuracy_tensor=0,
          dice_out=None):
    """-> results.avg: [loss, loss_CE, loss_var (-1 unless alpha is 1 or 2), pixel_accu, pixel_iou, pixel_recall, pixel_precision, pixel_F1]
    (:225, :259).  dice_out: an optional list that receives the epoch's mean dice term (the reference does not log it)."""
    trainer = optimizer
    dice, weight_map, alpha = _check_options(opt)
    trainer.dice, trainer.weight_map, trainer.alpha = dice, weight_map, float(alpha)
    results = utils.AverageMeter(9)
    dev = trainer.dev
    for i, sample in enumerate(train_loader):
        x, label, w = _unpack(sample, dev)
        trainer.train_step(x, label, w)
        r = trainer.mask_losses.detach().cpu().numpy().astype(np.float64)          # total, ce, dice, 5 metrics
        lv = float(trainer.loss_var.item()) if alpha in (1, 2) else -1.0
        results.update([r[0], r[1], lv, r[3], r[4], r[5], r[6], r[7], r[2]], x.size(0))
        if i % opt.train['log_interval'] == 0 and logger is not None:
            logger.info('\tIteration: [{:d}/{:d}]\t Loss {r[0]:.4f}\tLoss_CE {r[1]:.4f}\tLoss_var {r[2]:.4f}\tPixel_Accu {r[3]:.4f}'
                        '\n\t\t\t\t\t\t\t pixel_IoU {r[4]:.4f}\tpixel_Recall {r[5]:.4f}\tpixel_Precision {r[6]:.4f}\tpixel_F1 {r[7]:.4f}'
                        .format(i, len(train_loader), r=results.avg))
    avg = results.avg
    if getattr(trainer, 'world', 1) > 1:
        avg = np.asarray(trainer.reduce_scalars(avg))             # global-batch means, as DataParallel's gathered loss gives
    if logger is not None:
        logger.info('\t=> Train Avg: \t Loss {r[0]:.4f}\tLoss_CE {r[1]:.4f}\tLoss_var {r[2]:.4f}\tPixel_Accu {r[3]:.4f}'
                    '\n\t\t\t\t\t\t\t pixel_IoU {r[4]:.4f}\tpixel_Recall {r[5]:.4f}\tpixel_Precision {r[6]:.4f}\tpixel_F1 {r[7]:.4f}'
                    .format(r=avg))
    if dice_out is not None:
        dice_out.append(float(avg[8]))
    return avg[:8]


def mask_loss_values(logits, label, weight, terms, ws=None):
    """the eight values of cdnet_mask_loss (no gradient) of logits f32 [B,3,H,W] against label u8 [B,H,W] as a device tensor"""
    from . import _lib
    B, K, H, W = logits.shape
    if K != 3:
        raise ValueError('the mask loss serves three-class logits, got %s' % (tuple(logits.shape),))
    need = _lib.load().cdnet_mask_loss_workspace_floats(B, H * W)
    if ws is None or ws.numel() < need:
        ws = torch.empty((need,), dtype=torch.float32, device=logits.device)
    out = torch.empty((8,), dtype=torch.float32, device=logits.device)
    _lib.call('cdnet_mask_loss', _lib.ptr(logits), _lib.ptr(label), None if weight is None else _lib.ptr(weight), B, H, W, int(terms),
              _lib.ptr(ws), ws.numel(), _lib.ptr(out), None, _lib.stream_ptr())
    return out


def _variance_value(logits, label):
    """loss_var of the logits (cdnet_variance_loss, value only)"""
    from . import _lib
    B, K, H, W = logits.shape
    need = _lib.load().cdnet_variance_loss_workspace_bytes(B, K, H, W)
    ws = torch.empty(((need + 3) // 4,), dtype=torch.float32, device=logits.device)
    out = torch.empty((1,), dtype=torch.float32, device=logits.device)
    _lib.call('cdnet_variance_loss', _lib.ptr(logits), _lib.ptr(label), 1, B, K, H, W, 1.0, _lib.ptr(ws), ws.numel() * 4, _lib.ptr(out), None,
              None, None, None, _lib.stream_ptr())
    return float(out.item())


def validate(val_loader, model, criterion, epoch, opt, logger, labeled_df_list=None, get_process_worktime=1, get_process_detail=1,
             all_img_test=1, accuracy_tensor=0):
    """-> results.avg: [loss, pixel_accu, pixel_iou, pixel_recall, pixel_precision, pixel_F1] (:457, :480).  Eval-mode forward of the whole
    image (all_img_test == 1) or through `utils.split_forward` with opt.train['input_size'] / opt.train['val_overlap'] (:374-378); the
    loss is the UNWEIGHTED cross-entropy (:387-389) with the alpha and dice switches of `train` and no boundary term (the reference's
    validate has none): one cdnet_mask_loss call without gradient per batch."""
    dice, _, alpha = _check_options(opt)
    terms = utils.loss_terms(dice, 0, alpha)
    results = utils.AverageMeter(6)
    model.eval()
    dev = next(model.parameters()).device
    for i, sample in enumerate(val_loader):
        x, label, _ = _unpack(sample, dev)
        with torch.no_grad():
            if all_img_test == 1:
                out = model(x)
                out = out[0] if isinstance(out, (tuple, list)) else out
            else:
                out = torch.cat([utils.split_forward(model, x[b:b + 1], opt.train['input_size'], opt.train['val_overlap'], opt)
                                 for b in range(x.shape[0])], 0)
        out = out.float().contiguous()
        r = mask_loss_values(out, label, None, terms).cpu().numpy().astype(np.float64)
        loss = r[0]
        if alpha in (1, 2) and dice != 2:                  # :391-406; dice = 2 replaces the whole loss (:421-424)
            loss = loss + float(alpha) * _variance_value(out, label)
        results.update([loss, r[3], r[4], r[5], r[6], r[7]])
    if logger is not None:
        logger.info('\t=> Val Avg:   \tLoss {r[0]:.4f} \tPixel_Acc {r[1]:.4f}\tPixel_IoU {r[2]:.4f}\tpixel_Recall {r[3]:.4f}'
                    '\tpixel_Precision {r[4]:.4f}\tpixel_F1 {r[5]:.4f}'.format(r=results.avg))
    return results.avg
