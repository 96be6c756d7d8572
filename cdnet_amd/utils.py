"""Model factory, sliding-window forward and training helpers with the reference's names (utils.py).

  chooseModel(opt)                                     utils.py:816-886
  split_forward_dam(model, input, size, overlap, opt)  utils.py:658-726
  get_optimizer(args, model)                           utils.py:907-962   (returns the fused device optimiser and the scheduler)
  AverageMeter                                         utils.py:755-774
  adjust_learning_rate                                 utils.py:965-977
"""

import os

import numpy as np
import torch

from . import _lib


def chooseModel(opt):
    name = opt.model['modelName']
    # the reference hard-codes pretrained=True (an ImageNet download, utils.py:822-875); here the training entry passes --pretrained-path FILE
    # or, with --pretrained 1, lets get_backbone look for the file under ./pretrained_models (nothing is fetched).  The test entries load
    # a checkpoint over the model anyway: no search there, and nothing to freeze
    train = getattr(opt, 'isTrain', False)                 # (a bare options object, as the tools build: the test entries' behaviour)
    pretrained = (opt.model.get('pretrained_path') or bool(opt.model.get('pretrained', 0))) if train else False
    freeze = bool(opt.model.get('encoder_freeze', 0)) if train else False
    in_c = opt.model.get('in_c', 3)                  # 1: a grey-scale dataset (--dataset BBBC039V1); the Unet family then runs child0

    def stem(model):
        model.set_input_channels(in_c)
        return model
    if name == 'UNet':
        from .models.unet import UNet
        return UNet(num_classes=opt.model['out_c'], in_channels=opt.model['in_c'])
    if name == 'UNet2RevA1_vgg16':
        from .models.dam.model_unet_rev1 import Unet
        return stem(Unet(backbone_name='vgg16_bn', pretrained=pretrained, encoder_freeze=freeze, classes=opt.model['out_c']))
    if name == 'UNet_vgg16':                         # utils.py:822-824 (the ResNet backbones of :825-830 are not built)
        from .models.model_unet import Unet
        return stem(Unet(backbone_name='vgg16_bn', pretrained=pretrained, encoder_freeze=freeze, classes=opt.model['out_c']))
    if name in ('model_unet_MandD', 'model_unet_MandD4', 'model_unet_MandD16', 'model_unet_MandDandP'):      # utils.py:857-874
        import importlib
        mod = importlib.import_module('.models.dam.' + name, __package__)
        return stem(mod.Unet(backbone_name='vgg16_bn', pretrained=pretrained, encoder_freeze=freeze, classes=opt.model['out_c']))
    if name == 'HRNet18_rev1':                       # utils.py:880-882
        if in_c != 3:
            raise ValueError('HRNet18_rev1 has a fixed three-channel stem (in the reference too): in_c = {} is not served'.format(in_c))
        from .models.dam.seg_hrnet_rev1 import HighResolutionNet
        return HighResolutionNet(opt)
    if name == 'FullNet':                            # utils.py:833-838 (whose `dilations` entry options.py leaves commented out: the class default)
        from .models.FullNet import FullNet
        m = opt.model
        return FullNet(m['in_c'], m['out_c'], n_layers=m['n_layers'], growth_rate=m['growth_rate'], drop_rate=m['drop_rate'],
                       dilations=m.get('dilations', [1, 2, 4, 8, 16, 4, 1]), is_hybrid=m['is_hybrid'], compress_ratio=m['compress_ratio'],
                       layer_type=m['layer_type'])
    raise NotImplementedError('model {} is outside the CDNet hot path (SURVEY.md section 8: UNet, UNet_vgg16, UNet2RevA1_vgg16, model_unet_MandD*, HRNet18_rev1, FullNet)'.format(name))


def window_grid(h0, w0, size, overlap):
    """tile geometry of split_forward_dam (utils.py:664-683): padded extent, tile size, counts"""
    stride = size - overlap
    h = h0 + (stride - (h0 - size) % stride if h0 - size > 0 else 0)
    w = w0 + (stride - (w0 - size) % stride if w0 - size > 0 else 0)
    ny, nx = len(range(0, h - overlap, stride)), len(range(0, w - overlap, stride))
    return stride, min(size, h), min(size, w), ny, nx


def split_forward_views(model, image, size, overlap, xforms=(0,), direction_classes=9, max_batch=128, out=None):
    """Sliding-window forward of one image [3,H,W] (cuda float32; [1,H,W] for a one-channel model) for several TTA views at once.
    Returns a list (one entry per view) of the stitched logits of every output `model.forward_packed` returns: (mask [3,hv,wv], point [1,hv,wv],
    direction [9,hv,wv]) for the DAM networks, (mask [K,hv,wv], direction) for the model_unet_MandD* heads, (mask [K,hv,wv],) for UNet.
    `out` = one buffer per output, e.g. (mask f32 [V,3,H*W], point f32 [V,1,H*W], direction f32 [V,K,H*W]): the views are stitched straight
    into these buffers (a rotated view as [K][W][H]: the same element count) - pipeline.infer_image's one get_probmaps launch over all views
    reads them in place; pipeline.infer_image_mask passes the mask buffer alone and only the first output is stitched."""
    assert image.dim() == 3 and image.is_cuda and image.dtype == torch.float32
    Cc, H0, W0 = image.shape
    image = image.contiguous()
    from . import runtime
    f32 = runtime.PRECISION == 'fp32'
    geo = []
    for xf in xforms:
        hv, wv = (W0, H0) if xf & 4 else (H0, W0)
        stride, th, tw, ny, nx = window_grid(hv, wv, size, overlap)
        geo.append((hv, wv, stride, th, tw, ny, nx))

    def pack(i, dst):
        hv, wv, stride, th, tw, ny, nx = geo[i]
        _lib.call(_lib.entry('cdnet_window_pack', f32), _lib.ptr(image), Cc, H0, W0, int(xforms[i]), th, tw, stride, ny, nx,
                  _lib.ptr(dst), _lib.stream_ptr())

    def stitch(i, logits, off):
        hv, wv, stride, th, tw, ny, nx = geo[i]
        n = ny * nx
        st = []
        for j_, t_ in enumerate(logits):
            if out is not None and j_ >= len(out):
                break                                      # (outputs the caller gave no buffer for are not stitched)
            K = t_.shape[1]
            o = torch.empty((K, hv, wv), dtype=torch.float32, device=image.device) if out is None else out[j_][i].view(K, hv, wv)
            src = t_[off:off + n]                          # (a batch slice of a contiguous tensor is contiguous)
            _lib.call('cdnet_window_stitch', _lib.ptr(src), K, th, tw, stride, overlap, ny, nx, hv, wv, _lib.ptr(o), _lib.stream_ptr())
            st.append(o)
        return tuple(st)

    # windows of equal shape go through the network together, in batches of WHOLE views whenever a view's windows fit one batch: the
    # window tensors are then packed straight into the batch and stitched straight out of the network's outputs (the first version
    # concatenated all windows, cut 64-window batches across views and concatenated the outputs again: 1.1 GB of copies per 1000 x 1000
    # image with 8 views, and a last batch of 8 windows)
    outs = [None] * len(xforms)
    by_shape = {}
    for i, g_ in enumerate(geo):
        by_shape.setdefault((g_[3], g_[4], g_[5] * g_[6]), []).append(i)
    # (128: two batches of four views for a 1000 x 1000 image.  All eight views in one batch is another 3 % in steady state, but its multi-GB
    #  tensors make the caching allocator's behaviour - and the time - depend on what the process ran before: 24 to 65 ms per image)
    for (th, tw, n), idxs in by_shape.items():
        max_batch = max(1, min(max_batch, (1 << 24) // (th * tw)))      # at most 256 windows of 256 x 256 (64 of 512 x 512) per network batch
        if n <= max_batch:
            per = max(1, max_batch // n)
            per = -(-len(idxs) // -(-len(idxs) // per))    # equal-sized batches (8 views x 25 windows: 4 x 50, not 2 x 64 + ...)
            for g0 in range(0, len(idxs), per):
                grp = idxs[g0:g0 + per]
                tiles = torch.empty((len(grp) * n, th, tw, 16), dtype=runtime.act_dtype(), device=image.device)
                for k, i in enumerate(grp):
                    pack(i, tiles[k * n:(k + 1) * n])
                logits = model.forward_packed(tiles)
                for k, i in enumerate(grp):
                    outs[i] = stitch(i, logits, k * n)
            continue
        # a view with more windows than one batch holds: batches cut across the view, outputs gathered before the stitch
        for i in idxs:
            tiles = torch.empty((n, th, tw, 16), dtype=runtime.act_dtype(), device=image.device)
            pack(i, tiles)
            res = [model.forward_packed(tiles[s_:s_ + max_batch]) for s_ in range(0, n, max_batch)]
            logits = [torch.cat([r[k] for r in res], 0) for k in range(len(res[0]))]
            outs[i] = stitch(i, logits, 0)
    return outs


def split_forward(model, input, size, overlap, opt=None):
    """split the input image for forward process (reference signature, utils.py:603-654): the sliding-window forward of a network with ONE
    mask output (UNet; output[0] of the model_unet_MandD* heads).  input [1,C,H,W]; returns output [1,out_c,H,W] on the GPU."""
    assert input.shape[0] == 1, 'the reference calls this with one image at a time'
    with torch.no_grad():
        outs, = split_forward_views(model, input[0].cuda().float(), size, overlap, (0,))
    return outs[0][None]


def split_forward_dam(model, input, size, overlap, opt=None):
    """split the input image for forward process (reference signature).  input [1,C,H,W]; returns
    (output [1,out_c,H,W], output_point [1,1,H,W], output_direction [1,classes,H,W]) on the GPU."""
    assert input.shape[0] == 1, 'the reference calls this with one image at a time'
    with torch.no_grad():
        (m, p, d), = split_forward_views(model, input[0].cuda().float(), size, overlap, (0,))
    return m[None], p[None], d[None]


class AverageMeter(object):
    """ Computes and stores the average and current value (utils.py:755-774) """

    def __init__(self, shape=1):
        self.shape = shape
        self.reset()

    def reset(self):
        self.val = np.zeros(self.shape)
        self.avg = np.zeros(self.shape)
        self.sum = np.zeros(self.shape)
        self.count = 0

    def update(self, val, n=1):
        val = np.array(val)
        assert val.shape == self.val.shape
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


def trainer_class(model):
    """the Trainer that serves `model`: the plain UNet's (one mask output), the ablation heads' (plain classifiers instead of the gated
    head, model_unet_MandD / model_unet_MandDandP), FullNet's (the UNet's loss around its own tape), the backbone U-Net's (the UNet's loss
    around the rev1 tape, models/model_unet.py), the DAM networks'"""
    from .models.unet import UNet
    from .models.FullNet import FullNet
    from .models.model_unet import Unet as BackboneUnet
    from .trainer import Trainer, AblationTrainer, BackboneUNetTrainer, FullNetTrainer, UNetTrainer
    if isinstance(model, UNet):
        return UNetTrainer
    if isinstance(model, BackboneUnet):
        return BackboneUNetTrainer
    if isinstance(model, FullNet):
        return FullNetTrainer
    return AblationTrainer if getattr(model, 'VARIANT', 'rev1') != 'rev1' else Trainer


LOSS_WMAP, LOSS_CE, LOSS_DICE = 1, 2, 4              # CDNET_LOSS_* (include/cdnet_hip.h)


def loss_terms(dice=1, weight_map=1, alpha=0):
    """the `terms` word of cdnet_mask_loss / cdnet_dam_loss_terms for the option triple (--dice, --weight-map, --alpha):
      weight_map 1 -> WMAP: the CE map x weight / 20 (train_util.py:134-135);
      dice 1 / 2   -> DICE: + MulticlassDiceLoss (:183-186) / the dice term alone (:187-190), which takes CE out of the total;
      alpha 2      -> the variance term instead of the cross-entropy (:148-155): CE out of the total.
    Any other value raises ValueError: the reference ignores it silently, except alpha = 3 (its SSIM experiment, not built)."""
    if dice not in (0, 1, 2):
        raise ValueError('dice = %r: 0 (no dice term), 1 (+ MulticlassDiceLoss) or 2 (the dice term alone)' % (dice,))
    if weight_map not in (0, 1):
        raise ValueError('weight_map = %r: 0 (plain cross-entropy) or 1 (cross-entropy x weight map / 20)' % (weight_map,))
    if alpha not in (0, 1, 2):
        raise ValueError('alpha = %r: 0 (no variance term), 1 (loss_CE + loss_var) or 2 (2 * loss_var instead of loss_CE)%s'
                         % (alpha, '; alpha = 3 (SSIM) is not built' if alpha == 3 else ''))
    terms = LOSS_WMAP if weight_map == 1 else 0
    if alpha != 2 and dice != 2:
        terms |= LOSS_CE
    if dice != 0:
        terms |= LOSS_DICE
    return terms


def get_optimizer(args, model, world_size=1):
    """utils.py:907-962: returns (Trainer, scheduler).  cdnet_amd.trainer.Trainer steps the fused device optimiser (cdnet_amd.optim.stepper) - 'adam'
    (lr, betas=(0.9, 0.99), weight_decay; cdnet_adam_step) or one of 'sgd' (momentum = args.momentum), 'radam', 'radam4s', 'adamw',
    'ranger' (cdnet_sgd_step / cdnet_moment_step), matched case-insensitively.  An unknown name raises ValueError (the reference's
    `raise '<str>'` is a TypeError by accident).  The scheduler is an optim.LRSchedule for the four torch schedulers of :941-957 and None
    otherwise (the epoch loop then calls adjust_learning_rate, train.py:404-405)."""
    from . import optim
    boundary = int(getattr(args, 'model', {}).get('boundary_loss', 0))           # (an options object without a model dict: the term is off)
    if boundary not in (0, 1, 2, 3):
        # the reference adds nothing for any other value and says nothing (train_util_dam.py:207-208)
        raise ValueError('boundary_loss = %r: 0 (off), 1 (BoundaryLoss), 2 (FocalLoss2d) or 3 (RobustFocalLoss2d)' % (boundary,))
    md = getattr(args, 'model', {})
    dice, weight_map, alpha = md.get('dice', 1), md.get('add_weightMap', 1), args.train.get('alpha', 0.0)
    loss_terms(dice, weight_map, alpha)                                          # ValueError on anything but 0|1|2, 0|1, 0|1|2
    dice, weight_map = int(dice), int(weight_map)
    name = str(args.train['optimizer']).lower()
    if name not in optim.OPTIMIZERS:
        raise ValueError('Optimizer {} not available'.format(args.train['optimizer']))
    trainer = trainer_class(model)(model, lr=args.train['lr'], weight_decay=args.train['weight_decay'], world_size=world_size,
                                   optimizer=name, momentum=getattr(args, 'momentum', 0.95))
    if hasattr(trainer, 'seed'):                                  # FullNetTrainer: the dropout masks follow --seed and the rank
        trainer.seed = int(args.train.get('seed', 0)) + int(os.environ.get('RANK', '0'))
    trainer.alpha = float(args.train.get('alpha', 0.0))           # 1: + the instance variance term (train_util_dam.py:174-180)
    trainer.boundary = boundary                                   # 1 / 2 / 3: + the boundary / focal term (train_util_dam.py:195-205)
    trainer.dice, trainer.weight_map = dice, weight_map           # --dice 0|1|2, --weight-map 0|1 (train_util.py:134-136, 183-190)
    scheduler = None
    if args.train['scheduler'] in optim.SCHEDULERS:
        scheduler = optim.LRSchedule(args.train['scheduler'], args.train['lr'], step=args.train['step'], lr_decay=args.train['lr_decay'])
    return trainer, scheduler


def adjust_learning_rate(args, trainer, epoch):
    """utils.py:965-977: scheduler 'None' keeps the learning rate constant; any other name (the four of get_optimizer have a scheduler
    object and never come here) sets lr * 0.9 ** (epoch // step)"""
    if args.train['scheduler'] != 'None':
        trainer.lr = args.train['lr'] * (0.9 ** (epoch // args.train['step']))
    return trainer.lr


class EarlyStopping:
    """Early stops the training if the monitored value does not improve after `patience` epochs - and, as in the reference, never
    before epoch 100 (utils.py:992-1034)."""

    def __init__(self, patience=7, verbose=False, delta=0):
        self.patience, self.verbose, self.delta = patience, verbose, delta
        self.counter, self.best_score, self.early_stop = 0, None, False
        self.val_loss_min = np.inf

    def __call__(self, val_loss, epoch):
        score = -val_loss
        if self.best_score is None:
            self.best_score = score
            self.val_loss_min = val_loss
        elif score < self.best_score + self.delta:
            self.counter += 1
            print('===================== EarlyStopping counter: {} out of {} ====================='.format(self.counter, self.patience))
            if self.counter >= self.patience and epoch >= 100:
                self.early_stop = True
        else:
            self.best_score = score
            self.val_loss_min = val_loss
            self.counter = 0


def measure_label(a):
    """skimage.measure.label semantics (:248-249): 8-connected regions of EQUAL value, background 0, ids 1..K in raster order of
    each region's first pixel.  Instance maps from this package already are such regions (one lookup table); a binary image
    (validate's 0/255 target, train_util_dam.py:600-602) or a value that occurs in several separate regions is split here."""
    from scipy import ndimage as ndi
    a = np.ascontiguousarray(a).astype(np.int64)
    comp, _ = ndi.label(a != 0, structure=np.ones((3, 3), dtype=int))
    key = comp * (int(a.max()) + 1 if a.size else 1) + a              # (foreground component, value)
    key[a == 0] = 0
    vals, inv = np.unique(key.ravel(), return_inverse=True)
    lab = inv.reshape(a.shape).astype(np.int64)                         # 0 = background (key 0 sorts first), 1..K otherwise
    if vals[0] != 0:
        lab += 1
    # two regions of one value inside one foreground component touch only through other values: split them
    nxt = int(lab.max())
    for k, sl in enumerate(ndi.find_objects(lab), start=1):
        if sl is None:
            continue
        sub, n = ndi.label(lab[sl] == k, structure=np.ones((3, 3), dtype=int))
        for j in range(2, n + 1):
            nxt += 1
            lab[sl][sub == j] = nxt
    ids, first = np.unique(lab.ravel(), return_index=True)
    keep = ids != 0
    ids, first = ids[keep], first[keep]
    lut = np.zeros(nxt + 1, np.int32)
    lut[ids[np.argsort(first, kind='stable')]] = np.arange(1, len(ids) + 1, dtype=np.int32)
    return lut[lab].astype(np.int32)


def object_hausdorff_host(true, pred, pairs):
    """float64 [M, 2]: (h(P -> T), h(T -> P)) of every pair (true id, pred id) with scipy's directed_hausdorff on np.argwhere of the two
    objects - the calls the reference makes per matched object (utils.py:6, :303), O(pixels) each.  The host path: what
    stats_utils.object_hausdorff is compared with, and what it falls back to for pairs beyond its work bound."""
    from scipy.spatial.distance import directed_hausdorff
    out = np.zeros((len(pairs), 2), np.float64)
    for m, (ti, pi) in enumerate(np.asarray(pairs).reshape(-1, 2)):
        seg_ind, gt_ind = np.argwhere(pred == pi), np.argwhere(true == ti)
        out[m] = directed_hausdorff(seg_ind, gt_ind)[0], directed_hausdorff(gt_ind, seg_ind)[0]
    return out


def nuclei_accuracy_object_level_host(pred, gt):
    """nuclei_accuracy_object_level with the Hausdorff distances from object_hausdorff_host: one scipy call pair per matched object"""
    return nuclei_accuracy_object_level(pred, gt, hausdorff=lambda g, p, pairs: object_hausdorff_host(g, p, pairs).max(1))


def nuclei_accuracy_object_level(pred, gt, hausdorff=None):
    """(recall, precision, F1, dice, iou, haus, AJI) of utils.nuclei_accuracy_object_level (utils.py:245-330): ground-truth objects in
    id order, each greedily paired with the not-yet-used predicted object of largest IoU (first maximum in id order), used objects
    removed (:312).  The pixel pass (areas + sparse pairwise intersections) runs on the device (`stats_utils.pair_table`); the
    per-pair arithmetic is the reference's float arithmetic; the Hausdorff distances of all matched pairs come from one
    `stats_utils.object_hausdorff` call (exact integer squared distances on the device, sqrt in float64: the bits of scipy's
    directed_hausdorff on both sides, the call the reference makes, :6, :303) and are summed in the reference's order.
    `hausdorff(gt_labels, pred_labels, pairs [M, 2] of (gt id, pred id)) -> float64 [M]` replaces that call (see
    nuclei_accuracy_object_level_host).
    pred / gt: integer label or binary images; both are re-labelled like the reference does with skimage.measure.label (8-connected
    regions of equal value, raster-order ids)."""
    from . import stats_utils

    p, g = measure_label(pred), measure_label(gt)
    ag, ap, pairs = stats_utils.pair_table(g, p)
    Ng, Ns = int((ag[1:] > 0).sum()), int((ap[1:] > 0).sum())
    by_gt = {}
    for ti, pi, inter in pairs:
        by_gt.setdefault(int(ti), []).append((int(pi), float(inter)))
    used, matched = set(), []
    TP = FN = 0.0
    dice = iou = haus = C = U = count = 0.0
    for i in range(1, Ng + 1):
        cands = [(k, it) for k, it in sorted(by_gt.get(i, [])) if k not in used]
        if not cands:
            FN += 1
            U += float(ag[i])
            continue
        max_iou, best, overlap_area = 0.0, None, 0.0
        for k, it in cands:
            tmp_iou = it / (float(ap[k]) + float(ag[i]) - it)
            if tmp_iou > max_iou:
                max_iou, best, overlap_area = tmp_iou, k, it
        TP += 1
        count += 1
        a_p, a_g = float(ap[best]), float(ag[i])
        dice += 2 * overlap_area / (a_p + a_g)
        iou += overlap_area / (a_p + a_g - overlap_area)
        matched.append((i, best))
        C += overlap_area
        U += a_p + a_g - overlap_area
        used.add(best)
    if matched:
        if hausdorff is None:                                   # (the device packs a coordinate into 15 bits)
            hausdorff = stats_utils.object_hausdorff if max(g.shape) <= 32767 else (lambda a, b, m: object_hausdorff_host(a, b, m).max(1))
        for h in hausdorff(g, p, np.array(matched, dtype=np.int64)):
            haus += float(h)
    FP = Ns - TP
    recall = TP / (TP + FN + 1e-10)
    precision = TP / (TP + FP + 1e-10)
    F1 = 2 * TP / (2 * TP + FP + FN + 1e-10)
    if count == 0:
        count = 1
    dice, iou, haus = dice / count, iou / count, haus / count
    U += float(sum(int(ap[k]) for k in range(1, len(ap)) if ap[k] > 0 and k not in used))
    AJI = float(C) / U if U > 0 else float('nan')
    return recall, precision, F1, dice, iou, haus, AJI
