"""Checkpoint interchange with the reference.

The reference saves {'epoch', 'state_dict', 'best_iou', 'best_loss', 'optimizer'} with `model` wrapped in nn.DataParallel
(every key prefixed 'module.', train.py:183-185, 421-427), names the files checkpoint.pth.tar / checkpoint_<epoch>.pth.tar /
checkpoint_best.pth.tar (save_checkpoint, train.py:461-480) and loads them with load_state_dict (train.py:297-302,
test_dam.py:163-165).  The files written here load in the reference and vice versa: parameter names and shapes are the
reference's, and the optimiser entry is the state_dict of the reference's optimiser object - torch.optim.Adam by default, torch.optim.SGD,
RAdam / RAdam_4step / AdamW or Ranger for the other --optimizer values (cdnet_amd.optim.state_dict through Trainer.state_dict)."""
import os
import shutil

import torch

PREFIX = 'module.'


def model_state(model):
    """state_dict with the DataParallel prefix, on the CPU, contiguous (parameters may be views of flat / padded storage)"""
    return {PREFIX + k: v.detach().cpu().contiguous().clone() for k, v in model.state_dict().items()}


def make_state(model, trainer, epoch, best_iou=0.0, best_loss=float('inf')):
    """the dict train.py:421-427 hands to save_checkpoint"""
    trainer.write_bn_counters()
    return {'epoch': epoch + 1, 'state_dict': model_state(model), 'best_iou': best_iou, 'best_loss': best_loss,
            'optimizer': trainer.state_dict()}


def save_checkpoint(state, epoch, is_best, save_dir, branch_value, cp_flag):
    """train.py:461-480 (same arguments, same file names)"""
    cp_dir = '{:s}/checkpoints'.format(save_dir)
    os.makedirs(cp_dir, exist_ok=True)
    filename = '{:s}/checkpoint.pth.tar'.format(cp_dir)
    torch.save(state, filename)
    branch = '' if branch_value == 'Main' else branch_value
    if cp_flag:
        shutil.copyfile(filename, '{:s}/checkpoint{:s}_{:d}.pth.tar'.format(cp_dir, branch, epoch + 1))
    if is_best:
        shutil.copyfile(filename, '{:s}/checkpoint{:s}_best.pth.tar'.format(cp_dir, branch))
    return filename


# ----------------------------------------------------------------------------------------------------------
# ImageNet encoder weights: a torchvision vgg16_bn file into the `backbone` of a Unet-family model (model_unet_rev1.py:22-43, where the
# reference calls models.vgg16_bn(pretrained=True).features).  Nothing is fetched: the file is on disk or it is not used.
PRETRAINED_SEARCH = ('./pretrained_models/{name}/hub/checkpoints/{name}-*.pth', './pretrained_models/{name}/checkpoints/{name}-*.pth')


def find_pretrained(name='vgg16_bn'):
    """(first file under the reference's TORCH_HOME layout below the working directory or None, the patterns searched)"""
    import glob
    patterns = [p.format(name=name) for p in PRETRAINED_SEARCH]
    for pat in patterns:
        hits = sorted(glob.glob(pat))
        if hits:
            return hits[0], patterns
    return None, patterns


def _backbone_key(k):
    """(name inside `backbone` or None, dropped unread?) of one key of the source"""
    if k.startswith('classifier.'):
        return None, True
    for prefix in ('features.', 'backbone.'):
        if k.startswith(prefix):
            return k[len(prefix):], False
    return (k, False) if k.split('.', 1)[0].isdigit() else (None, False)


def load_encoder_state(backbone, source, strict=True):
    """load_backbone_weights on the bare encoder module (what get_backbone holds before the model exists)"""
    if not isinstance(source, dict):
        path = os.fspath(source)
        if not os.path.isfile(path):
            raise FileNotFoundError("no encoder weights file at '{}'".format(path))
        source = torch.load(path, map_location='cpu', weights_only=True)
    want = backbone.state_dict()
    found, dropped, extra, origin = {}, [], [], {}
    for k, v in source.items():
        name, drop = _backbone_key(k)
        if drop:
            dropped.append(k)
        elif name is None or name not in want or name in found:
            extra.append(k)
        else:
            found[name], origin[name] = v, k
    # a file written before BatchNorm counted its batches has no num_batches_tracked at all: nn.BatchNorm2d reads such a file as zero
    # counters (its _load_from_state_dict, version < 2), and so does this loader; one counter missing among others is a missing key
    old_bn = not any(k.endswith('num_batches_tracked') for k in found)
    defaulted = [n for n in want if n.endswith('num_batches_tracked') and n not in found] if old_bn else []
    missing = [n for n in want if n not in found and n not in defaulted]
    misshaped = [n for n in found if not torch.is_tensor(found[n]) or tuple(found[n].shape) != tuple(want[n].shape)]
    if strict:
        if missing:
            raise ValueError('encoder weights: missing key backbone.{} ({} more missing)'.format(missing[0], len(missing) - 1))
        if extra:
            raise ValueError("encoder weights: unexpected key '{}' ({} more; only classifier.* is dropped)".format(extra[0], len(extra) - 1))
        if misshaped:
            n = misshaped[0]
            raise ValueError("encoder weights: key '{}' has shape {} where backbone.{} has {}".format(
                origin[n], tuple(getattr(found[n], 'shape', ())), n, tuple(want[n].shape)))
    # validated: copy (the destinations are the module's own tensors - views of the trainer's flat buffer once a trainer exists)
    loaded = []
    with torch.no_grad():
        for n, dst in want.items():
            if n in found and n not in misshaped:
                dst.copy_(found[n].to(dst.dtype))
                loaded.append('backbone.' + n)
            elif n in defaulted:
                dst.zero_()
    from . import runtime
    runtime.WEIGHTS_EPOCH[0] += 1          # every packed weight copy and BatchNorm fold is stale (what Trainer.refresh_parameters does)
    return {'loaded': loaded, 'dropped': dropped + extra, 'missing': ['backbone.' + n for n in missing + misshaped],
            'zeroed': ['backbone.' + n for n in defaulted]}


def load_backbone_weights(model, source, strict=True):
    """Load a torchvision VGG16-BN file into `model.backbone` (any model of the Unet family).  `source`: a path (read with weights_only) or
    a state dict, in one of three layouts: the whole torchvision model (`features.N.*`; `classifier.*` is dropped unread), the bare
    `.features` dict (`N.*`), or this project's `backbone.N.*`.  Every weight, bias, running_mean, running_var and num_batches_tracked of
    the backbone must be there with the model's shape; with `strict` a missing, unknown or mis-shaped entry raises ValueError naming the key
    and the model is left untouched (everything is validated before the first copy).  Nothing outside `backbone.` is written.
    Works before a trainer exists, after one exists (the parameters are then views of its flat buffer: the copy lands there) and on a
    model that has already run: the weight epoch is bumped, so packs and BatchNorm folds are rebuilt on next use.
    Returns {'loaded': model keys written, 'dropped': source keys not used, 'missing': model keys left as they were (strict=False only),
    'zeroed': counters a pre-num_batches_tracked file does not have}."""
    return load_encoder_state(model.backbone, source, strict=strict)


def _numpy_safe_globals():
    """what unpickling a numpy scalar needs: numpy._core.multiarray.scalar, numpy.dtype and the dtype classes of the scalars
    the reference writes (float / int AverageMeter values)"""
    import numpy as np
    try:
        from numpy._core.multiarray import scalar
    except ImportError:                                  # numpy < 2
        from numpy.core.multiarray import scalar
    return [scalar, np.dtype] + [type(np.dtype(t)) for t in ('float64', 'float32', 'int64', 'int32', 'bool')]


def load_checkpoint(path, model, trainer=None, strict=True, trusted_pickle=False):
    """Load a checkpoint written by the reference or by save_checkpoint.  Returns the checkpoint dict (epoch, best_iou, ...).
    Keys with or without the DataParallel prefix are accepted (test_dam.py:163-165 loads with strict=False).
    The interchange format holds only tensors, numbers, strings and containers of them, so the file is read with
    `weights_only=True` - with numpy's scalar / dtype reconstructors allow-listed, because the reference stores
    `best_iou` / `best_loss` as numpy.float64 (AverageMeter.avg, train.py:390-427), which a bare `weights_only=True`
    refuses; `trusted_pickle=True` (CDNET_TRUSTED_PICKLE=1, `--trusted-pickle`) opts into full unpickling for legacy files
    from a trusted source."""
    if trusted_pickle or os.environ.get('CDNET_TRUSTED_PICKLE', '0') == '1':
        ck = torch.load(path, map_location='cpu', weights_only=False)
    else:
        with torch.serialization.safe_globals(_numpy_safe_globals()):
            ck = torch.load(path, map_location='cpu', weights_only=True)
    for k in ('best_iou', 'best_loss'):
        if k in ck and not isinstance(ck[k], torch.Tensor):
            ck[k] = float(ck[k])                         # numpy.float64 -> float
    sd = ck['state_dict'] if 'state_dict' in ck else ck
    sd = {(k[len(PREFIX):] if k.startswith(PREFIX) else k): v for k, v in sd.items()}
    model.load_state_dict(sd, strict=strict)
    if trainer is not None:
        # the fused optimiser keeps its own fp32 master copy of the parameters: refresh it from the module
        trainer.refresh_parameters()
        nbt = [v for k, v in sd.items() if k.endswith('num_batches_tracked')]
        trainer._bn_base, trainer._forwards = (int(max(int(v) for v in nbt)) if nbt else 0), 0
        if ck.get('optimizer') is not None:
            trainer.load_state_dict(ck['optimizer'])
    return ck
