"""Inference pipelines on the device: model forward -> get_probmaps epilogue -> direction-difference map ->
boost/argmax -> connected-component chain, without leaving the GPU (only the final int32 label maps do).

`infer_tiles`   : a batch of independent tiles, one view each (the benchmark unit "256x256 tile incl. post-proc")
`infer_image`   : the reference's per-image procedure of test_dam.py:297-563: 8 dihedral TTA views, whole-image
                  forward (all_img_test == 1) or sliding windows (utils.split_forward_dam), per-view DDM, mean,
                  point-guided boost, CC chain.
`infer_tiles_mask` / `infer_image_mask`: the same for networks with one mask output (UNet, output[0] of the model_unet_MandD* heads) -
                  test.py:216-296: mean of the views' softmax, arg-max, CC chain (or the watershed variant with postproc 1).
"""
import contextlib

import numpy as np
import torch

from . import postproc


@torch.no_grad()
def infer_tiles(model, x, classes=9, min_area=20, radius=2, want_stages=False, post_stream=None, check=False, want_prob=False, fused=True):
    """x: float32 NCHW [B,3,H,W] on the GPU.  Returns dict(final int32 [B,H,W], counts, pred, dcm, minmax, ...; `prob` with want_prob / want_stages).
    `fused=False` takes the per-step chain (probmaps -> ddm_codes -> tta_boost_argmax -> cc_chain: ~17 launches) whatever the shape - the
    form every shape falls back to that the two-launch chain does not serve (W not a multiple of 64, more than 65536 pixels per tile).

    `post_stream` (a torch.cuda.Stream; cdnet_amd.streams.side_stream() picks one that does not share the compute stream's hardware
    queue): the post-processing chain is queued on that stream, ordered after this batch's forward, and
    the call returns at once - the small, latency-bound connected-component / direction kernels of batch i then run beside the
    convolutions of batch i + 1 queued on the caller's stream.  The returned tensors belong to `post_stream`: wait for `r['done']`
    (an event) - or synchronize - before reading them on another stream.

    The reference asserts PER IMAGE on a constant direction-difference map (0/0 -> NaN, test_dam.py:535) - `infer_image` keeps that assertion.
    A batch of independent tiles may legitimately hold a background-only tile, and a host-side assert costs a device-to-host
    synchronisation: here the test is opt-in.  `check=True` (serial form only) raises the reference's AssertionError for the batch;
    otherwise call `check_tiles(r)` when wanted - it reads the (min, max) codes the DDM kernel already leaves in `r['minmax']` (int32 [B, 2];
    no extra launch in the chain), after waiting for `r['done']` in the pipelined form."""
    assert not model.training
    mask, point, direction = model(x)
    B, _, H, W = mask.shape
    ctx = contextlib.nullcontext()
    if post_stream is not None:
        post_stream.wait_stream(torch.cuda.current_stream())
        for t in (mask, point, direction):
            t.record_stream(post_stream)                  # (allocated on the caller's stream, last read on the other one)
        ctx = torch.cuda.stream(post_stream)
    with ctx:
        if fused and postproc.tile_postproc_eligible(B, direction.shape[1], H, W):
            # two launches: probabilities / direction classes / DDM codes, then everything else of a tile in one workgroup (csrc/postproc_tile.hip);
            # the probability planes are written only when asked for (want_prob / want_stages)
            r = postproc.tile_postproc(mask, direction, point, min_area, radius, want_stages=want_stages, want_prob=want_prob)
        else:
            prob, dcm = postproc.probmaps(mask, direction)                        # test_dam.py:984, 1011-1013
            code, minmax = postproc.ddm_codes(dcm, classes)                       # generate_dd_map per tile
            r = postproc.tta_boost_argmax(prob.reshape(B, 1, 3 * H * W), point.reshape(B, 1, H * W),
                                          code.reshape(B, 1, H * W), minmax.reshape(B, 1, 2), [0], H, W,
                                          want_stages=want_stages)
            cc = postproc.cc_chain(r['pred'], 1, min_area, radius, want_stages=want_stages)
            r.update(cc)
            r.update(prob=prob, dcm=dcm, minmax=minmax, point=point)
        if post_stream is not None:
            r['done'] = torch.cuda.Event()
            r['done'].record(post_stream)
    if check:
        assert post_stream is None and not torch.cuda.is_current_stream_capturing(), 'check=True synchronises: serial form, outside a graph capture'
        check_tiles(r)
    return r


def check_tiles(r):
    """the reference's `assert(np.min(enhanced_boundary) >= 0)` (test_dam.py:535: NaN when a tile's direction-difference map is constant) for
    a result of infer_tiles; reads the device flag (synchronises with the stream that produced it)"""
    if 'done' in r:
        r['done'].synchronize()
    if 'ddm_constant' in r:                                     # (a precomputed flag tensor, bool [B])
        flags = r['ddm_constant'].cpu()
    else:
        mm = r['minmax'].reshape(-1, 2).cpu()
        flags = mm[:, 0] == mm[:, 1]
    bad = torch.nonzero(flags).flatten().tolist()
    assert not bad, ('tile(s) %s have a constant direction-difference map: 0/0 -> NaN; the reference asserts here (test_dam.py:535)' % bad)


@torch.no_grad()
def infer_image(model, image, opt=None, tta=True, all_img_test=1, patch_size=256, overlap=40, classes=9, min_area=20,
                radius=2, want_stages=False, defer=False, postproc=0, model_mode='Unet_rev1', restore=None):
    """The reference's per-image inference (test_dam.py:297-563) for one image tensor [3,H,W] float32 on the GPU
    (already ToTensor'd / normalised; [1,H,W] for a model set to one input channel, whose windows are packed with C = 1): the eight dihedral views (TTA) through the network - whole image
    (all_img_test == 1, options.py:35) or 256/40 sliding windows (utils.split_forward_dam) - softmax / gated direction
    argmax per view (get_probmaps), per-view direction-difference maps, their mean, the point-guided boundary boost, argmax,
    fill holes, remove small objects, label, dilate.  Returns dict(final int32 [H,W], count, pred, ...).
    `postproc=1` (opt.post['postproc'], --postproc 1; test_dam.py:558-563): after the boost and arg-max `final` is
    dilate_labels(postproc_other.process(pred == 1, model_mode, min_size=10), radius) with model_mode = opt.model['modelName'] - the raw
    prediction and postproc_other's default min_size 10, not min_area, because test_dam.py:559 passes none - and `counts` the number of
    distinct non-zero ids of `final`; `postproc_err` (device int32) is checked here unless `defer`; a deferring caller may
    read it with postproc.check_postproc_err (test_dam.main does not: the ids come from this package's own labelling and the flood's pass bound
    cannot be reached, so the flag cannot be raised there).  postproc=0: the chain above, unchanged.
    `defer=True`: nothing is read back - no host synchronisation; instead of `count` the device tensor `counts` stays in the result and the
    reference's constant-DDM assertion is left to the caller (postproc.check_views on `minmax`) - the form test_dam.main pipelines images with.
    `restore=(ori_h, ori_w)` (the 'scale' test transform: `image` was resized for the network, test_dam.py:551-553): holes are filled and small
    objects removed at the network's size, that mask is resized to (ori_h, ori_w) on the device (resize.resize_mask), then labelled and
    dilated (postproc.restore_chain): `final`, `counts` and `count` are at the original size, `pred` and `prob_mean` stay at the scaled
    size, where the reference saves them.  With postproc=1 a ValueError.  None: the path above, unchanged.
    With 'scale' in opt.transform['test'] and no `restore`, `image` is the transformed image at its ORIGINAL size - what test_dam.main and
    test_dam.process_image hand over - and the transform's Scale step runs here, on the device (scale_transformed).
    With opt.model['in_c'] == 1 (a grey-scale dataset) a THREE-plane `image` is taken to be what test_dam.main and test_dam.process_image
    hand over - the file read as RGB, / 255.0 and normalised per opt.transform['test'] - and is converted to Pillow's mode L here, on
    the device (grey_transformed: its bytes are recovered by rounding, so a three-plane tensor that is not such an image is quantised to
    bytes).  The entry module keeps its loader: cdnet_amd/test_dam.py falls under the repository's rule that a feature change leaves
    existing test_*.py files as they are.  A caller who loads the file itself hands over [1,H,W] (pipeline.host_input(..., in_c=1), as
    cdnet_amd.test does): one plane goes through untouched."""
    from . import postproc as postproc_mod, utils                         # (`postproc` is the reference's option name here)
    if opt is not None:
        tta, all_img_test = opt.test['tta'], opt.all_img_test
        patch_size, overlap = opt.test['patch_size'], opt.test['overlap']
        classes, min_area, radius = opt.direction_classes, opt.post['min_area'], opt.post['radius']
        postproc, model_mode = int(opt.post['postproc']), opt.model['modelName']
    if (restore is not None or _has_scale(opt)) and int(postproc) == 1:
        raise ValueError(postproc_mod.SCALE_POSTPROC1)
    image = grey_transformed(image, opt)                       # in_c = 1 and an image the entry read as RGB: Pillow's convert('L'), on the device
    if restore is None and _has_scale(opt):
        image, restore = scale_transformed(image, opt.transform['test'])
    assert not model.training and image.dim() == 3
    _, H, W = image.shape
    xforms = list(postproc_mod.TTA_XFORMS) if tta else [0]
    V = len(xforms)
    plane = H * W
    dev = image.device
    # every view's logits are stitched straight into one buffer per output (a rotated view as [K][W][H]: the same element count), get_probmaps'
    # epilogue is ONE launch over all views and writes the post-processing's inputs in place (round 5: eight launches and 24 device copies)
    mask_all = torch.empty((V, 3, plane), dtype=torch.float32, device=dev)
    dir_all = torch.empty((V, classes, plane), dtype=torch.float32, device=dev)
    probs = torch.empty((1, V, 3 * plane), dtype=torch.float32, device=dev)
    points = torch.empty((1, V, plane), dtype=torch.float32, device=dev)
    dcms = torch.empty((1, V, plane), dtype=torch.uint8, device=dev)
    bufs = (mask_all, points[0].view(V, 1, plane), dir_all)
    if all_img_test == 1:
        # whole-image forward: one window as large as the view
        utils.split_forward_views(model, image, max(H, W), 0, xforms, classes, out=bufs)
    else:
        utils.split_forward_views(model, image, patch_size, overlap, xforms, classes, out=bufs)
    postproc_mod.probmaps(mask_all.view(V, 3, 1, plane), dir_all.view(V, classes, 1, plane), prob_out=probs, dcm_out=dcms)
    r = postproc_mod.postprocess_views(probs, points, dcms, xforms=xforms, H=H, W=W, classes=classes, min_area=min_area,
                                   radius=radius, want_stages=want_stages, check=not defer, postproc=int(postproc), model_mode=model_mode,
                                   restore=restore)
    out = {k: (v[0] if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == 1 else v) for k, v in r.items()}
    if not defer:
        out['count'] = int(r['counts'][0])
    return out


def mask_channels(model):
    """K, the number of mask logits of a network with a mask output (UNet: final_conv; the Unet family: mask_conv)"""
    conv = getattr(model, 'mask_conv', None) or getattr(model, 'final_conv')
    return int(conv.out_channels)


def _mask_logits(out):
    """the mask output of a forward: UNet's tensor, output[0] of the model_unet_MandD* heads' (mask, direction) (test.py:629-630)"""
    if torch.is_tensor(out):
        return out
    if len(out) > 2:
        raise ValueError('a network with %d outputs (mask, point, direction) is evaluated by cdnet_amd.test_dam, not the mask-only path' % len(out))
    return out[0]


@torch.no_grad()
def infer_tiles_mask(model, x, min_area=20, radius=2, post_stream=None, want_stages=False, fused=True):
    """Mask-only counterpart of infer_tiles: x float32 NCHW [B,3,H,W] on the GPU through a network with one mask output, then softmax, class
    (arg-max; `>= 0.5` for one channel) and the CC chain - TWO launches (cdnet_tile_mask_postproc) when the shape allows (W a multiple of 64,
    at most 65536 pixels per tile), else `mask_views_argmax` (one view) + `cc_chain`; `fused=False` takes that per-step form for every shape.
    Returns dict(final int32 [B,H,W], counts int32 [B], pred u8 [B,H,W] [, prob, fill, small, label with want_stages]).
    `post_stream`: as for infer_tiles - the post-processing is queued on that stream after this batch's forward and the call returns at once;
    wait for `r['done']` before reading the results on another stream."""
    assert not model.training
    logits = _mask_logits(model(x))
    B, K, H, W = logits.shape
    ctx = contextlib.nullcontext()
    if post_stream is not None:
        post_stream.wait_stream(torch.cuda.current_stream())
        logits.record_stream(post_stream)
        ctx = torch.cuda.stream(post_stream)
    with ctx:
        if fused and postproc.tile_mask_postproc_eligible(B, K, H, W):
            r = postproc.tile_mask_postproc(logits, min_area, radius, want_stages=want_stages)
        else:
            m = postproc.mask_views_argmax(logits, [0], H, W, want_prob=want_stages)
            r = postproc.cc_chain(m['pred'], 1, min_area, radius, want_stages=want_stages)
            r['pred'] = m['pred']
            if want_stages:
                r['prob'] = m['prob_mean']
        if post_stream is not None:
            r['done'] = torch.cuda.Event()
            r['done'].record(post_stream)
    return r


@torch.no_grad()
def infer_image_mask(model, image, opt=None, tta=True, all_img_test=1, patch_size=256, overlap=40, min_area=20, radius=2, postproc=0,
                     model_mode='UNet', want_prob=False, defer=False, restore=None):
    """The reference's per-image procedure of test.py:213-296 for one image tensor [3,H,W] float32 on the GPU (already ToTensor'd /
    normalised; [1,H,W] for a one-channel network) and a network with one mask output: the eight dihedral views (TTA) - whole image (all_img_test == 1) or sliding windows
    (utils.split_forward, :627) - stitched into ONE buffer, then ONE launch for every view's softmax, the mean and the class
    (postproc.mask_views_argmax), then
      postproc == 0: fill holes, remove small objects, 8-connected label, dilate (cc_chain on pred == 1, :277-295);
      postproc == 1: postproc_other.process(pred_inside, model_mode, min_size=min_area) on the raw `pred == 1` (BEFORE fill holes, as
                     :289-290 passes it), then the disk dilation (:295).  The reference passes model_mode = opt.model['modelName'] = 'UNet',
                     and 'UNet' != 'unet' (postproc_other.py:35), so the watershed branch IS taken there: kept.
    Returns dict(final int32 [H,W], pred u8 [H,W] [, prob_mean f32 [K,H,W] with want_prob] [, counts int32 [1] with postproc 0]; `count`
    unless defer).  `defer=True`: nothing is read back (test.main pipelines images with this form).
    `restore=(ori_h, ori_w)` (the 'scale' test transform, test.py:281-283): as for infer_image - `final`, `counts` and `count` at the original
    size through postproc.restore_chain, `pred` and `prob_mean` at the scaled size; a ValueError with postproc == 1."""
    from . import postproc as postproc_mod, postproc_other, utils          # (`postproc` is the reference's option name here)
    if opt is not None:
        tta, all_img_test = opt.test['tta'], opt.all_img_test
        patch_size, overlap = opt.test['patch_size'], opt.test['overlap']
        min_area, radius, postproc =  opt.post['min_area'], opt.post['radius'], int(opt.post['postproc'])
        model_mode = opt.model['modelName']
    if restore is not None and int(postproc) == 1:
        raise ValueError(postproc_mod.SCALE_POSTPROC1)
    assert not model.training and image.dim() == 3
    _, H, W = image.shape
    xforms = list(postproc_mod.TTA_XFORMS) if tta else [0]
    V, K = len(xforms), mask_channels(model)
    mask_all = torch.empty((V, K, H * W), dtype=torch.float32, device=image.device)
    if all_img_test == 1:
        utils.split_forward_views(model, image, max(H, W), 0, xforms, out=(mask_all,))
    else:
        utils.split_forward_views(model, image, patch_size, overlap, xforms, out=(mask_all,))
    m = postproc_mod.mask_views_argmax(mask_all[None], xforms, H, W, want_prob=want_prob)
    pred = m['pred']
    if int(postproc) == 1:
        lab = postproc_other.process((pred == 1).to(torch.uint8), model_mode, min_size=min_area)
        out = dict(final=postproc_mod.dilate_labels(lab, radius)[0], pred=pred[0])
    else:
        cc = postproc_mod.cc_chain(pred, 1, min_area, radius) if restore is None else postproc_mod.restore_chain(pred, restore, 1, min_area, radius)
        out = dict(final=cc['final'][0], counts=cc['counts'], pred=pred[0])
    if want_prob:
        out['prob_mean'] = m['prob_mean'][0]
    if not defer:
        if 'counts' in out:
            out['count'] = int(out['counts'][0])
        else:                                              # (watershed labels keep their marker ids: count the distinct ones)
            f = out['final'].cpu().numpy()
            out['count'] = int(len(np.unique(f[f > 0])))
    return out


_NORM = {}


def scaled_input(img_u8, transform, device=None):
    """The test transform of an image with the 'scale' key on the device (test_transform((img,)) of test_dam.py:297 / test.py:213: Scale ->
    ToTensor -> Normalize).  img_u8: uint8 [H,W,3] tensor - [H,W] for a grey-scale dataset (mode L: resize.hip's one-channel form, the first
    entry of mean and std, x float32 [1,h,w]) -, on the host (uploaded as bytes through pinned memory) or already on the device.
    The image is resized there with Pillow's bilinear filter (resize.resize_bilinear, the size by resize.scaled_size), then converted and
    normalised with the fp32 operations of the host path (`/ 255.0`, `(x - mean) / std`).  Returns (x float32 [3,h,w] on the device,
    restore): restore = (H, W) for infer_image / infer_image_mask when the size changed, else None.  Nothing is read back."""
    from . import resize
    assert img_u8.dtype == torch.uint8 and (img_u8.dim() == 2 or (img_u8.dim() == 3 and img_u8.shape[2] == 3))
    nc = 1 if img_u8.dim() == 2 else 3
    H, W = int(img_u8.shape[0]), int(img_u8.shape[1])
    if not img_u8.is_cuda:
        dev = torch.device('cuda', torch.cuda.current_device()) if device is None else device
        img_u8 = img_u8.contiguous().pin_memory().to(dev, non_blocking=True)
    new = resize.scaled_size(W, H, transform['scale']) if 'scale' in transform else None
    restore = None
    if new is not None and (new[1], new[0]) != (H, W):
        img_u8 = resize.resize_bilinear(img_u8, (new[1], new[0]))
        restore = (H, W)
    # (tensor / tensor: the device's division by a Python scalar is a multiplication by its reciprocal, one ulp off the host's `/ 255.0`
    #  for some bytes)
    if ('255', img_u8.device) not in _NORM:
        _NORM[('255', img_u8.device)] = torch.full((1,), 255.0, dtype=torch.float32, device=img_u8.device)
    x = (img_u8[None] if nc == 1 else img_u8.permute(2, 0, 1)).contiguous().float() / _NORM[('255', img_u8.device)]
    if 'normalize' in transform:
        x = (x - _norm_pair(transform, nc, x.device)[0]) / _norm_pair(transform, nc, x.device)[1]
    return x, restore


def _norm_pair(transform, nc, device):
    """(mean, std) of the `normalize` transform as f32 [nc,1,1] device tensors: its first nc entries, uploaded once (a pageable copy would
    wait for the images in flight)"""
    mean, std = (list(v)[:nc] for v in transform['normalize'])
    key = (tuple(float(v) for v in mean), tuple(float(v) for v in std), device)
    if key not in _NORM:
        _NORM[key] = tuple(torch.tensor(v, dtype=torch.float32).view(nc, 1, 1).to(device) for v in (mean, std))
    return _NORM[key]


def host_input(image, transform, in_c=3):
    """ToTensor -> Normalize of the test transform on the host, as the entries always did it for RGB: a PIL image -> float32 [in_c,H,W]
    (in_c = 1: converted to mode L, the first entry of mean and std)"""
    nc, mode = (1, 'L') if in_c == 1 else (3, 'RGB')
    img = np.asarray(image.convert(mode), dtype=np.float32) / 255.0
    x = torch.from_numpy(img[:, :, None] if nc == 1 else img).permute(2, 0, 1).contiguous()
    if 'normalize' in transform:
        mean, std = transform['normalize']
        x = (x - torch.tensor(mean[:nc], dtype=torch.float32).view(nc, 1, 1)) / torch.tensor(std[:nc], dtype=torch.float32).view(nc, 1, 1)
    return x


def grey_transformed(image, opt):
    """A grey-scale dataset (opt.model['in_c'] == 1) whose image was read as RGB and went through the test transform at its original
    size - what test_dam.main and test_dam.process_image hand over: image float32 [3,H,W] on the device = bytes / 255.0 [- mean) / std].
    Returns what loading the file with convert('L') gives, float32 [1,H,W]: the bytes are recovered (exact, as in scale_transformed),
    Pillow's L = (R * 19595 + G * 38470 + B * 7471 + 0x8000) >> 16 is taken in integers (the identity for a grey image stored as RGB),
    and the result is converted and normalised with the first entry of mean and std.  Anything else comes back as it is."""
    if opt is None or opt.model.get('in_c', 3) != 1 or image.dim() != 3 or image.shape[0] != 3:
        return image
    transform = getattr(opt, 'transform', {}).get('test', {})
    x = image.float()
    if 'normalize' in transform:
        x = x * _norm_pair(transform, 3, x.device)[1] + _norm_pair(transform, 3, x.device)[0]
    b = torch.round(x * 255.0).clamp_(0, 255).to(torch.int32)
    grey = ((b[0] * 19595 + b[1] * 38470 + b[2] * 7471 + 0x8000) >> 16).to(torch.uint8)
    if ('255', x.device) not in _NORM:
        _NORM[('255', x.device)] = torch.full((1,), 255.0, dtype=torch.float32, device=x.device)
    x = grey[None].float() / _NORM[('255', x.device)]
    if 'normalize' in transform:
        x = (x - _norm_pair(transform, 1, x.device)[0]) / _norm_pair(transform, 1, x.device)[1]
    return x


def _has_scale(opt):
    return opt is not None and 'scale' in getattr(opt, 'transform', {}).get('test', {})


def scale_transformed(image, transform):
    """The Scale step for an image that already went through the rest of the test transform at its original size: image float32 [3,H,W] on
    the device = (bytes / 255.0 [- mean) / std], as test_dam.main and test_dam.process_image build it.  Pillow resizes bytes, so the bytes
    are recovered first - round((x * std + mean) * 255) is exact: the float32 error of the round trip is below 1e-4 of a grey level - and
    then go through scaled_input, whose result has the bits of Scale -> ToTensor -> Normalize on the original bytes.  Returns (x, restore);
    the image itself and None when Scale leaves its size alone.  Nothing is read back."""
    from . import resize
    assert image.is_cuda and image.dtype == torch.float32 and image.dim() == 3 and image.shape[0] in (1, 3)
    nc = int(image.shape[0])
    H, W = int(image.shape[1]), int(image.shape[2])
    new = resize.scaled_size(W, H, transform['scale'])
    if new is None or (new[1], new[0]) == (H, W):
        return image, None
    x = image
    if 'normalize' in transform:
        x = x * _norm_pair(transform, nc, x.device)[1] + _norm_pair(transform, nc, x.device)[0]
    img_u8 = torch.round(x * 255.0).clamp_(0, 255).to(torch.uint8)
    return scaled_input(img_u8[0].contiguous() if nc == 1 else img_u8.permute(1, 2, 0).contiguous(), transform)


def scale_inputs(image, opt, ori_size=None):
    """(x float32 [3,h,w] on the device, restore) for the entries' process_image.  A uint8 image [H,W,3] (tensor, numpy array or PIL image:
    before the test transform) goes through scaled_input, which applies opt.transform['test'] on the device.  A float tensor [3,h,w] is
    already transformed: with `ori_size=(ori_h, ori_w)` it was also scaled by the caller (the reference's Scale on the host) and the mask
    is resized back to ori_size; without it, it is at its original size and the Scale step runs here (scale_transformed)."""
    if not torch.is_tensor(image):
        mode = 'L' if opt.model.get('in_c', 3) == 1 else 'RGB'
        image = torch.from_numpy(np.array(image if isinstance(image, np.ndarray) else image.convert(mode), dtype=np.uint8))
    if image.dtype == torch.uint8:
        return scaled_input(image, opt.transform['test'])
    x = image.cuda().float()
    if ori_size is not None:
        restore = (int(ori_size[0]), int(ori_size[1]))
        return x, (restore if restore != tuple(x.shape[-2:]) else None)
    if _has_scale(opt):
        return scale_transformed(x, opt.transform['test'])
    return x, None
