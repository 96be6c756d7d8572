"""postproc_other.process on the GPU (reference: postproc_other.py:15-99).

Same signature as the reference: `process(pred, model_mode, min_size=10, ws=True) -> labels`.  `pred` is a numpy HW
probability / binary map (or a torch CUDA tensor [H,W] / [N,H,W]); the result is an int32 label map in the input's container type.
Every model_mode of the reference is served:
  'unet'      forces ws=False exactly like postproc_other.py:35 - that branch (fill holes -> 4-connected label -> remove small labels,
              :49-52) is `cdnet_fill_label_process`, built from the kernels of the watershed entry's marker stage;
  'micronet'  the same branch, then every instance dilated by the 3 x 3 cross, its holes filled, painted in id order (:56-68);
  'dcan'      pred is [H,W,2] (or [N,H,W,2]) = (blb, cnt): `blb - cnt > 0.3` -> 4-connected label -> remove small labels -> every instance
              dilated by k_disk (the diamond of radius 3), filled, painted (:70-97);
  any other   the watershed variant (ws=True) or the 'unet' branch (ws=False).
The per-instance loop of the last two is `redilate_instances` (cdnet_instance_redilate, csrc/instance_fill.hip): one wave per instance on
bit planes of its bounding box, the result the maximum id whose dilated and filled instance covers a pixel.
All compute runs in csrc (postproc.hip, instance_fill.hip); there is no CPU fallback.  `process_host` is the yardstick the device is
compared with - the reference's two branches restated with numpy + scipy - never a code path of `process`."""
import numpy as np
import torch

from . import _lib


def watershed_process(pred_u8, min_size=10, stages=False):
    """pred_u8: torch.uint8 CUDA [N,H,W], non-zero = foreground.  Returns labels int32 [N,H,W] (and dist u8, marker i32
    when stages=True)."""
    assert pred_u8.is_cuda and pred_u8.dtype == torch.uint8 and pred_u8.dim() == 3
    pred_u8 = pred_u8.contiguous()
    N, H, W = pred_u8.shape
    lib = _lib.load()
    ws = torch.empty((lib.cdnet_watershed_workspace_bytes(N, H, W),), dtype=torch.uint8, device=pred_u8.device)
    labels = torch.empty((N, H, W), dtype=torch.int32, device=pred_u8.device)
    dist = torch.empty((N, H, W), dtype=torch.uint8, device=pred_u8.device) if stages else None
    marker = torch.empty((N, H, W), dtype=torch.int32, device=pred_u8.device) if stages else None
    _lib.call('cdnet_watershed_process', _lib.ptr(pred_u8), N, H, W, int(min_size), _lib.ptr(ws), ws.numel(), _lib.ptr(dist),
              _lib.ptr(marker), _lib.ptr(labels), _lib.stream_ptr())
    return (labels, dist, marker) if stages else labels


def _label_chain(entry, pred_u8, min_size):
    assert pred_u8.is_cuda and pred_u8.dtype == torch.uint8 and pred_u8.dim() == 3
    pred_u8 = pred_u8.contiguous()
    N, H, W = pred_u8.shape
    lib = _lib.load()
    ws = torch.empty((lib.cdnet_watershed_workspace_bytes(N, H, W),), dtype=torch.uint8, device=pred_u8.device)
    labels = torch.empty((N, H, W), dtype=torch.int32, device=pred_u8.device)
    _lib.call(entry, _lib.ptr(pred_u8), N, H, W, int(min_size), _lib.ptr(ws), ws.numel(), _lib.ptr(labels), _lib.stream_ptr())
    return labels


def fill_label_process(pred_u8, min_size=10):
    """ws=False branch on the device: pred_u8 torch.uint8 CUDA [N,H,W], non-zero = foreground -> labels int32 [N,H,W]"""
    return _label_chain('cdnet_fill_label_process', pred_u8, min_size)


def label_process(pred_u8, min_size=10):
    """the 'dcan' branch's labelling (postproc_other.py:79-80): fill_label_process without the hole filling"""
    return _label_chain('cdnet_label_process', pred_u8, min_size)


def redilate_limits():
    """(rows, cols): the largest window (an instance's bounding box grown by r, clipped to the image) that cdnet_instance_redilate works
    on in LDS; larger windows take the workspace form"""
    lib = _lib.load()
    return int(lib.cdnet_instance_redilate_lds_rows()), int(lib.cdnet_instance_redilate_lds_cols())


def _check(err, what):
    e = int(err.item())
    if e == 1:
        raise ValueError('%s: a label id lies outside 0..cap' % what)
    if e:
        raise RuntimeError('%s: device error flag %d (the flood of an instance did not end within its pass bound)' % (what, e))


def _redilate(labels, r, cap):
    """labels int32 CUDA [N,H,W] contiguous -> (out, err): no host synchronisation"""
    N, H, W = labels.shape
    lib = _lib.load()
    nbytes = lib.cdnet_instance_redilate_workspace_bytes(N, H, W, int(cap))
    if nbytes == 0:
        raise ValueError('redilate_instances: sizes N=%d H=%d W=%d cap=%d are not served (N * cap <= 2^28)' % (N, H, W, cap))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=labels.device)
    out = torch.empty_like(labels)
    err = torch.empty((1,), dtype=torch.int32, device=labels.device)
    _lib.call('cdnet_instance_redilate', _lib.ptr(labels), N, H, W, int(r), int(cap), _lib.ptr(ws), ws.numel(), _lib.ptr(out), _lib.ptr(err),
              _lib.stream_ptr())
    return out, err


def redilate_instances(labels, r, cap=None):
    """The per-instance loop of postproc_other.py:62-68 (r = 1) and :92-97 (r = 3) for int32 CUDA label maps [N,H,W] or [H,W], into a new
    tensor: out(p) = the largest id k with p in binary_fill_holes(binary_dilation(labels == k, diamond(r))).  Ids must lie in 1..cap
    (0 = background; ValueError otherwise); cap=None takes the largest id present (one read-back)."""
    assert labels.is_cuda and labels.dtype == torch.int32 and labels.dim() in (2, 3)
    lab = labels.contiguous()
    if lab.dim() == 2:
        lab = lab[None]
    if cap is None:
        cap = max(int(lab.max().item()), 1) if lab.numel() else 1
    out, err = _redilate(lab, r, cap)
    _check(err, 'redilate_instances')
    return out[0] if labels.dim() == 2 else out


def _max_components(H, W):
    """no 4-connected labelling of an H x W image has more components than a checkerboard: the id bound of the chains' label maps"""
    return (H * W + 1) // 2


def process_device(pred, model_mode, min_size=10, ws=True):
    """`process` for CUDA tensors without the read-back of the error flag: returns (labels int32 [N,H,W] or [H,W], err) with err an int32 [1]
    device tensor for 'micronet' / 'dcan' (0 = fine; the ids come from this module's own labelling, so 1 cannot occur) and None otherwise."""
    t = pred
    if model_mode == 'dcan':
        assert t.dim() in (3, 4) and t.shape[-1] == 2, 'Prediction should have contour and blb'          # postproc_other.py:70
        if t.dtype not in (torch.float32, torch.float64):
            raise TypeError("postproc_other.process('dcan'): float32 or float64 expected, got %s (the reference would wrap integers)" % t.dtype)
        squeeze = t.dim() == 3
        if squeeze:
            t = t[None]
        thr = torch.tensor(0.3, dtype=t.dtype, device=t.device)            # the threshold in the array's own type, as numpy compares
        binary = ((t[..., 0] - t[..., 1]) > thr).to(torch.uint8)           # :71-78
        lab = label_process(binary, min_size)                              # :79-80
        out, err = _redilate(lab, 3, _max_components(*lab.shape[1:]))      # :81-97
        return (out[0] if squeeze else out), err
    assert t.dim() in (2, 3), 'Prediction shape is not HW'                 # postproc_other.py:30
    squeeze = t.dim() == 2
    if squeeze:
        t = t[None]
    binary = (t > 0.5).to(torch.uint8)                                     # :31-32
    if model_mode in ('unet', 'micronet'):
        ws = False                                                         # :35
    err = None
    if ws:
        out = watershed_process(binary, min_size)
    else:
        out = fill_label_process(binary, min_size)                         # :51-53
    if model_mode == 'micronet':
        out, err = _redilate(out, 1, _max_components(*out.shape[1:]))      # :56-68
    return (out[0] if squeeze else out), err


def process(pred, model_mode, min_size=10, ws=True):
    is_np = isinstance(pred, np.ndarray)
    t = torch.from_numpy(np.ascontiguousarray(pred)).cuda() if is_np else pred
    out, err = process_device(t, model_mode, min_size, ws)
    if err is not None:
        _check(err, "postproc_other.process('%s')" % model_mode)
    return out.cpu().numpy() if is_np else out


def _remove_small_host(lab, min_size):
    """skimage.morphology.remove_small_objects on a label image: ids with fewer than min_size pixels become 0, the others are kept"""
    small = np.bincount(lab.ravel()) < min_size
    small[0] = False
    out = lab.copy()
    out[small[lab]] = 0
    return out


def redilate_host(lab, r):
    """postproc_other.py:62-68 / :92-97 literally: every id in 1..max dilates alone over the whole image (cv2.dilate of a 0/1 image with its
    default border = binary_dilation with border_value 0), has its holes filled and is painted over the canvas.  int32 out."""
    from scipy import ndimage as ndi
    diamond = ndi.iterate_structure(ndi.generate_binary_structure(2, 1), r)
    canvas = np.zeros(lab.shape, np.int32)
    for inst_id in range(1, int(lab.max()) + 1):
        inst = ndi.binary_dilation(lab == inst_id, structure=diamond)
        inst = ndi.binary_fill_holes(inst)
        canvas[inst] = inst_id
    return canvas


def process_host(pred, model_mode, min_size=10, ws=True):
    """The reference's 'micronet' and 'dcan' branches restated with numpy + scipy only (cv2.dilate and skimage's remove_small_objects by
    their exact binary-morphology / bincount equivalents), with the literal per-instance whole-image loop.  One image: [H,W], or [H,W,2]
    for 'dcan'.  This is the yardstick the device chain is compared with, bit for bit (as weight_map_host and object_hausdorff_host are
    for their kernels) - slow (a whole-image dilation and fill per instance) and never called by `process`.  `ws` is ignored: 'micronet'
    forces it off (:35) and 'dcan' has no such branch."""
    from scipy import ndimage as ndi
    pred = np.asarray(pred)
    if model_mode == 'micronet':
        assert pred.ndim == 2, 'Prediction shape is not HW'
        lab = ndi.label(ndi.binary_fill_holes(pred > 0.5))[0].astype(np.int32)
        return redilate_host(_remove_small_host(lab, min_size), 1)
    if model_mode == 'dcan':
        assert pred.ndim == 3 and pred.shape[2] == 2, 'Prediction should have contour and blb'
        if pred.dtype not in (np.float32, np.float64):
            raise TypeError("process_host('dcan'): float32 or float64 expected, got %s" % pred.dtype)
        diff = pred[..., 0] - pred[..., 1]
        lab = ndi.label(diff > 0.3)[0].astype(np.int32)
        return redilate_host(_remove_small_host(lab, min_size), 3)
    raise ValueError("process_host restates the 'micronet' and 'dcan' branches only, not %r" % (model_mode,))
