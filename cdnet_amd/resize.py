"""Pillow's 8-bit bilinear resize - the reference's 'scale' test transform - with its coefficient tables made here on the host.

  resize_tables(in_size, out_size)          bounds int32 [out][2], kk int32 [out][ksize] of one axis (cached)
  resize_bilinear(img_u8, (oh, ow), form)   Image.resize((ow, oh), Image.BILINEAR) of a uint8 tensor; device tensors on csrc/resize.hip
  resize_mask(mask01, (oh, ow))             misc.imresize(mask * 255, (oh, ow), 'bilinear') > 127.5 as {0, 1} (test_dam.py:552-553)
  resize_bilinear_host(a, (oh, ow))         the numpy mirror on the same tables (CPU tensors; what the tests compare the device with)
  scaled_size(w, h, size)                   the output size rule of Scale (my_transforms_direction.py:46-64)

Images are [H, W] (mode L), [H, W, C] with C = 1 or 3 (RGB interleaved, as np.asarray(img) gives it) or a batch [N, H, W, C] of one size.
The tables follow Pillow's precompute_coeffs / normalize_coeffs_8bpc (src/libImaging/Resample.c) operation by operation in float64; the
device computes no coefficient.
"""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2

_TABLES = {}
_DEV_TABLES = {}


def resize_tables(in_size, out_size):
    """(bounds int32 [out][2] = (xmin, n), kk int32 [out][ksize]) of the bilinear filter for one axis, default box (0, in_size)"""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError('resize_tables: sizes must be >= 1, got {} -> {}'.format(in_size, out_size))
    key = (in_size, out_size)
    if key in _TABLES:
        return _TABLES[key]
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale                                        # bilinear: filterp->support = 1.0
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)            # (int) truncates toward zero
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size)
    n = xmax - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    arg = ((x + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss
    w = np.where(x < n[:, None], np.maximum(1.0 - np.abs(arg), 0.0), 0.0)              # 1 - |x| below 1, else 0
    ww = np.zeros(out_size, dtype=np.float64)
    for j in range(ksize):                                                             # left to right, as the C loop adds
        ww = ww + w[:, j]
    nz = ww != 0.0
    w[nz] = w[nz] / ww[nz][:, None]
    scaled = w * float(1 << PRECISION_BITS)
    kk = np.where(w < 0, np.trunc(-0.5 + scaled), np.trunc(0.5 + scaled)).astype(np.int32)
    bounds = np.ascontiguousarray(np.stack([xmin, n], axis=1).astype(np.int32))
    tab = (bounds, np.ascontiguousarray(kk))
    for a in tab:
        a.setflags(write=False)
    _TABLES[key] = tab
    return tab


def scaled_size(w, h, size):
    """(ow, oh) of Scale(size) for a w x h image, or None when the image is returned unchanged: an int `size` leaves an image whose smaller
    edge already equals it, else sets the smaller edge to `size` and the other to int(size * other / smaller); a pair is (ow, oh) as is."""
    if isinstance(size, (int, np.integer)):
        size = int(size)
        if (w <= h and w == size) or (h <= w and h == size):
            return None
        if w < h:
            return size, int(size * h / w)
        return int(size * w / h), size
    ow, oh = size
    return int(ow), int(oh)


def _canon(shape):
    """(N, H, W, C) of an image array shape"""
    if len(shape) == 2:
        return (1,) + tuple(shape) + (1,)
    if len(shape) == 3:
        return (1,) + tuple(shape)
    if len(shape) == 4:
        return tuple(shape)
    raise ValueError('an image is [H, W], [H, W, C] or [N, H, W, C], got shape {}'.format(tuple(shape)))


def _out_shape(shape, oh, ow):
    if len(shape) == 2:
        return (oh, ow)
    if len(shape) == 3:
        return (oh, ow, shape[2])
    return (shape[0], oh, ow, shape[3])


def _pass_host(a, axis, out_size):
    """one pass along `axis` of a uint8 array: clip8((2^21 + sum a * kk) >> 22), the sum in integers as Pillow holds it"""
    in_size = a.shape[axis]
    bounds, kk = resize_tables(in_size, out_size)
    a = np.moveaxis(a, axis, -1).astype(np.int64)
    acc = np.full(a.shape[:-1] + (out_size,), 1 << (PRECISION_BITS - 1), dtype=np.int64)
    for j in range(kk.shape[1]):
        idx = np.minimum(bounds[:, 0].astype(np.int64) + j, in_size - 1)               # (taps past n have weight 0)
        acc += a[..., idx] * kk[:, j].astype(np.int64)
    out = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, -1, axis)


def resize_bilinear_host(a, size):
    """numpy mirror of the device kernels: Image.resize((ow, oh), Image.BILINEAR) of a uint8 array; size = (oh, ow)"""
    a = np.asarray(a)
    if a.dtype != np.uint8:
        raise TypeError('resize_bilinear_host takes uint8, got {}'.format(a.dtype))
    oh, ow = int(size[0]), int(size[1])
    N, H, W, Cn = _canon(a.shape)
    if Cn not in (1, 3):
        raise ValueError('C = {} not in (1, 3)'.format(Cn))
    x = a.reshape(N, H, W, Cn)
    if ow != W:
        x = _pass_host(x, 2, ow)                     # horizontal first, rounded to u8 ...
    if oh != H:
        x = _pass_host(x, 1, oh)                     # ... before the vertical pass reads it
    return np.ascontiguousarray(x).reshape(_out_shape(a.shape, oh, ow)).copy()


def _device_tables(in_size, out_size, device):
    import torch
    key = (in_size, out_size, device.index if device.index is not None else torch.cuda.current_device())
    t = _DEV_TABLES.get(key)
    if t is None:
        bounds, kk = resize_tables(in_size, out_size)
        t = (torch.from_numpy(bounds.copy()).to(device), torch.from_numpy(kk.copy()).to(device), int(kk.shape[1]))
        _DEV_TABLES[key] = t
    return t


def _resize_device(img, oh, ow, mask_mode, form):
    import torch
    from . import _lib
    N, H, W, Cn = _canon(img.shape)
    if Cn not in (1, 3):
        raise ValueError('C = {} not in (1, 3)'.format(Cn))
    img = img.contiguous()
    dev = img.device
    hb = hk = vb = vk = None
    hks = vks = 0
    if ow != W:
        hb, hk, hks = _device_tables(W, ow, dev)
    if oh != H:
        vb, vk, vks = _device_tables(H, oh, dev)
    nbytes = _lib.load().cdnet_resize_workspace_bytes(N, H, W, Cn, oh, ow, int(form))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev) if nbytes else None
    out = torch.empty(_out_shape(tuple(img.shape), oh, ow), dtype=torch.uint8, device=dev)
    _lib.call('cdnet_resize_bilinear', _lib.ptr(img), N, H, W, Cn, oh, ow, _lib.ptr(hb), _lib.ptr(hk), hks, _lib.ptr(vb), _lib.ptr(vk), vks,
              int(mask_mode), int(form), _lib.ptr(ws), nbytes, _lib.ptr(out), _lib.stream_ptr())
    return out


def last_form():
    """the form the last device resize of this thread ran: 0 copy (equal sizes), 1 LDS form, 2 two-pass form"""
    from . import _lib
    return int(_lib.load().cdnet_resize_last_form())


def resize_bilinear(img_u8, size, form=0):
    """Image.resize((ow, oh), Image.BILINEAR) of a uint8 tensor, size = (oh, ow).  A device tensor runs on csrc/resize.hip (form 0: the
    library chooses, 1: LDS form, 2: two-pass form); a CPU tensor on the numpy mirror."""
    import torch
    assert torch.is_tensor(img_u8) and img_u8.dtype == torch.uint8, 'resize_bilinear takes a uint8 tensor'
    oh, ow = int(size[0]), int(size[1])
    if not img_u8.is_cuda:
        return torch.from_numpy(resize_bilinear_host(img_u8.numpy(), (oh, ow)))
    return _resize_device(img_u8, oh, ow, 0, form)


def resize_mask(mask01, size, form=0):
    """(misc.imresize(mask * 255, (oh, ow), 'bilinear') > 127.5) as uint8 {0, 1} of a {0, 1} uint8 mask [H, W] or [N, H, W] in one call
    (test_dam.py:552-553, test.py:282-283)"""
    import torch
    assert torch.is_tensor(mask01) and mask01.dtype == torch.uint8 and mask01.dim() in (2, 3), 'resize_mask takes a uint8 mask [H, W] or [N, H, W]'
    oh, ow = int(size[0]), int(size[1])
    m4 = mask01.reshape((1,) * (3 - mask01.dim()) + tuple(mask01.shape) + (1,))
    if not mask01.is_cuda:
        out = torch.from_numpy((resize_bilinear_host((m4.numpy() * 255).astype(np.uint8), (oh, ow)) > 127.5).astype(np.uint8))
    else:
        out = _resize_device(m4, oh, ow, 1, form)
    return out.reshape(tuple(mask01.shape[:-2]) + (oh, ow))
