"""Training augmentation of the reference's default recipe (my_transforms_direction.py:155-540), on the device.

  draw_params(rs, H, W, recipe)       one sample's parameters, drawn from the loader's RandomState in the reference's order
  augment_batch(sources, params, ...) one batch on the device: cdnet_augment_batch (csrc/augment.hip)
  augment_host(img, weight, label, p, size, field=None)
                                      the same sample on the host: PIL for the colour chain and the filters, numpy for the
                                      restated OpenCV geometry; it serves TileBatches(device='cpu') and checks the device path
  Recipe                              which steps run, the elastic parameters (alpha, sigma, alpha_affine) and the crop size

Per sample, on the whole source image: random_color -> horizontal / vertical flip -> random_elastic (random affine, then a
Gaussian-smoothed displacement field) -> random_chooseAug -> random_crop.  The contract is the same distributions and the same operation
for given parameters, not the reference's random streams (Python `random`, np.random and albumentations' RandomState spread over
DataLoader workers).  The colour chain and the filters equal Pillow's bit for bit; the geometry restates OpenCV 4's nearest rules (cv2
parity unpinned); the field noise is a counter-based hash of (seed, plane, y, x), not numpy's MT19937.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib

HALO = 6                                   # the field window: crop + 6 px on every side (csrc/augment.hip)


class AugSample(C.Structure):              # cdnet_aug_sample (include/cdnet_hip.h)
    _fields_ = [('minv', C.c_double * 6), ('img', C.c_void_p), ('weight', C.c_void_p), ('label', C.c_void_p)] + \
        [(n, C.c_int32) for n in ('H', 'W', 'img_stride', 'weight_stride', 'label_stride', 'label_i32')] + \
        [('color', C.c_float * 4)] + [(n, C.c_int32) for n in ('hflip', 'vflip', 'filter', 'y0', 'x0')] + \
        [('alpha', C.c_float), ('sigma', C.c_float), ('seed', C.c_uint32)]


@dataclass
class Recipe:
    """the steps of a transform dict (options.py:327-351) and the elastic parameters; the reference ignores random_elastic's [6, 15]
    arguments and always runs ElasticTransform(alpha=1, sigma=50, alpha_affine=50) (my_transforms_direction.py:281)"""
    size: int
    color: bool = True
    hflip: bool = True
    vflip: bool = True
    elastic: bool = True
    choose_aug: bool = True
    elastic_alpha: float = 1.0
    elastic_sigma: float = 50.0
    elastic_alpha_affine: float = 50.0

    @classmethod
    def from_transform(cls, transform, **elastic):
        return cls(size=int(transform['random_crop']), color=bool(transform.get('random_color')),
                   hflip=bool(transform.get('horizontal_flip')), vflip=bool(transform.get('vertical_flip')),
                   elastic=bool(transform.get('random_elastic')), choose_aug=bool(transform.get('random_chooseAug')), **elastic)


@dataclass
class Params:
    """one sample's drawn parameters"""
    color: tuple                # Color, Brightness, Contrast, Sharpness factors
    hflip: int
    vflip: int
    minv: tuple                 # inverse affine (2 x 3 row-major, float64): destination -> source pixel, flipped frame
    alpha: float
    sigma: float
    seed: int
    filter: int                 # 0 none, 1 BLUR, 2 GaussianBlur, 3 MedianFilter
    y0: int
    x0: int


def affine_points(H, W):
    """albumentations' pts1 (row, col order, fed to OpenCV as (x, y)): centre (H, W) // 2, square min(H, W) // 3"""
    c = np.array((H, W), np.float32) // 2
    s = np.float32(min(H, W) // 3)
    return np.array([c + s, [c[0] + s, c[1] - s], c - s], np.float32)


def affine_inverse(pts1, pts2):
    """M = getAffineTransform(pts1, pts2) (float64 solve), then invertAffineTransform's formula: the 6 doubles the kernel reads"""
    A = np.zeros((6, 6))
    rhs = np.zeros(6)
    for i in range(3):
        x, y = float(pts1[i, 0]), float(pts1[i, 1])
        A[2 * i, :3] = (x, y, 1.0)
        A[2 * i + 1, 3:] = (x, y, 1.0)
        rhs[2 * i], rhs[2 * i + 1] = float(pts2[i, 0]), float(pts2[i, 1])
    M = np.linalg.solve(A, rhs)
    D = M[0] * M[4] - M[1] * M[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22, A12, A21 = M[4] * D, M[0] * D, -M[1] * D, -M[3] * D
    b1 = -A11 * M[2] - A12 * M[5]
    b2 = -A21 * M[2] - A22 * M[5]
    return (A11, A12, b1, A21, A22, b2)


IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def draw_params(rs, H, W, recipe):
    """the reference's draws in its order (RandomColor :162-172, flips :233 / :251, ElasticTransform's affine offsets and field,
    RandomChooseAug :451, RandomCrop): `rs` is the loader's numpy RandomState"""
    color = tuple(1 + (rs.rand() - 0.5) for _ in range(4)) if recipe.color else (1.0, 1.0, 1.0, 1.0)
    hflip = int(rs.rand() < 0.5) if recipe.hflip else 0
    vflip = int(rs.rand() < 0.5) if recipe.vflip else 0
    minv, alpha, seed = IDENTITY, 0.0, 0
    if recipe.elastic:
        pts1 = affine_points(H, W)
        aa = recipe.elastic_alpha_affine
        pts2 = pts1 + rs.uniform(-aa, aa, size=pts1.shape).astype(np.float32)
        if min(H, W) >= 3:                       # a square of size 0 has no affine (albumentations fails there)
            minv = affine_inverse(pts1, pts2)
        alpha = float(recipe.elastic_alpha)
        seed = int(rs.randint(0, 2 ** 31))
    filt = 0
    if recipe.choose_aug:
        r = rs.rand()
        filt = 1 if r < 0.25 else 2 if r < 0.5 else 3 if r < 0.75 else 0
    s = recipe.size
    y0 = int(rs.randint(0, max(H - s, 0) + 1))
    x0 = int(rs.randint(0, max(W - s, 0) + 1))
    return Params(color, hflip, vflip, tuple(float(v) for v in minv), alpha, float(recipe.elastic_sigma), seed, filt, y0, x0)


def gauss_radius(sigma):
    return int(np.float32(4.0) * np.float32(sigma) + np.float32(0.5))


# ---------------------------------------------------------------------------------------------------- host implementation

def _fmix32(h):
    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x85EBCA6B)
    h = h ^ (h >> np.uint32(13))
    h = h * np.uint32(0xC2B2AE35)
    return h ^ (h >> np.uint32(16))


def field_noise(seed, plane, H, W):
    """the device's displacement noise U[-1, 1) (f32 [H, W]) of plane 0 (dx) or 1 (dy)"""
    with np.errstate(over='ignore'):
        h = _fmix32(np.uint32(seed) * np.uint32(0x9E3779B1) + np.uint32(plane) * np.uint32(0x7F4A7C15))
        h = _fmix32(h ^ (np.arange(H, dtype=np.uint32) * np.uint32(0xC2B2AE3D)))[:, None]
        h = _fmix32(h ^ (np.arange(W, dtype=np.uint32) * np.uint32(0x27D4EB2F))[None, :])
    return (h >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 8388608.0) - np.float32(1.0)


def field_window(p, H, W, size):
    """dx, dy (f32 [2, size + 12, size + 12]) over the crop window as the host computes them: scipy's gaussian_filter of the device's
    noise (mode 'reflect', truncate 4) times alpha; 0 outside the image"""
    from scipy.ndimage import gaussian_filter
    FS = size + 2 * HALO
    out = np.zeros((2, FS, FS), np.float32)
    ys, xs = np.arange(p.y0 - HALO, p.y0 - HALO + FS), np.arange(p.x0 - HALO, p.x0 - HALO + FS)
    iy, ix = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
    for k in range(2):
        f = gaussian_filter(field_noise(p.seed, k, H, W), p.sigma, mode='reflect', truncate=4.0) * np.float32(p.alpha)
        out[k][np.ix_(iy, ix)] = f[np.ix_(ys[iy], xs[ix])]
    return out


def colour_chain(img, color):
    """random_color (my_transforms_direction.py:161-179) with given factors, through PIL itself"""
    from PIL import Image, ImageEnhance
    im = Image.fromarray(np.ascontiguousarray(img))
    for enh, f in zip((ImageEnhance.Color, ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Sharpness), color):
        im = enh(im).enhance(f)
    return np.asarray(im)


def apply_filter(img, code):
    """random_chooseAug's filter `code` (1 BLUR, 2 GaussianBlur, 3 MedianFilter, 0 none) through PIL"""
    from PIL import Image, ImageFilter
    if code == 0:
        return img
    f = (None, ImageFilter.BLUR, ImageFilter.GaussianBlur, ImageFilter.MedianFilter)[code]
    return np.asarray(Image.fromarray(np.ascontiguousarray(img)).filter(f))


def warp_source(minv, H, W, ry, rx):
    """OpenCV 4 warpAffine, nearest, restated: fixed point with AB_BITS = 10 and a half-step rounding delta; -> (Y, X, inside)"""
    M = minv
    ry, rx = ry.astype(np.float64), rx.astype(np.float64)
    X0 = np.rint((M[1] * ry + M[2]) * 1024.0).astype(np.int64) + 512
    Y0 = np.rint((M[4] * ry + M[5]) * 1024.0).astype(np.int64) + 512
    X = (X0 + np.rint(M[0] * rx * 1024.0).astype(np.int64)) >> 10
    Y = (Y0 + np.rint(M[3] * rx * 1024.0).astype(np.int64)) >> 10
    return Y, X, (X >= 0) & (X < W) & (Y >= 0) & (Y < H)


def augment_host(img, weight, label, p, size, field=None):
    """one sample through the whole chain on the host.  img u8 [H, W, 3], weight u8 [H, W], label u8 / i32 [H, W]; `field` (f32 [2,
    size + 12, size + 12], as augment_batch returns it) replaces the host's own dx, dy when given.  Returns the crop (img u8 [s, s, 3],
    weight u8 [s, s], label [s, s]) before the division by 255."""
    H, W = weight.shape
    im = colour_chain(img, p.color)
    planes = [im[..., c] for c in range(3)] + [weight, label]
    if p.hflip:
        planes = [a[:, ::-1] for a in planes]
    if p.vflip:
        planes = [a[::-1] for a in planes]
    # elastic: q -> r = round(q + d(q)) (remap) -> s = M^-1 r (warpAffine); anything outside reads 0 in every plane
    qy, qx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    ry, rx, inside = qy, qx, np.ones((H, W), bool)
    if p.alpha != 0.0:
        if field is None:
            field = field_window(p, H, W, size)
        d = np.zeros((2, H, W), np.float32)
        FS = size + 2 * HALO
        ys, xs = np.arange(p.y0 - HALO, p.y0 - HALO + FS), np.arange(p.x0 - HALO, p.x0 - HALO + FS)
        iy, ix = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
        for k in range(2):
            d[k][np.ix_(ys[iy], xs[ix])] = np.asarray(field[k], np.float32)[np.ix_(iy, ix)]
        rx = np.rint(qx.astype(np.float32) + d[0]).astype(np.int64)
        ry = np.rint(qy.astype(np.float32) + d[1]).astype(np.int64)
        inside = (rx >= 0) & (rx < W) & (ry >= 0) & (ry < H)
    Y, X, ok = warp_source(p.minv, H, W, ry, rx)
    ok &= inside
    Yc, Xc = np.where(ok, Y, 0), np.where(ok, X, 0)
    warped = [np.where(ok, a[Yc, Xc], 0).astype(a.dtype) for a in planes]
    im = apply_filter(np.stack(warped[:3], -1), p.filter)
    s = size
    out = [im, warped[3], warped[4]]
    out = [a[p.y0:p.y0 + s, p.x0:p.x0 + s] for a in out]
    if out[1].shape != (s, s):
        out = [np.pad(a, ((0, s - a.shape[0]), (0, s - a.shape[1])) + ((0, 0),) * (a.ndim - 2)) for a in out]
    return [np.ascontiguousarray(a) for a in out]


# ---------------------------------------------------------------------------------------------------- device path

class Source:
    """one source image resident on the device: img u8 [H, W, 3], weight u8 [H, W], label u8 [H, W] (channel 0) or i32 [H, W]"""

    def __init__(self, img, weight, label, dev):
        self.H, self.W = weight.shape[:2]
        self.img = torch.from_numpy(np.array(img, dtype=np.uint8, order='C')).to(dev)          # (a copy: PIL arrays are read-only)
        self.weight = torch.from_numpy(np.array(weight if weight.ndim == 2 else weight[:, :, 0], dtype=np.uint8, order='C')).to(dev)
        lab = label if label.ndim == 2 else label[:, :, 0]
        self.label_i32 = lab.dtype != np.uint8
        self.label = torch.from_numpy(np.array(lab, dtype=np.int32 if self.label_i32 else np.uint8, order='C')).to(dev)


_WS = {}


def augment_batch(sources, params, size, normalize=None, want_field=False):
    """the batch on the device (one call of cdnet_augment_batch, csrc/augment.hip).  sources: [Source], params: [Params].
    Returns (image f32 [B, 3, s, s], weight u8 [B, s, s], label u8 / i32 [B, s, s], varied i32 [B][, field f32 [B, 2, s + 12, s + 12]]);
    varied[b] == 0: the label crop holds one value (re-draw)."""
    B = len(sources)
    assert B == len(params) and B > 0
    dev = sources[0].img.device
    label_i32 = int(sources[0].label_i32)
    table = (AugSample * B)()
    rmax = 0
    for t, src, p in zip(table, sources, params):
        t.minv[:] = p.minv
        t.img, t.weight, t.label = src.img.data_ptr(), src.weight.data_ptr(), src.label.data_ptr()
        t.H, t.W, t.img_stride, t.weight_stride, t.label_stride, t.label_i32 = src.H, src.W, 3 * src.W, src.W, src.W, int(src.label_i32)
        t.color[:] = p.color
        t.hflip, t.vflip, t.filter, t.y0, t.x0 = p.hflip, p.vflip, p.filter, p.y0, p.x0
        t.alpha, t.sigma, t.seed = p.alpha, p.sigma, p.seed
        if p.alpha != 0.0:
            rmax = max(rmax, gauss_radius(p.sigma))
    lib = _lib.load()
    nbytes = lib.cdnet_augment_workspace_bytes(B, size, rmax)
    key = (dev.index, torch.cuda.current_stream().cuda_stream)
    ws = _WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        _WS[key] = ws
    table_dev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
    image = torch.empty((B, 3, size, size), dtype=torch.float32, device=dev)
    weight = torch.empty((B, size, size), dtype=torch.uint8, device=dev)
    label = torch.empty((B, size, size), dtype=torch.int32 if label_i32 else torch.uint8, device=dev)
    varied = torch.empty((B,), dtype=torch.int32, device=dev)
    FS = size + 2 * HALO
    field = torch.zeros((B, 2, FS, FS), dtype=torch.float32, device=dev) if want_field else None
    norm = (C.c_float * 6)(*(list(normalize[0]) + list(normalize[1]))) if normalize else None
    _lib.call('cdnet_augment_batch', _lib.ptr(table_dev), table, B, size, norm, _lib.ptr(ws), ws.numel(), _lib.ptr(image),
              _lib.ptr(weight), _lib.ptr(label), label_i32, _lib.ptr(varied), _lib.ptr(field), _lib.stream_ptr())
    if want_field:
        return image, weight, label, varied, field
    return image, weight, label, varied
