"""Training augmentation of the reference's recipe (my_transforms_direction.py:69-540), on the device.

  draw_params(rs, H, W, recipe)       one sample's parameters, drawn from the loader's RandomState in the reference's order
  augment_batch(sources, params, ...) one batch on the device: cdnet_augment_batch (csrc/augment.hip)
  augment_host(img, weight, label, p, size, field=None)
                                      the same sample on the host: PIL for the colour chain and the filters, numpy for the
                                      restated OpenCV geometry; it serves TileBatches(device='cpu') and checks the device path
  Recipe                              which steps run, the elastic parameters (alpha, sigma, alpha_affine) and the crop size

Grey-scale sources (img u8 [H, W], Pillow's mode L) take the same three functions: cdnet_augment_batch_c / cdnet_augment_batch_geo_c with
channels = 1.  The parameters are drawn alike for both channel counts; on L the Color factor is drawn and ignored (Pillow's Color of an L
image is the identity).

Per sample, on the whole source image, in the order options.py:331-347 fixes: [random_resize] -> random_color -> [random_affine] ->
horizontal / vertical flip -> random_elastic (random affine, then a Gaussian-smoothed displacement field) -> [random_rotation] ->
random_chooseAug -> random_crop; the bracketed steps are off in the default recipe and go through cdnet_augment_batch_geo.  The contract is the same distributions and the same operation
for given parameters, not the reference's random streams (Python `random`, np.random and albumentations' RandomState spread over
DataLoader workers).  The colour chain, the filters and random_affine equal Pillow's bit for bit; the other geometry (elastic, resize,
rotation) restates OpenCV 4's nearest rules (cv2 / albumentations parity unpinned); the field noise is a counter-based hash of (seed, plane, y, x), not numpy's MT19937.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import AugGeo, AugSample

HALO = 6                                   # the field window: crop + 6 px on every side (csrc/augment.hip)


GEO_RESIZE, GEO_AFFINE, GEO_ROTATION = 1, 2, 4


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
    resize: tuple = None            # random_resize: None or (lb, ub), the scale's range (my_transforms_direction.py:95)
    affine: float = None            # random_affine: None or the bound of the four coefficients' deviations (:195-199: inside [0, 0.5])
    rotation: bool = False          # random_rotation: the reference ignores its `degrees` and always runs albu.Rotate(limit=(-90, 90)) (:417)
    rotation_limit: float = 90.0

    def __post_init__(self):
        if self.affine is not None and not 0 <= self.affine <= 0.5:
            raise ValueError('Bound is invalid, should be in range [0, 0.5)')
        if self.resize is not None:
            self.resize = (float(self.resize[0]), float(self.resize[1]))
            if not 0 < self.resize[0] <= self.resize[1]:
                raise ValueError('random_resize needs 0 < lb <= ub')

    @classmethod
    def from_transform(cls, transform, **elastic):
        rr, ra = transform.get('random_resize'), transform.get('random_affine')
        return cls(size=int(transform['random_crop']), color=bool(transform.get('random_color')),
                   hflip=bool(transform.get('horizontal_flip')), vflip=bool(transform.get('vertical_flip')),
                   elastic=bool(transform.get('random_elastic')), choose_aug=bool(transform.get('random_chooseAug')),
                   resize=tuple(rr) if rr else None, affine=float(ra) if ra is not None and ra is not False else None,
                   rotation=bool(transform.get('random_rotation')), **elastic)


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
    # the optional steps; the defaults mean "off"
    scale: float = 1.0          # random_resize's scale
    Hr: int = 0                 # the resized size (0: the source's)
    Wr: int = 0
    paff: tuple = None          # random_affine: Pillow's (a, b, c, d, e, f), output -> input pixel
    angle: float = 0.0          # random_rotation's angle in degrees (counter-clockwise)
    rinv: tuple = None          # its inverse matrix (2 x 3 row-major, float64): destination -> source pixel
    fy0: int = None             # the displacement-field window's origin and edge (None: crop + 6 px at (y0 - 6, x0 - 6))
    fx0: int = None
    fedge: int = None

    def dims(self, H, W):
        """the size every step after random_resize works in"""
        return (self.Hr or H, self.Wr or W)


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
    return invert_affine(np.linalg.solve(A, rhs))


def invert_affine(M):
    """OpenCV's invertAffineTransform formula on M (6 doubles, row-major 2 x 3)"""
    D = M[0] * M[4] - M[1] * M[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22, A12, A21 = M[4] * D, M[0] * D, -M[1] * D, -M[3] * D
    b1 = -A11 * M[2] - A12 * M[5]
    b2 = -A21 * M[2] - A22 * M[5]
    return (A11, A12, b1, A21, A22, b2)


IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def rotation_inverse(angle, H, W):
    """the inverse of OpenCV's getRotationMatrix2D((W / 2, H / 2), angle, 1) - the centre albumentations' Rotate passed in the
    reference's era (later versions use W / 2 - 0.5; parity unpinned)"""
    t = angle * np.pi / 180.0
    al, be = float(np.cos(t)), float(np.sin(t))
    cx, cy = W / 2.0, H / 2.0
    return invert_affine((al, be, (1 - al) * cx - be * cy, -be, al, be * cx + (1 - al) * cy))


def resize_dims(H, W, scale):
    """RandomResize's output size (my_transforms_direction.py:99-100)"""
    return int(H * scale), int(W * scale)


def resize_index(n_out, n_in):
    """OpenCV INTER_NEAREST: the source index behind each of n_out output rows / columns"""
    return np.minimum(np.floor(np.arange(n_out) * (1.0 / (n_out / n_in))).astype(np.int64), n_in - 1)


def pil_affine_source(paff, H, W, y, x):
    """Pillow's Image.transform(AFFINE, NEAREST) in its 16.16 fixed point (Geometry.c affine_fixed), restated: -> (yin, xin, inside)
    of output pixels (y, x) of an H x W image"""
    a = [float(v) for v in paff]
    fix = lambda v: int(np.floor(v * 65536.0 + 0.5))
    a0, a1, a3, a4 = fix(a[0]), fix(a[1]), fix(a[3]), fix(a[4])
    a2, a5 = fix(a[2] + (a[0] * 0.5 + a[1] * 0.5)), fix(a[5] + (a[3] * 0.5 + a[4] * 0.5))
    y, x = np.asarray(y, np.int64), np.asarray(x, np.int64)
    xin = (a2 + a1 * y + a0 * x) >> 16
    yin = (a5 + a4 * y + a3 * x) >> 16
    return yin, xin, (xin >= 0) & (xin < W) & (yin >= 0) & (yin < H)


def field_box(p, H, W, size):
    """the displacement-field window a sample needs in a batch that holds a rotation: the bounding box of the four corners of the crop +
    6 px, mapped through the rotation's inverse by the kernel's fixed-point rule (monotone in each coordinate, so the corners bound
    every pixel), + 2 px, clipped to the H x W image -> (fy0, fx0, edge)"""
    ys = np.array([p.y0 - HALO, p.y0 - HALO, p.y0 + size + HALO - 1, p.y0 + size + HALO - 1])
    xs = np.array([p.x0 - HALO, p.x0 + size + HALO - 1, p.x0 - HALO, p.x0 + size + HALO - 1])
    if p.rinv is not None:
        ys, xs, _ = warp_source(p.rinv, H, W, ys, xs)
    ylo, yhi = max(int(ys.min()) - 2, 0), min(int(ys.max()) + 2, H - 1)
    xlo, xhi = max(int(xs.min()) - 2, 0), min(int(xs.max()) + 2, W - 1)
    if yhi < ylo or xhi < xlo:                   # wholly outside the image: nothing is read
        return 0, 0, 1
    return ylo, xlo, max(yhi - ylo, xhi - xlo) + 1


def draw_params(rs, H, W, recipe):
    """the reference's draws in its order (RandomResize :95, RandomColor :162-172, RandomAffine :205-208, flips :233 / :251,
    ElasticTransform's affine offsets and field, RandomRotation / albu.Rotate's angle, RandomChooseAug :451, RandomCrop): `rs` is the
    loader's numpy RandomState.  With random_resize every later step is drawn for the resized size."""
    geo = {}
    if recipe.resize is not None:
        scale = float(rs.uniform(*recipe.resize))
        H, W = resize_dims(H, W, scale)
        if H < 1 or W < 1:
            raise ValueError('random_resize: the scale {} leaves no pixel'.format(scale))
        geo.update(scale=scale, Hr=H, Wr=W)
    color = tuple(1 + (rs.rand() - 0.5) for _ in range(4)) if recipe.color else (1.0, 1.0, 1.0, 1.0)
    if recipe.affine is not None:
        v = recipe.affine
        a = 1 + 2 * v * (rs.rand() - 0.5)
        b = 2 * v * (rs.rand() - 0.5)
        d = 2 * v * (rs.rand() - 0.5)
        e = 1 + 2 * v * (rs.rand() - 0.5)
        # :211-212: the transformation centre is the image centre (x = width, y = height)
        c = -a * W / 2 - b * H / 2 + W / 2
        f = -d * W / 2 - e * H / 2 + H / 2
        geo['paff'] = tuple(float(t) for t in (a, b, c, d, e, f))
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
    if recipe.rotation:
        angle = float(rs.uniform(-recipe.rotation_limit, recipe.rotation_limit))
        geo.update(angle=angle, rinv=tuple(float(t) for t in rotation_inverse(angle, H, W)))
    filt = 0
    if recipe.choose_aug:
        r = rs.rand()
        filt = 1 if r < 0.25 else 2 if r < 0.5 else 3 if r < 0.75 else 0
    s = recipe.size
    y0 = int(rs.randint(0, max(H - s, 0) + 1))
    x0 = int(rs.randint(0, max(W - s, 0) + 1))
    p = Params(color, hflip, vflip, tuple(float(v) for v in minv), alpha, float(recipe.elastic_sigma), seed, filt, y0, x0, **geo)
    if p.rinv is not None:
        p.fy0, p.fx0, p.fedge = field_box(p, H, W, s)
    return p


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
    """random_color (my_transforms_direction.py:161-179) with given factors, through PIL itself (img u8 [H, W, 3], or [H, W]: mode L)"""
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


def field_full(p, H, W):
    """dx, dy (f32 [2, H, W]) over the whole image as the host computes them (field_window's rule)"""
    from scipy.ndimage import gaussian_filter
    return np.stack([gaussian_filter(field_noise(p.seed, k, H, W), p.sigma, mode='reflect', truncate=4.0) * np.float32(p.alpha)
                     for k in range(2)])


def _gather(planes, Y, X, ok):
    Yc, Xc = np.where(ok, Y, 0), np.where(ok, X, 0)
    return [np.where(ok if a.ndim == 2 else ok[..., None], a[Yc, Xc], 0).astype(a.dtype) for a in planes]


def augment_host(img, weight, label, p, size, field=None, origin=None):
    """one sample through the whole chain on the host.  img u8 [H, W, 3] or [H, W] (mode L), weight u8 [H, W], label u8 / i32 [H, W]; `field` (f32 [2, E, E],
    as augment_batch returns it) replaces the host's own dx, dy when given, `origin` = the (row, column) of its first element in the
    (resized) image (default: the crop origin - 6, the window without a rotation).  Returns the crop (img u8 [s, s, 3] or [s, s], weight u8 [s, s],
    label [s, s]) before the division by 255."""
    planes = [img, weight, label]
    if p.Hr:                                     # random_resize: OpenCV's nearest index rule
        iy, ix = resize_index(p.Hr, weight.shape[0]), resize_index(p.Wr, weight.shape[1])
        planes = [a[iy][:, ix] for a in planes]
    H, W = planes[1].shape
    im = colour_chain(planes[0], p.color)
    nc = 1 if im.ndim == 2 else 3
    planes = ([im] if nc == 1 else [im[..., c] for c in range(3)]) + planes[1:]
    if p.paff is not None:                       # random_affine: through PIL itself, per plane (my_transforms_direction.py:216-218)
        from PIL import Image
        rgb = Image.fromarray(np.ascontiguousarray(im)).transform((W, H), Image.AFFINE, p.paff)
        rest = [np.asarray(Image.fromarray(np.ascontiguousarray(a)).transform((W, H), Image.AFFINE, p.paff)).astype(a.dtype)
                for a in planes[nc:]]
        rgb = np.asarray(rgb)
        planes = ([rgb] if nc == 1 else [rgb[..., c] for c in range(3)]) + rest
    if p.hflip:
        planes = [a[:, ::-1] for a in planes]
    if p.vflip:
        planes = [a[::-1] for a in planes]
    # elastic: q -> r = round(q + d(q)) (remap) -> s = M^-1 r (warpAffine); anything outside reads 0 in every plane
    qy, qx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    ry, rx, inside = qy, qx, np.ones((H, W), bool)
    if p.alpha != 0.0:
        if field is None:
            d = field_full(p, H, W)
        else:
            d = np.zeros((2, H, W), np.float32)
            fy0, fx0 = origin if origin is not None else (p.y0 - HALO, p.x0 - HALO)
            FS = np.asarray(field[0]).shape[0]
            ys, xs = np.arange(fy0, fy0 + FS), np.arange(fx0, fx0 + FS)
            iy, ix = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
            for k in range(2):
                d[k][np.ix_(ys[iy], xs[ix])] = np.asarray(field[k], np.float32)[np.ix_(iy, ix)]
        rx = np.rint(qx.astype(np.float32) + d[0]).astype(np.int64)
        ry = np.rint(qy.astype(np.float32) + d[1]).astype(np.int64)
        inside = (rx >= 0) & (rx < W) & (ry >= 0) & (ry < H)
    Y, X, ok = warp_source(p.minv, H, W, ry, rx)
    warped = _gather(planes, Y, X, ok & inside)
    if p.rinv is not None:                       # random_rotation: warpAffine nearest, zero border
        warped = _gather(warped, *warp_source(p.rinv, H, W, qy, qx))
    im = apply_filter(warped[0] if nc == 1 else np.stack(warped[:3], -1), p.filter)
    s = size
    out = [im, warped[nc], warped[nc + 1]]
    out = [a[p.y0:p.y0 + s, p.x0:p.x0 + s] for a in out]
    if out[1].shape != (s, s):
        out = [np.pad(a, ((0, s - a.shape[0]), (0, s - a.shape[1])) + ((0, 0),) * (a.ndim - 2)) for a in out]
    return [np.ascontiguousarray(a) for a in out]


# ---------------------------------------------------------------------------------------------------- device path

class Source:
    """one source image resident on the device: img u8 [H, W, 3] or [H, W] (mode L), weight u8 [H, W], label u8 [H, W] (channel 0) or i32 [H, W]"""

    def __init__(self, img, weight, label, dev):
        self.H, self.W = weight.shape[:2]
        img = np.array(img, dtype=np.uint8, order='C')                                         # (a copy: PIL arrays are read-only)
        if not (img.shape == (self.H, self.W) or img.shape == (self.H, self.W, 3)):
            raise ValueError('Source: img is u8 [H, W, 3] or [H, W] of the weight map\'s size {} x {}, got {}'.format(self.H, self.W, img.shape))
        self.channels = 1 if img.ndim == 2 else 3
        self.img = torch.from_numpy(img).to(dev)
        self.weight = torch.from_numpy(np.array(weight if weight.ndim == 2 else weight[:, :, 0], dtype=np.uint8, order='C')).to(dev)
        lab = label if label.ndim == 2 else label[:, :, 0]
        self.label_i32 = lab.dtype != np.uint8
        self.label = torch.from_numpy(np.array(lab, dtype=np.int32 if self.label_i32 else np.uint8, order='C')).to(dev)


_WS = {}


def _geo_table(sources, params, size):
    """(AugGeo table, field edge) of a batch that needs cdnet_augment_batch_geo, else (None, size + 12).  With a rotation in the batch
    every sample's field window is its field_box and the edge is the largest; else the windows are the crop + 6 px."""
    if not any(p.Hr or p.paff is not None or p.rinv is not None for p in params):
        return None, size + 2 * HALO
    rot = any(p.rinv is not None for p in params)
    geo = (AugGeo * len(params))()
    edge = 1 if rot else size + 2 * HALO
    for g, src, p in zip(geo, sources, params):
        g.Hr, g.Wr = p.dims(src.H, src.W)
        g.flags = (GEO_RESIZE if p.Hr else 0) | (GEO_AFFINE if p.paff is not None else 0) | (GEO_ROTATION if p.rinv is not None else 0)
        g.paff[:] = p.paff if p.paff is not None else IDENTITY
        g.rinv[:] = p.rinv if p.rinv is not None else IDENTITY
        g.fy0, g.fx0 = p.y0 - HALO, p.x0 - HALO
        if rot:
            box = (p.fy0, p.fx0, p.fedge) if p.fedge is not None else field_box(p, g.Hr, g.Wr, size)
            g.fy0, g.fx0 = box[0], box[1]
            edge = max(edge, box[2])
    return geo, edge


def augment_batch(sources, params, size, normalize=None, want_field=False, want_origin=False):
    """the batch on the device (one call of cdnet_augment_batch, or of cdnet_augment_batch_geo when a sample has one of the optional
    steps; csrc/augment.hip).  sources: [Source], params: [Params].
    Sources of mode L ([H, W] images, all of the batch alike) go through the same calls' `_c` forms with channels = 1.
    Returns (image f32 [B, 3, s, s] ([B, 1, s, s] on L; `normalize` then gives one mean and one std, or more of which the first is read), weight u8 [B, s, s], label u8 / i32 [B, s, s], varied i32 [B][, field f32 [B, 2, E, E]][, origin
    i64 [B, 2]]); varied[b] == 0: the label crop holds one value (re-draw).  The field window's edge E is s + 12 and its origin (y0 - 6,
    x0 - 6) unless the batch holds a rotation.  want_field keeps its five values; the origins, each sample's (row, column), are a
    separate request (want_origin) so that earlier callers of want_field stay as they are."""
    B = len(sources)
    assert B == len(params) and B > 0
    dev = sources[0].img.device
    label_i32 = int(sources[0].label_i32)
    nc = sources[0].channels
    if any(src.channels != nc for src in sources):
        raise ValueError('augment_batch: RGB and L sources in one batch')
    table = (AugSample * B)()
    rmax = 0
    for t, src, p in zip(table, sources, params):
        t.minv[:] = p.minv
        t.img, t.weight, t.label = src.img.data_ptr(), src.weight.data_ptr(), src.label.data_ptr()
        t.H, t.W, t.img_stride, t.weight_stride, t.label_stride, t.label_i32 = src.H, src.W, nc * src.W, src.W, src.W, int(src.label_i32)
        t.color[:] = p.color
        t.hflip, t.vflip, t.filter, t.y0, t.x0 = p.hflip, p.vflip, p.filter, p.y0, p.x0
        t.alpha, t.sigma, t.seed = p.alpha, p.sigma, p.seed
        if p.alpha != 0.0:
            rmax = max(rmax, gauss_radius(p.sigma))
    geo, FS = _geo_table(sources, params, size)
    lib = _lib.load()
    nbytes = lib.cdnet_augment_geo_workspace_bytes(B, size, rmax, FS)
    key = (dev.index, torch.cuda.current_stream().cuda_stream)
    ws = _WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        _WS[key] = ws
    table_dev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
    image = torch.empty((B, nc, size, size), dtype=torch.float32, device=dev)
    weight = torch.empty((B, size, size), dtype=torch.uint8, device=dev)
    label = torch.empty((B, size, size), dtype=torch.int32 if label_i32 else torch.uint8, device=dev)
    varied = torch.empty((B,), dtype=torch.int32, device=dev)
    field = torch.zeros((B, 2, FS, FS), dtype=torch.float32, device=dev) if want_field else None
    norm = (C.c_float * (2 * nc))(*(list(normalize[0])[:nc] + list(normalize[1])[:nc])) if normalize else None
    grey = () if nc == 3 else (nc,)                 # RGB keeps the calls it always made
    suffix = '_c' if grey else ''
    if geo is None:
        _lib.call('cdnet_augment_batch' + suffix, _lib.ptr(table_dev), table, B, size, norm, _lib.ptr(ws), ws.numel(), _lib.ptr(image),
                  _lib.ptr(weight), _lib.ptr(label), label_i32, _lib.ptr(varied), _lib.ptr(field), _lib.stream_ptr(), *grey)
        origin = np.array([(p.y0 - HALO, p.x0 - HALO) for p in params], np.int64)
    else:
        geo_dev = torch.frombuffer(bytearray(bytes(geo)), dtype=torch.uint8).to(dev)
        _lib.call('cdnet_augment_batch_geo' + suffix, _lib.ptr(table_dev), table, _lib.ptr(geo_dev), geo, FS, B, size, norm, _lib.ptr(ws), ws.numel(),
                  _lib.ptr(image), _lib.ptr(weight), _lib.ptr(label), label_i32, _lib.ptr(varied), _lib.ptr(field), _lib.stream_ptr(), *grey)
        origin = np.array([(g.fy0, g.fx0) for g in geo], np.int64)
    out = (image, weight, label, varied) + ((field,) if want_field else ()) + ((origin,) if want_origin else ())
    return out
