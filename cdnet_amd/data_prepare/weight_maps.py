"""Border weight maps from instance labels: the `<stem>_weight.png` of every training sample, which the losses read as png / 20
(train_util_dam.py:102,171,230,242).  The reference ships no generator for them; this is U-Net's map,

    w = 1 + w0 * exp(-(d1 + d2)^2 / (2 sigma^2))   on background pixels          stored u8 = floor(20 * w)
    w = 1                                          on the pixels of an instance, and where fewer than two instances are in reach

with d1 <= d2 the Euclidean distances to the nearest and the second-nearest distinct instance.  No instance farther than
R = ceil(sigma * sqrt(2 ln(20 w0))) changes a stored byte (`radius`), which bounds the search of both paths.

    weight_map(instances, w0, sigma, device)      one cdnet_weight_map launch (csrc/weight_map.hip); device='cpu': weight_map_host
    weight_map_host(instances, w0, sigma)         the same bytes with numpy / scipy, one EDT per instance on its bounding box grown by R
    instances_of(path)                            the instance map of a label file at full integer width
    make_missing(label_dir, out_dir, ...)         `<out_dir>/<stem>_weight.png` for every `<label_dir>/<stem>_label.{npy,mat,png}`

    python -m cdnet_amd.data_prepare.weight_maps --label-dir D --out-dir O [--w0 10 --sigma 5 --device cpu --overwrite]
"""
import argparse
import os

import numpy as np

LABEL_SUFFIXES = ('_label.npy', '_label.mat', '_label.png')
MAX_RADIUS = 64                                   # csrc/weight_map.hip: the LDS window of a tile must fit the CU


def radius(w0, sigma):
    """R above, from cdnet_weight_map_radius (host code of the library: no GPU needed); ValueError for constants cdnet_weight_map refuses"""
    from .. import _lib
    R = _lib.load().cdnet_weight_map_radius(float(w0), float(sigma))
    if R == 0:
        raise ValueError('weight_map: w0 = {} and sigma = {} must be positive, and 20 * (1 + w0) at most 255'.format(w0, sigma))
    if R > MAX_RADIUS:
        raise ValueError('weight_map: search radius R = {} > {} (w0 = {}, sigma = {})'.format(R, MAX_RADIUS, w0, sigma))
    return R


def _as_map(instances):
    a = instances.detach().cpu().numpy() if hasattr(instances, 'detach') else np.asarray(instances)
    if a.ndim != 2 or a.size == 0:
        raise ValueError('weight_map: an instance map [H, W] is needed, got shape {}'.format(a.shape))
    if a.dtype.kind not in 'iub' or (a.size and (int(a.max()) > 0x7fffffff or int(a.min()) < -0x80000000)):
        raise ValueError('weight_map: integer ids within int32 are needed, got {}'.format(a.dtype))
    return np.ascontiguousarray(a.astype(np.int32))


def weight_map_host(instances, w0=10.0, sigma=5.0):
    """the bytes of `weight_map` with numpy and scipy: a running two-smallest over the instances, each one's EDT taken on its bounding
    box grown by R only (beyond R it changes no byte), so memory stays O(H W)"""
    from scipy import ndimage as ndi
    lab = _as_map(instances)
    R = radius(w0, sigma)
    H, W = lab.shape
    ids, compact = np.unique(np.where(lab > 0, lab, 0), return_inverse=True)
    compact = compact.reshape(H, W).astype(np.int32)
    if ids[0] != 0:                                # no background at all: compact id 0 is an instance
        compact += 1
    d1 = np.full((H, W), np.inf)
    d2 = np.full((H, W), np.inf)
    for k, box in enumerate(ndi.find_objects(compact), start=1):
        if box is None:
            continue
        sl = tuple(slice(max(s.start - R, 0), s.stop + R) for s in box)
        d = ndi.distance_transform_edt(compact[sl] != k)
        a, b = d1[sl], d2[sl]
        nearer = d < a
        b[...] = np.where(nearer, a, np.minimum(b, d))
        a[...] = np.where(nearer, d, a)
    s = d1 + d2
    with np.errstate(over='ignore'):
        w = 20.0 * (1.0 + w0 * np.exp(-(s * s) / (2.0 * sigma * sigma)))
    out = np.floor(w).astype(np.uint8)
    out[(lab > 0) | (d2 > R)] = 20
    return out


def weight_map(instances, w0=10.0, sigma=5.0, device=None):
    """uint8 [H, W] weight map of an instance map (numpy array or torch tensor; ids <= 0 are background).  On the device unless
    device == 'cpu' or, with device None, no GPU is there."""
    import torch
    if device is None:
        device = 'cuda' if torch.cuda.is_available() else 'cpu'
    if torch.device(device).type == 'cpu':
        return weight_map_host(instances, w0, sigma)
    from .. import _lib
    if hasattr(instances, 'detach') and instances.is_cuda and instances.dtype == torch.int32 and instances.dim() == 2 and instances.numel() > 0:
        lab = instances.contiguous()
    else:
        lab = torch.from_numpy(_as_map(instances)).to(device)
    H, W = lab.shape
    out = torch.empty((H, W), dtype=torch.uint8, device=lab.device)
    with torch.cuda.device(lab.device):
        _lib.call('cdnet_weight_map', _lib.ptr(lab), H, W, float(w0), float(sigma), _lib.ptr(out), _lib.stream_ptr())
    return out.cpu().numpy()


def instances_of(path):
    """instance map of a label file at full integer width: a .npy as stored (channel 0 if 3-D), the 'inst_map' of a .mat, a 3-class
    `_label.png` through the rule of test_dam.ground_truth_instances (8-connected components of channel 0 > 127, grown by disk(1)).
    Not through data_folder.img_loader, which casts ids to uint8."""
    if path.endswith('.npy'):
        a = np.load(path)
        return a[:, :, 0] if a.ndim == 3 else a
    if path.endswith('.mat'):
        import scipy.io as scio
        return scio.loadmat(path)['inst_map']
    from PIL import Image
    from scipy import ndimage as ndi
    lab = np.asarray(Image.open(path))
    inside = (lab if lab.ndim == 2 else lab[:, :, 0]) > 127
    cc, _ = ndi.label(inside, structure=np.ones((3, 3), int))
    disk1 = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)
    return ndi.grey_dilation(cc, footprint=disk1).astype(np.int32)


def label_files(label_dir):
    """[(stem, path)] of the `<stem>_label.{npy,mat,png}` files of a directory, sorted; .npy before .mat before .png for one stem"""
    found = {}
    for name in sorted(os.listdir(label_dir)):
        for rank, suffix in enumerate(LABEL_SUFFIXES):
            if name.endswith(suffix):
                stem = name[:-len(suffix)]
                if stem not in found or rank < found[stem][0]:
                    found[stem] = (rank, os.path.join(label_dir, name))
    return [(stem, found[stem][1]) for stem in sorted(found)]


def make_missing(label_dir, out_dir, w0=10.0, sigma=5.0, device=None, overwrite=False, report=None):
    """write `<out_dir>/<stem>_weight.png` (mode L) for every label file of `label_dir` that has none yet (all of them with
    `overwrite`); `report(stem, path, written, max byte)` per image.  Returns (written, skipped)."""
    from PIL import Image
    radius(w0, sigma)
    os.makedirs(out_dir, exist_ok=True)
    written = skipped = 0
    for stem, path in label_files(label_dir):
        dst = os.path.join(out_dir, stem + '_weight.png')
        if os.path.exists(dst) and not overwrite:
            skipped += 1
            if report is not None:
                report(stem, dst, False, None)
            continue
        w = weight_map(instances_of(path), w0, sigma, device)
        Image.fromarray(w).save(dst)                  # uint8 [H, W]: mode L
        written += 1
        if report is not None:
            report(stem, dst, True, int(w.max()))
    return written, skipped


def main(argv=None):
    ap = argparse.ArgumentParser(description='border weight maps (<stem>_weight.png) from instance labels')
    ap.add_argument('--label-dir', required=True, help='directory of <stem>_label.npy / .mat (instance maps) or .png (3-class labels)')
    ap.add_argument('--out-dir', required=True)
    ap.add_argument('--w0', type=float, default=10.0)
    ap.add_argument('--sigma', type=float, default=5.0)
    ap.add_argument('--device', default=None, help="'cpu' for the numpy / scipy path; default: the GPU when there is one")
    ap.add_argument('--overwrite', action='store_true')
    a = ap.parse_args(argv)

    def report(stem, path, made, top):
        print('{:s}: {:s}'.format(path, 'written, max {:d}'.format(top) if made else 'exists, skipped'))
    written, skipped = make_missing(a.label_dir, a.out_dir, a.w0, a.sigma, a.device, a.overwrite, report)
    print('{:d} weight maps written, {:d} skipped'.format(written, skipped))
    return written, skipped


if __name__ == '__main__':
    main()
