"""Regenerate tests/golden/variance.npz: the reference's instance variance term (loss.py:9-33 LossVariance, fed as train_util_dam.py:174-180
feeds it: F.softmax of the mask logits and measure.label(target == 1) per sample) and its gradient w.r.t. the LOGITS, on hand-built labels.

CONTAINER-ONLY: imports the reference's class from /root/reference (read-only, never copied) through _ref_shims (measure.label restated with
scipy.ndimage, 8-connectivity).  The fixture holds data only.

    python tests/golden/make_golden_variance.py

Every evaluation runs twice through torch.softmax + LossVariance + autograd: in float64 (the truth the device is compared with) and in float32
(the yardstick: the reference's own arithmetic error on the same inputs).

Cases (labels by hand, at the smallest sizes that reach each way the device code can go wrong):
  A   B = 2, K = 3, 48 x 80 (W no multiple of 64, H no multiple of 4).  Sample 0: two pairs of blobs that touch only diagonally (NW-SE and NE-SW;
      one instance each under 8-connectivity), a U whose arms meet below (late union), a blob across the x = 64 segment boundary inside a ring of
      class 2, blobs on the top border and in the bottom-right corner, two blobs separated by one column of class 2 (stay two), one isolated
      pixel (counts in U, contributes nothing), a two-pixel diagonal instance (n - 1 = 1).  Sample 1: all background (loss and gradient 0).
  A2  the labels of A with K = 2 logits.
  B   B = 1, K = 3, 64 x 64: isolated pixels at stride 2, 1024 instances - the worst-case count; loss and gradient exactly 0.
  C   B = 1, K = 3, 256 x 256: one instance over the whole tile, n = 65 536 (the accumulator's range, the longest sums).  Its logits are one
      random 16 x 16 tile repeated 16 x 16 times: the arrays then deflate to a few KB instead of 4.7 MB, which the 1 MiB limit on committed
      files would not take, and n, the sums' length and both precisions' rounding are those of any other 65 536-pixel instance.
Logit scales per case: 's3' = randn * 3 (saturated soft-max), 's005' = randn * 0.05 (near-uniform: variances of 1e-4 against p^2 of 0.1, the
cancellation regime).

Keys: '<case>/label' u8 [B,H,W]; '<case>/root' i32 [B,H,W] (flat index y * W + x of the first pixel, in raster order, of the pixel's instance;
-1 off the mask); '<case>/U' i32 [B]; per scale '<case>/<scale>/logits' f32 [B,K,H,W], '/loss64' f64, '/grad64' f64 [B,K,H,W],
'/eloss32' = |loss32 - loss64| / |loss64| and '/egrad32' = max|grad32 - grad64| / max|grad64| (both 0 where the float64 value is exactly 0
and the float32 one too).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_shims  # noqa: E402

SCALES = {'s3': 3.0, 's005': 0.05}


def labels_a():
    lab = np.zeros((2, 48, 80), np.uint8)
    s = lab[0]
    s[2:6, 2:7] = 1
    s[6:10, 7:12] = 1                                   # touches the first at (5,6)-(6,7) only
    s[36:40, 50:55] = 1
    s[40:44, 45:50] = 1                                 # touches at (39,50)-(40,49) only
    s[12:21, 4:7] = 1
    s[12:21, 12:15] = 1
    s[21:24, 4:15] = 1                                  # the U's bottom joins the arms
    s[9:18, 57:72] = 2
    s[10:17, 58:71] = 1                                 # across x = 64, ringed by class 2
    s[0:2, 30:41] = 1                                   # top border
    s[40:48, 72:80] = 1                                 # bottom-right corner
    s[26:31, 4:9] = 1
    s[26:31, 9] = 2
    s[26:31, 10:15] = 1                                 # two instances: class 2 does not connect them
    s[30, 40] = 1                                       # isolated pixel
    s[34, 20] = 1
    s[35, 21] = 1                                       # two pixels, diagonal
    return lab


def labels_b():
    lab = np.zeros((1, 64, 64), np.uint8)
    lab[0, ::2, ::2] = 1
    return lab


def roots_of(lab, measure):
    root = np.full(lab.shape, -1, np.int32)
    U = np.zeros((lab.shape[0],), np.int32)
    labeled = np.zeros(lab.shape, np.int64)
    for k in range(lab.shape[0]):
        L = measure.label(lab[k] == 1)
        labeled[k] = L
        U[k] = int(L.max())
        flat = L.ravel()
        idx = np.flatnonzero(flat)
        first = np.full((U[k] + 1,), flat.size, np.int64)
        np.minimum.at(first, flat[idx], idx)
        root[k].ravel()[idx] = first[flat[idx]]
    return root, U, labeled


def evaluate(crit, logits, labeled, dtype):
    z = torch.from_numpy(logits).to(dtype).requires_grad_(True)
    loss = crit(torch.softmax(z, dim=1), torch.from_numpy(labeled).to(dtype))
    if not torch.is_tensor(loss):                       # no instance with n > 1 anywhere: the reference returns the number 0
        return float(loss), np.zeros(logits.shape, np.float64)
    loss.backward()
    return float(loss.detach().double()), z.grad.double().numpy()


def main():
    _ref_shims.install()
    from skimage import measure
    from loss import LossVariance
    crit = LossVariance()
    rng = np.random.RandomState(20221)
    out = {}
    cases = [('A', labels_a(), 3, None), ('A2', labels_a(), 2, None), ('B', labels_b(), 3, None),
             ('C', np.ones((1, 256, 256), np.uint8), 3, 16)]
    for name, lab, K, tile in cases:
        root, U, labeled = roots_of(lab, measure)
        out[name + '/label'], out[name + '/root'], out[name + '/U'] = lab, root, U
        B, H, W = lab.shape
        for sname, scale in SCALES.items():
            if tile:
                z = np.tile(rng.standard_normal((B, K, tile, tile)), (1, 1, H // tile, W // tile))
            else:
                z = rng.standard_normal((B, K, H, W))
            logits = (z * scale).astype(np.float32)
            l64, g64 = evaluate(crit, logits, labeled, torch.float64)
            l32, g32 = evaluate(crit, logits, labeled, torch.float32)
            el = abs(l32 - l64) / abs(l64) if l64 != 0 else float(l32 != 0)
            gm = np.abs(g64).max()
            eg = np.abs(g32 - g64).max() / gm if gm != 0 else float(np.abs(g32).max() != 0)
            key = '%s/%s/' % (name, sname)
            out[key + 'logits'], out[key + 'loss64'], out[key + 'grad64'] = logits, np.float64(l64), g64
            out[key + 'eloss32'], out[key + 'egrad32'] = np.float64(el), np.float64(eg)
            print('%-3s %-5s U=%s loss64=%.9e eloss32=%.3e egrad32=%.3e' % (name, sname, U.tolist(), l64, el, eg))
    path = os.path.join(HERE, 'variance.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
