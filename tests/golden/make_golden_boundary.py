"""Regenerate tests/golden/boundary.npz: the reference's boundary-switch terms (loss.py:331-393 BoundaryLoss, :37-78 FocalLoss2d, :81-127
RobustFocalLoss2d, fed as train_util_dam.py:195-205 feeds them: the mask logits and the three-channel one-hot target) and their gradients
w.r.t. the logits, on hand-built labels.

CONTAINER-ONLY: imports the reference's classes from /root/reference (read-only, never copied) through _ref_shims.  The fixture holds data only.

    python tests/golden/make_golden_boundary.py

Every evaluation runs twice through the reference class + autograd: in float64 (the truth the device is compared with) and in float32 (the
yardstick: the reference's own arithmetic error on the same inputs).  The one-hot target is [label == c] for c = 0, 1, 2 (the reference's
np.unique-over-the-batch construction, which shifts channels when a batch lacks a class, is not reproduced).

Cases (labels by hand; the device code works on 32 x 32 tiles with a 6-pixel halo):
  A   B = 2, K = 3, 40 x 72 (neither side a multiple of 32, more than one tile both ways).  Sample 0: a nucleus of class 1 ringed by class 2;
      one such structure across each internal tile edge (x = 32, x = 64, y = 32) and one across the tile corner (32, 32); a blob on the top
      border and a ringed one in the bottom-right corner (pooling windows clipped to the image); a one-pixel-wide line; an isolated pixel; two
      blobs two pixels apart (their extended boundaries overlap).  Sample 1: all background (contributes exactly 1 per class, gradient 0).
  B   B = 1, 13 x 13: smaller than twice the halo - every pixel is a border case.
  C   B = 1, 256 x 256: a 16-periodic grid of ringed nuclei; the logits are one random 16 x 16 tile repeated (the period exceeds both
      windows, the arrays deflate to a few KB): the longest sums.
  T   B = 1, 24 x 40, logits constant on 4 x 4 blocks: the 3x3 minimum and the 5x5 maximum tie exactly in both precisions, which pins the
      first-in-raster-order rule of the pools' gradients.
  S   focal only, B = 1, 40 x 72 (sample 0 of A), logits randn * 12: the sigmoid saturates.  float64 is NOT the truth here (float32's clamp bound
      1 - 1e-8 is 1 and 1 - sigmoid is 0 from z = 17 on: the two precisions differ by parts in a thousand); the fixture stores the reference's
      FLOAT32 loss.
Logit scales of A, B, C, T: 's3' = randn * 3, 's005' = randn * 0.05.

A boundary case is committed only if the float32 and the float64 evaluation choose the same arg-max position at every pixel of both pools
(indices of F.max_pool2d(..., return_indices=True) on the reference's own operands); a flipped near-tie is no arithmetic error and would make
the yardstick meaningless, so another seed is drawn.  The robust focal form is asserted bitwise equal to the plain one and not stored.

Keys: '<case>/label' u8 [B,H,W]; per scale '<case>/<scale>/logits' f32 [B,3,H,W]; per kind k in (1, 2) '<case>/<scale>/k<k>/loss64' f64,
'/grad64' f64 [B,3,H,W], '/eloss32' = |loss32 - loss64| / |loss64|, '/egrad32' = max|grad32 - grad64| / max|grad64|;
'S/s12/logits', 'S/s12/k2/loss32' f32.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_shims  # noqa: E402

SCALES = {'s3': 3.0, 's005': 0.05}


def ringed(s, y0, y1, x0, x1):
    s[y0:y1, x0:x1] = 2
    s[y0 + 2:y1 - 2, x0 + 2:x1 - 2] = 1


def labels_a():
    lab = np.zeros((2, 40, 72), np.uint8)
    s = lab[0]
    ringed(s, 4, 13, 4, 15)
    ringed(s, 10, 20, 26, 40)                           # across x = 32
    ringed(s, 27, 37, 8, 18)                            # across y = 32
    ringed(s, 14, 24, 58, 70)                           # across x = 64
    ringed(s, 28, 37, 27, 38)                           # across the corner (32, 32)
    s[0:3, 44:52] = 1                                   # top border
    s[34:40, 64:72] = 2
    s[36:40, 66:72] = 1                                 # bottom-right corner
    s[22, 40:52] = 1                                    # one-pixel-wide line
    s[26, 22] = 1                                       # isolated pixel
    s[3:8, 20:24] = 1
    s[3:8, 26:30] = 1                                   # two pixels apart
    return lab


def labels_b():
    lab = np.zeros((1, 13, 13), np.uint8)
    ringed(lab[0], 3, 10, 3, 10)
    lab[0, 0, 0] = 1
    lab[0, 12, 6:9] = 1
    return lab


def labels_c():
    cell = np.zeros((16, 16), np.uint8)
    ringed(cell, 3, 12, 3, 12)
    return np.tile(cell, (16, 16))[None]


def labels_t():
    lab = np.zeros((1, 24, 40), np.uint8)
    ringed(lab[0], 4, 14, 6, 20)
    lab[0, 16:22, 26:36] = 1                            # across x = 32
    return lab


def one_hot(lab, dtype):
    return torch.from_numpy(np.stack([(lab == c) for c in range(3)], 1)).to(dtype)


def evaluate(crit, logits, lab, dtype):
    z = torch.from_numpy(logits).to(dtype).requires_grad_(True)
    loss = crit(z, one_hot(lab, dtype))
    loss.backward()
    return loss.detach(), z.grad.double().numpy()


def pool_indices(logits, dtype):
    """arg-max positions of the reference's two pools over the prediction (loss.py:369-375), on its own operands"""
    p = torch.softmax(torch.from_numpy(logits).to(dtype), dim=1)
    m, i3 = F.max_pool2d(1 - p, kernel_size=3, stride=1, padding=1, return_indices=True)
    b = m - (1 - p)
    _, i5 = F.max_pool2d(b, kernel_size=5, stride=1, padding=2, return_indices=True)
    return i3.numpy(), i5.numpy()


def flips(logits):
    a3, a5 = pool_indices(logits, torch.float64)
    b3, b5 = pool_indices(logits, torch.float32)
    return int((a3 != b3).sum()), int((a5 != b5).sum())


def draw(rng, shape, scale, tile, block):
    B, K, H, W = shape
    if tile:
        z = np.tile(rng.standard_normal((B, K, tile, tile)), (1, 1, H // tile, W // tile))
    elif block:
        z = np.repeat(np.repeat(rng.standard_normal((B, K, H // block, W // block)), block, 2), block, 3)
    else:
        z = rng.standard_normal(shape)
    return (z * scale).astype(np.float32)


def main():
    _ref_shims.install()
    from loss import BoundaryLoss, FocalLoss2d, RobustFocalLoss2d
    crits = {1: BoundaryLoss(), 2: FocalLoss2d(), 3: RobustFocalLoss2d()}
    out = {}
    cases = [('A', labels_a(), None, None), ('B', labels_b(), None, None), ('C', labels_c(), 16, None), ('T', labels_t(), None, 4)]
    seed = 20222
    for name, lab, tile, block in cases:
        out[name + '/label'] = lab
        B, H, W = lab.shape
        for sname, scale in SCALES.items():
            while True:
                logits = draw(np.random.RandomState(seed), (B, 3, H, W), scale, tile, block)
                f3, f5 = flips(logits)
                seed += 1
                if f3 == 0 and f5 == 0:
                    break
                print('%s %s: seed %d flips %d (3x3) / %d (5x5) arg-max positions between float32 and float64: redrawn' % (name, sname, seed - 1, f3, f5))
            key = '%s/%s/' % (name, sname)
            out[key + 'logits'] = logits
            res = {}
            for k, crit in crits.items():
                l64, g64 = evaluate(crit, logits, lab, torch.float64)
                l32, g32 = evaluate(crit, logits, lab, torch.float32)
                res[k] = (l32, g32)
                l64 = float(l64)
                el = abs(float(l32.double()) - l64) / abs(l64)
                eg = np.abs(g32 - g64).max() / np.abs(g64).max()
                print('%-2s %-5s kind %d seed %d loss64=%.9e eloss32=%.3e egrad32=%.3e' % (name, sname, k, seed - 1, l64, el, eg))
                if k == 3:
                    continue
                kk = key + 'k%d/' % k
                out[kk + 'loss64'], out[kk + 'grad64'] = np.float64(l64), g64
                out[kk + 'eloss32'], out[kk + 'egrad32'] = np.float64(el), np.float64(eg)
            assert torch.equal(res[2][0], res[3][0]) and np.array_equal(res[2][1], res[3][1]), 'robust focal differs from focal'
    lab = labels_a()[:1]
    logits = draw(np.random.RandomState(seed), (1, 3) + lab.shape[1:], 12.0, None, None)
    l32, g32 = evaluate(crits[2], logits, lab, torch.float32)
    l64, _ = evaluate(crits[2], logits, lab, torch.float64)
    r32, h32 = evaluate(crits[3], logits, lab, torch.float32)
    assert torch.equal(l32, r32) and np.array_equal(g32, h32) and np.isfinite(g32).all()
    print('S  s12   kind 2 seed %d loss32=%.9e  (float64: %.9e, relative difference %.3e)' % (seed, float(l32), float(l64), abs(float(l32) - float(l64)) / float(l64)))
    out['S/label'], out['S/s12/logits'], out['S/s12/k2/loss32'] = lab, logits, np.float32(float(l32))
    path = os.path.join(HERE, 'boundary.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
