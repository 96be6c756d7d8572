"""Golden outputs of Pillow's bilinear resize for the resize kernels: writes tests/golden/resize.npz.  PIL and numpy only.

  python tests/golden/make_golden_resize.py

Inputs are not stored: `case_input` / `mask_input` build them from a seed with 64-bit integer arithmetic alone (splitmix64), so the tests
rebuild the same bytes on any numpy.  Outputs are Pillow's `Image.resize((ow, oh), Image.BILINEAR)`; for the mask cases `> 127.5` of
Pillow's output on `mask * 255`.  An output of more than FULL_BYTES bytes (white noise does not compress) is stored as its SHA-256
(`sha_<key>`, 32 bytes) instead of `out_<key>`: the tests compare such a case digest to digest, and element by element with the numpy
mirror, which the CPU test holds to the same digest and to live Pillow.
"""
import hashlib
import os

import numpy as np

# (H, W) -> (oh, ow), each for C = 1 and C = 3
KERNEL_CASES = [
    (1, 1, 5, 7),            # single source pixel
    (7, 5, 1, 1),            # everything collapses to one output pixel
    (37, 53, 96, 137),       # upscale, non-integer ratio
    (200, 150, 23, 17),      # downscale, ratio about 8.7: ksize 19 / 21
    (40, 64, 40, 100),       # only the horizontal pass
    (40, 64, 90, 64),        # only the vertical pass
    (40, 64, 40, 64),        # identity
    (130, 257, 259, 515),    # several workgroup tiles, ragged in both axes
    (2000, 16, 8, 16),       # ksize 501: the two-pass form only
]
MASK_CASES = [(61, 83, 120, 170), (61, 83, 31, 40)]
FULL_BYTES = 16384


def _splitmix64(x):
    x = (x + np.uint64(0x9E3779B97F4A7C15))
    z = x
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def noise_u8(n, seed):
    """n seeded bytes: the top byte of splitmix64(seed * 2^32 + index)"""
    with np.errstate(over='ignore'):
        idx = np.arange(n, dtype=np.uint64) + (np.uint64(seed) << np.uint64(32))
        return (_splitmix64(idx) >> np.uint64(56)).astype(np.uint8)


def case_key(H, W, oh, ow, C):
    return '{}x{}_{}x{}_c{}'.format(H, W, oh, ow, C)


def case_seed(H, W, oh, ow, C):
    return (H * 31 + W * 17 + oh * 7 + ow * 3 + C) % 100003 + 1


def case_input(H, W, oh, ow, C):
    """uint8 [H, W] (C = 1) or [H, W, 3]"""
    a = noise_u8(H * W * C, case_seed(H, W, oh, ow, C))
    return a.reshape((H, W) if C == 1 else (H, W, C))


def mask_input(H, W, seed=7):
    """{0, 1} blobs: seeded noise summed over 7 x 7 windows (integers) and cut at the windows' mean level"""
    n = noise_u8((H + 6) * (W + 6), seed).reshape(H + 6, W + 6).astype(np.int64)
    c = np.zeros((H + 7, W + 7), dtype=np.int64)
    c[1:, 1:] = n.cumsum(0).cumsum(1)
    s = c[7:, 7:] - c[:-7, 7:] - c[7:, :-7] + c[:-7, :-7]
    return (s > 49 * 128).astype(np.uint8)


def pillow_resize(a, oh, ow):
    from PIL import Image
    return np.asarray(Image.fromarray(a).resize((ow, oh), Image.BILINEAR))


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def main():
    out = {}
    for (H, W, oh, ow) in KERNEL_CASES:
        for C in (1, 3):
            want = pillow_resize(case_input(H, W, oh, ow, C), oh, ow)
            key = case_key(H, W, oh, ow, C)
            if want.nbytes > FULL_BYTES:
                out['sha_' + key] = sha(want)
            else:
                out['out_' + key] = want
    for (H, W, oh, ow) in MASK_CASES:
        m = mask_input(H, W)
        assert 0.2 < m.mean() < 0.8
        out['mask_' + case_key(H, W, oh, ow, 1)] = np.packbits(pillow_resize(m * np.uint8(255), oh, ow) > 127.5)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'resize.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
