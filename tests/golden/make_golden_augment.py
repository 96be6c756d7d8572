"""Regenerate tests/golden/augment.npz: Pillow's colour chain (ImageEnhance Color -> Brightness -> Contrast -> Sharpness) and the
three random_chooseAug filters (BLUR, GaussianBlur(2), MedianFilter(3)) on small RGB sources of odd sizes.  PIL only.

    python tests/golden/make_golden_augment.py
"""
import os

import numpy as np
import PIL
from PIL import Image, ImageEnhance, ImageFilter

SIZES = ((61, 77), (96, 96), (118, 113))
FACTORS = ((0.5, 0.5, 0.5, 0.5), (1.4999999, 1.4999999, 1.4999999, 1.4999999), (0.73, 1.31, 0.52, 1.44))
FILTERS = (ImageFilter.BLUR, ImageFilter.GaussianBlur, ImageFilter.MedianFilter)


def main():
    rs = np.random.RandomState(2024)
    out = {'pillow_version': np.array(PIL.__version__), 'factors': np.array(FACTORS, np.float32)}
    for k, (H, W) in enumerate(SIZES):
        # smooth structure plus noise, so that the filters and the contrast mean are exercised away from saturation
        yy, xx = np.mgrid[0:H, 0:W]
        base = 128 + 90 * np.sin(yy[..., None] / (5.0 + np.arange(3)) + xx[..., None] / 7.0)
        img = np.clip(base + rs.randint(-12, 13, size=(H, W, 3)), 0, 255).astype(np.uint8)
        out['src%d' % k] = img
        chains = []
        for f in FACTORS:
            im = Image.fromarray(img)
            for enh, v in zip((ImageEnhance.Color, ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Sharpness), f):
                im = enh(im).enhance(float(np.float32(v)))
            chains.append(np.asarray(im))
        out['chain%d' % k] = np.stack(chains)
        out['filt%d' % k] = np.stack([np.asarray(Image.fromarray(img).filter(f)) for f in FILTERS])
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'augment.npz'), **out)


if __name__ == '__main__':
    main()
