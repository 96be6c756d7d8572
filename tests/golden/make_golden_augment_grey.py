"""Regenerate tests/golden/augment_grey.npz: Pillow's colour chain (ImageEnhance Color -> Brightness -> Contrast -> Sharpness) and the
three random_chooseAug filters (BLUR, GaussianBlur(2), MedianFilter(3)) on small mode-L sources of odd sizes.  PIL only.

    python tests/golden/make_golden_augment_grey.py

`chain<k>[j]` is source k through FACTORS[j]; `colour<k>[i]` is source k through ImageEnhance.Color alone with COLOR_ONLY[i] (the identity
on an L image); `filt<k>[c - 1]` is filter code c.
"""
import os

import numpy as np
import PIL
from PIL import Image, ImageEnhance, ImageFilter

SIZES = ((37, 45), (48, 56), (33, 40))
FACTORS = ((0.5, 0.5, 0.5, 0.5), (1.4999999, 1.4999999, 1.4999999, 1.4999999), (0.73, 1.31, 0.52, 1.44), (1.5, 0.8, 1.37, 0.61))
COLOR_ONLY = (0.5, 1.5)
FILTERS = (ImageFilter.BLUR, ImageFilter.GaussianBlur, ImageFilter.MedianFilter)


def main():
    rs = np.random.RandomState(2039)
    out = {'pillow_version': np.array(PIL.__version__), 'factors': np.array(FACTORS, np.float32),
           'color_only': np.array(COLOR_ONLY, np.float32)}
    for k, (H, W) in enumerate(SIZES):
        # smooth structure plus noise (fluorescence-like: dark background, bright blobs), away from and into saturation
        yy, xx = np.mgrid[0:H, 0:W]
        base = 110 + 100 * np.sin(yy / (4.0 + k) + xx / 6.0) * np.cos(xx / (9.0 - k))
        img = np.clip(base + rs.randint(-14, 15, size=(H, W)), 0, 255).astype(np.uint8)
        out['src%d' % k] = img
        chains = []
        for f in FACTORS:
            im = Image.fromarray(img)
            assert im.mode == 'L'
            for enh, v in zip((ImageEnhance.Color, ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Sharpness), f):
                im = enh(im).enhance(float(np.float32(v)))
            chains.append(np.asarray(im))
        out['chain%d' % k] = np.stack(chains)
        out['colour%d' % k] = np.stack([np.asarray(ImageEnhance.Color(Image.fromarray(img)).enhance(float(np.float32(v)))) for v in COLOR_ONLY])
        out['filt%d' % k] = np.stack([np.asarray(Image.fromarray(img).filter(f)) for f in FILTERS])
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'augment_grey.npz'), **out)


if __name__ == '__main__':
    main()
