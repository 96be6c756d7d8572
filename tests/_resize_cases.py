"""Cases of the resize tests (CPU and GPU): the generator module of tests/golden/resize.npz and the comparison with that file."""
import importlib.util
import os

import numpy as np

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
_spec = importlib.util.spec_from_file_location('make_golden_resize', os.path.join(_GOLDEN, 'make_golden_resize.py'))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)

KERNEL_CASES, MASK_CASES = mg.KERNEL_CASES, mg.MASK_CASES
ALL = [(H, W, oh, ow, C) for (H, W, oh, ow) in KERNEL_CASES for C in (1, 3)]
_FILE = None


def golden_file():
    global _FILE
    if _FILE is None:
        _FILE = dict(np.load(os.path.join(_GOLDEN, 'resize.npz')))
    return _FILE


def assert_golden(case, got):
    """`got` (uint8 array) is the stored Pillow output of `case` = (H, W, oh, ow, C): element by element, or by SHA-256 for the large ones"""
    g, key = golden_file(), mg.case_key(*case)
    H, W, oh, ow, C = case
    assert got.dtype == np.uint8 and got.shape == ((oh, ow) if C == 1 else (oh, ow, C)), (key, got.shape)
    if 'out_' + key in g:
        assert np.array_equal(got, g['out_' + key]), key
    else:
        assert np.array_equal(mg.sha(got), g['sha_' + key]), key


def golden_mask(case):
    H, W, oh, ow = case
    bits = golden_file()['mask_' + mg.case_key(H, W, oh, ow, 1)]
    return np.unpackbits(bits)[:oh * ow].reshape(oh, ow).astype(np.uint8)
