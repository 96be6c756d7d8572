"""Device resize (csrc/resize.hip) against Pillow on the host, in one process: a 1000 x 1000 RGB image to 2000 x 2000 and to 500 x 500, and the
{0, 1} mask back to 1000 x 1000.  Device times are HIP events around one call, the median of 5 after a warm-up call (tables uploaded, kernels
loaded), for both forms; the host time is the median of 5 `Image.resize` calls.  Prints a markdown table and, per row, whether the device
resize took less time than the Pillow call it replaces - the one condition this kernel has to meet.

  python tools/bench_resize.py
"""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def device_ms(fn, reps=5):
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def host_ms(fn, reps=5):
    fn()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out)


def launches(ran, src, dst):
    """kernel launches of a resize that ran as form `ran` (0: a copy, no kernel): the LDS form is one, the two-pass form one per axis that changes"""
    if ran == 0:
        return 0
    return 1 if ran == 1 else int(src[0] != dst[0]) + int(src[1] != dst[1])


def main():
    import torch
    from PIL import Image
    from cdnet_amd import resize
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (1000, 1000, 3), dtype=np.uint8)
    rows = []
    for oh, ow in ((2000, 2000), (500, 500)):
        pil = Image.fromarray(img)
        d = torch.from_numpy(img).cuda()
        want = np.asarray(pil.resize((ow, oh), Image.BILINEAR))
        host = host_ms(lambda: pil.resize((ow, oh), Image.BILINEAR))
        for form in (1, 2):
            assert np.array_equal(resize.resize_bilinear(d, (oh, ow), form=form).cpu().numpy(), want)
            ms = device_ms(lambda: resize.resize_bilinear(d, (oh, ow), form=form))
            rows.append(('RGB 1000x1000 -> %dx%d' % (oh, ow), form, resize.last_form(), launches(resize.last_form(), (1000, 1000), (oh, ow)), ms, host))
        # the mask of that size back to the original: blobs, as a cleaned prediction has
        yy, xx = np.mgrid[0:oh, 0:ow]
        mask = (((yy // 23 + xx // 31) % 3) == 0).astype(np.uint8)
        pm = Image.fromarray(mask * np.uint8(255))
        dm = torch.from_numpy(mask).cuda()
        want = (np.asarray(pm.resize((1000, 1000), Image.BILINEAR)) > 127.5).astype(np.uint8)
        host = host_ms(lambda: np.asarray(pm.resize((1000, 1000), Image.BILINEAR)) > 127.5)
        for form in (1, 2):
            assert np.array_equal(resize.resize_mask(dm, (1000, 1000), form=form).cpu().numpy(), want)
            ms = device_ms(lambda: resize.resize_mask(dm, (1000, 1000), form=form))
            rows.append(('mask %dx%d -> 1000x1000' % (oh, ow), form, resize.last_form(), launches(resize.last_form(), (oh, ow), (1000, 1000)), ms, host))
    print('| resize | form asked | form ran | launches | device ms | Pillow ms | device faster |')
    print('|---|---|---|---|---|---|---|')
    ok = True
    for name, form, ran, nl, ms, host in rows:
        ok = ok and ms < host
        print('| %s | %d | %d | %d | %.3f | %.3f | %s |' % (name, form, ran, nl, ms, host, 'yes' if ms < host else 'NO'))
    print('every device resize faster than the Pillow call it replaces: %s' % ('yes' if ok else 'NO - the host twin would be the better implementation'))
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
