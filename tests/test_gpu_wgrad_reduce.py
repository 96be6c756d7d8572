"""The split-K reduce kernels of csrc/wgrad.hip on their own: slabs of lattice integers (every sum exact in any order) through
cdnet_wgrad_reduce_desc_fill + cdnet_wgrad_reduce_batch, compared for equality with the numpy restatement of the sum and the scatter
(tests/_wgrad_cases.py, pinned to the PyTorch layouts by test_wgrad_refs_cpu.py).  dW starts from a sentinel inside a larger buffer;
slab elements the scatter must drop (padded input channels, output channels past Cout, the stride-2 form's tap / parity pairs outside
the 3x3 kernel) hold a large off-lattice value."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _wgrad_cases as wc  # noqa: E402

pytestmark = pytest.mark.gpu

POISON = 7777.25
# mode -> (taps, npar)
FORMS = {(0, 9): (9, 1), (0, 1): (1, 1), (2, 4): (4, 4), (3, 1): (1, 4), (6, 9): (9, 1)}


class Job:
    """one descriptor: geometry, slab, expected dW"""

    def __init__(self, mode, taps, ci_t, C_src, Csrc_real, Cin_real, src_coff, Cout, ksplit, seed):
        import torch
        self.mode, self.taps, self.npar = mode, taps, FORMS[(mode, taps)][1]
        self.ci_t, self.C_src, self.Csrc_real, self.Cin_real, self.src_coff, self.Cout, self.ksplit = ci_t, C_src, Csrc_real, Cin_real, src_coff, Cout, ksplit
        CI, CO = ci_t * 32, (4 // ci_t) * 32
        cib, cob = -(-C_src // CI), -(-Cout // CO)
        self.idx = wc.scatter_index(mode, self.npar, cib, cob, taps, CI, CO, Csrc_real, Cin_real, src_coff, Cout)
        rng = np.random.default_rng(seed)
        slab = rng.integers(-8, 9, size=(ksplit, self.idx.size)).astype(np.float32)
        slab[:, self.idx < 0] = POISON
        k = {0: int(round(taps ** 0.5)), 2: 4, 3: 2, 6: 3}[mode]
        cin = Cin_real // 4 if mode == 6 else Cin_real
        self.shape = (cin, Cout, k, k) if mode in (2, 3) else (Cout, cin, k, k)
        n = int(np.prod(self.shape))
        live = self.idx[self.idx >= 0]
        assert len(np.unique(live)) == len(live) and live.max() < n and 0 < len(live) < n     # (some of dW belongs to other sources)
        self.want = wc.reduce_ref(slab, self.idx, np.full(n, np.float32(wc.SENTINEL), dtype=np.float32))
        self.slab = torch.from_numpy(slab).cuda()
        self.buf = wc.DwBuffer((n,))
        assert self.slab.numel() == self.lib_floats()

    def lib_floats(self):
        from cdnet_amd import _lib
        return _lib.load().cdnet_conv_wgrad_slab_floats(self.C_src, self.Cout, self.taps, self.npar, self.ci_t, self.ksplit)

    def args(self):
        from cdnet_amd import _lib
        return (self.C_src, self.src_coff, self.Csrc_real, self.Cin_real, self.Cout, self.taps, self.npar, self.ci_t, self.ksplit,
                _lib.ptr(self.slab), self.buf.ptr(), self.mode)

    def check(self, what):
        got, slack_ok = self.buf.read()
        assert slack_ok, what + ': wrote outside dW'
        got = got.numpy()
        bad = np.nonzero(got != self.want)[0]
        assert np.array_equal(got, self.want), '%s: %d of %d differ, first %s: got %r want %r' % (
            what, len(bad), got.size, np.unravel_index(bad[0], self.shape), got[bad[0]], self.want[bad[0]])


# ksplit on each side of the eight-in-flight loop's bound (k + 28 < ksplit) for each of the four k-lanes, and of its second round
@pytest.mark.parametrize('ksplit', [1, 2, 3, 4, 5, 28, 29, 31, 32, 33, 61, 64, 256])
def test_reduce_split_factors(ksplit):
    """the smallest slab (one 1x1 block: 4096 floats per slice), ragged on both sides, inside a wider layer (src_coff > 0)"""
    for ci_t, C_src, real, Cout in ((2, 40, 35, 24), (1, 32, 29, 72), (4, 128, 127, 8)):
        j = Job(0, 1, ci_t, C_src, real, real + 9, 5, Cout, ksplit, seed=ksplit * 8 + ci_t)
        descs = wc.reduce_batch([j.args()])
        assert descs[0].blocks * 256 == j.idx.size
        j.check('ci_tiles %d ksplit %d' % (ci_t, ksplit))


@pytest.mark.parametrize('mode,taps', sorted(FORMS))
@pytest.mark.parametrize('ci_t', [1, 2, 4])
def test_reduce_modes(mode, taps, ci_t):
    """every scatter mode x block shape: Cout no multiple of CO, Csrc_real < C, src_coff > 0; mode 6: the two row-parity sources of a
    stride-2 layer (Cin_real = 4 Ct, source a at src_coff 2 a Ct), whose out-of-kernel tap / parity pairs must not be written"""
    CI, CO = ci_t * 32, (4 // ci_t) * 32
    Cout = CO + 8
    for n, ksplit in enumerate((3, 29, 33)):
        if mode == 6:
            Ct = (CI + 8) // 2 if ci_t != 4 else 68
            jobs = [Job(6, 9, ci_t, 2 * Ct, 2 * Ct, 4 * Ct, a * 2 * Ct, Cout, ksplit, seed=100 * mode + 10 * ci_t + a) for a in (0, 1)]
            for a, j in enumerate(jobs):
                kh = (j.idx[j.idx >= 0] // 3) % 3
                assert set(kh.tolist()) == ({1} if a == 0 else {0, 2})
        else:
            C_src = CI + 8
            jobs = [Job(mode, taps, ci_t, C_src, C_src - 3, C_src + 13, 16, Cout, ksplit, seed=100 * mode + 10 * ci_t + n)]
        for j in jobs:
            wc.reduce_batch([j.args()])
            j.check('mode %d taps %d ci_tiles %d ksplit %d' % (mode, taps, ci_t, ksplit))


def test_reduce_batch_of_seven():
    """seven descriptors of unequal block counts in one launch: the bisection over block0 meets the first entry, the last entry and
    every exact block0 boundary (each workgroup's result is checked, so a block attributed to a neighbour shows)"""
    jobs = [Job(0, 1, 2, 40, 35, 50, 5, 24, 5, seed=1),              # 16 blocks
            Job(2, 4, 1, 40, 40, 72, 32, 136, 29, seed=2),           # 4 x 2 x 2 x 4 blocks of 4096
            Job(0, 9, 4, 136, 130, 135, 5, 40, 2, seed=3),
            Job(0, 1, 1, 32, 30, 37, 7, 8, 33, seed=4),              # 16 blocks
            Job(6, 9, 2, 72, 72, 144, 72, 72, 4, seed=5),
            Job(3, 1, 2, 64, 61, 64, 0, 32, 61, seed=6),
            Job(0, 1, 4, 128, 128, 131, 3, 24, 1, seed=7)]           # 16 blocks
    descs = wc.reduce_batch([j.args() for j in jobs])
    counts = [d.blocks for d in descs]
    assert len(set(counts)) >= 4 and [d.block0 for d in descs] == np.cumsum([0] + counts[:-1]).tolist()
    for n, j in enumerate(jobs):
        j.check('descriptor %d' % n)
