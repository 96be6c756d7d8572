"""CPU-side checks of tests/_bn_exact_cases.py: the float64 reference of BatchNorm backward against CPU autograd in float64 (random data,
no ties), its first-maximum rule against F.max_pool2d(return_indices=True) on the lattices, the guard of every row, and the plan decoder
against the bit layout include/cdnet_hip.h documents.  No GPU."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bn_exact_cases as bx  # noqa: E402
from conftest import ROOT  # noqa: E402

N, H, W, CC = 2, 5, 7, 8

# (sources, res, relu, bn)
AUTOGRAD_CASES = [
    (('same',), False, 1, True), (('same', 'slice', 'same'), True, 1, True), (('pad',), False, 1, True), (('pad', 'slice'), True, 1, True),
    (('pool1',), False, 1, True), (('pool2',), False, 1, True), (('pool2s', 'same'), True, 1, True), (('pool1', 'pool2', 'pad'), False, 1, True),
    (('same',), False, 0, True), (('same', 'same'), True, 2, True), (('same', 'pad'), False, 1, False), (('pool2',), True, 1, False),
]


def _autograd_case(srcs, res, relu, bn, seed):
    """random float64 data -> (row, data for `reference`, autograd gradients as NHWC numpy)"""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(seed)
    row = bx.Row('cpu', 'f32', (N, H, W), CC, srcs, bx.PATH_GENERIC, res=res, relu=relu, bn=bn, lat='R')
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).permute(0, 3, 1, 2).contiguous()
    raw = t(rng.standard_normal((N, H, W, CC))).requires_grad_(True)
    r0 = t(rng.standard_normal((N, H, W, CC))).requires_grad_(True) if res else None
    gamma = torch.from_numpy((rng.random(CC) + 0.5) * np.where(np.arange(CC) % 3 == 0, -1.0, 1.0)).requires_grad_(True)
    beta = torch.from_numpy(0.2 * rng.standard_normal(CC)).requires_grad_(True)
    y = F.batch_norm(raw, None, None, gamma, beta, training=True, eps=1e-5) if bn else raw
    if res:
        y = y + r0
    y.retain_grad()
    a = F.relu(y) if relu else y
    d = dict(raw=raw.detach().permute(0, 2, 3, 1).numpy().copy(), res=None, scale=None, shift=None, mean=None, invstd=None, gamma=None, srcs=[])
    if bn:
        x = d['raw'].reshape(-1, CC)
        d['mean'], d['invstd'], d['gamma'] = x.mean(0), 1.0 / np.sqrt(x.var(0) + 1e-5), gamma.detach().numpy().copy()
        d['scale'] = d['gamma'] * d['invstd']
        d['shift'] = beta.detach().numpy() - d['mean'] * d['scale']
    if res:
        # relu = 2: the call gets the stored output of the unit and reads the mask from it
        d['res'] = (a if relu == 2 else r0).detach().permute(0, 2, 3, 1).numpy().copy()
    total = 0
    for kind in srcs:
        g = bx.src_geometry(kind, H, W, CC)
        G = rng.standard_normal((N, g['Hg'], g['Wg'], g['cstride']))
        Gt = t(G)[:, g['coff']:g['coff'] + CC]
        if g['pooled']:
            total = total + (F.max_pool2d(a, 2, ceil_mode=g['pooled'] == 2) * Gt).sum()
        elif kind == 'pad':
            total = total + (F.pad(a, (2, 1, 1, 0)) * Gt).sum()
        else:
            total = total + (a * Gt).sum()
        G[~bx.read_mask(g, N, H, W, CC)] = np.nan
        d['srcs'].append(dict(g, G=G, kind=kind))
    total.backward()
    nhwc = lambda x: x.permute(0, 2, 3, 1).numpy()
    return row, d, dict(draw=nhwc(raw.grad), dz=nhwc(y.grad), dgamma=gamma.grad.numpy() if bn else None, dbeta=beta.grad.numpy() if bn else None)


@pytest.mark.parametrize('case', AUTOGRAD_CASES, ids=['%s-res%d-relu%d-bn%d' % ('+'.join(c[0]), c[1], c[2], c[3]) for c in AUTOGRAD_CASES])
def test_reference_matches_autograd(case):
    """F.batch_norm, F.relu, F.max_pool2d with and without ceil_mode, F.pad and slicing in float64 autograd.  The reference rounds the
    activation's argument to fp32 (relative 2^-24), nothing else: 1e-6 of the largest gradient."""
    row, d, want = _autograd_case(*case, seed=7 + len(case[0]))
    ref = bx.reference(row, d)
    close = lambda a, b: np.abs(a - b).max() <= 1e-6 * max(1.0, np.abs(b).max())
    assert close(ref['draw'], want['draw'])
    # y.grad is the gradient behind the ReLU mask: dz (relu = 0: the source is masked already, dz = g)
    assert close(ref['dz'], want['dz'])
    if row.bn:
        assert close(ref['dgamma'], want['dgamma']) and close(ref['dbeta'], want['dbeta'])


_POOLED = [r for r in bx.ROWS if r.pooled and r.shape == bx.A and r.C == 32 and r.lat != 'R']


@pytest.mark.parametrize('row', _POOLED[::3], ids=[r.id for r in _POOLED[::3]])
def test_first_maximum_is_max_pool2d(row):
    """the arg-max of nn.MaxPool2d on lattice data (placed ties, ties made by the bf16 rounding), floor and ceil mode"""
    import torch
    import torch.nn.functional as F
    n, h, w = row.shape
    d = bx.make_data(row)
    a, _ = bx.activation(row.shape, d, row.relu, row.f32)
    sel = bx.first_max(a, h, w)
    at = torch.from_numpy(a).permute(0, 3, 1, 2).contiguous()
    for ceil in (False, True):
        _, idx = F.max_pool2d(at, 2, ceil_mode=ceil, return_indices=True)
        want = torch.zeros((n, row.C, h * w), dtype=torch.bool)
        want.scatter_(2, idx.reshape(n, row.C, -1), True)
        want = want.reshape(n, row.C, h, w).permute(0, 2, 3, 1).numpy()
        hh, ww = (h, w) if ceil else (h // 2 * 2, w // 2 * 2)
        assert np.array_equal(sel[:, :hh, :ww], want[:, :hh, :ww])
        assert not want[:, hh:].any() and not want[:, :, ww:].any()


@pytest.mark.parametrize('row', bx.ROWS, ids=[r.id for r in bx.ROWS])
def test_guard(row):
    d = bx.make_data(row)
    bx.guard(row, d, bx.reference(row, d))


def test_rows_reach_every_instantiation():
    """the plans the rows name, both passes: every instantiation of `launch` but the six flat apply kernels with a residual, which run only
    in a process with CDNET_BN_DZ_REUSE=0 (test_gpu_bn_bwd_exact.py starts one)"""
    reached = set()
    for r in bx.ROWS:
        for p in r.plans():
            if p is not None:
                reached.add(bx.instantiation(p))
    no_reuse = {bx.instantiation(r.plans(reuse=False)[1]) for r in bx.ROWS if r.reuse}
    assert no_reuse == {('flat', f, n, 1, 1) for f in (0, 1) for n in (1, 2, 3)}
    assert reached == bx.all_instantiations() - no_reuse
    assert len(reached | no_reuse) == 40
    for r in bx.ROWS:
        if r.shape == bx.K:
            assert r.nb == 512, r.id


def test_plan_decoder_matches_the_header():
    txt = open(os.path.join(ROOT, 'include', 'cdnet_hip.h')).read()
    doc = txt[:txt.index('int cdnet_bn_backward_last_plan(void);')]
    doc = doc[doc.rindex('Bit layout:'):]
    fields = {m.group(3): (int(m.group(1)), int(m.group(2) or m.group(1))) for m in re.finditer(r'bits?\s+(\d+)(?:-(\d+))?\s+(\w+)', doc)}
    names = dict(path='path', f32='f32', n='NF', res='RES', kp='kp', apply='pass', dz_source='the', nb='nb')
    assert set(names.values()) <= set(fields), fields
    for key, word in names.items():
        lo, hi = fields[word]
        for v in (1, (1 << (hi - lo + 1)) - 1):
            dec = bx.plan_decode(v << lo)
            assert dec[key] == v and all(x == 0 for k, x in dec.items() if k != key), (key, v, dec)
    for name, val in (('WINDOW', bx.PATH_WINDOW), ('FLAT', bx.PATH_FLAT), ('GENERIC', bx.PATH_GENERIC)):
        assert int(re.search(r'#define CDNET_BN_PATH_%s\s+(\d+)' % name, txt).group(1)) == val
    p = bx.plan_encode(bx.PATH_WINDOW, 1, 2, 0, 2, 1, 0, 512)
    assert p == 1 | 1 << 2 | 2 << 3 | 2 << 6 | 1 << 8 | 512 << 10
    assert bx.plan_decode(p) == dict(path=1, f32=1, n=2, res=0, kp=2, apply=1, dz_source=0, nb=512)
    assert bx.plan_decode(bx.plan_encode(bx.PATH_FLAT, 0, 1, 0, 0, 1, 1, 2048))['nb'] == 2048
