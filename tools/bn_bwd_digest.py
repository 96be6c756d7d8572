"""SHA-256 of what the BatchNorm-backward entries write, path by path: two builds print equal listings exactly when every kernel path
computes the same bits.

  python tools/bn_bwd_digest.py [--out FILE]

The cases are those of tests/test_gpu_bn_bwd.py and of the pool / pad cases of the older kernel tests (N = 2, 13 x 21, C = 32 or 48),
plus one large shape per kernel family (N = 1, 365 x 363, C = 32: more than 512 workgroups' worth of pixels and of windows in both
precisions, so the grid-stride loop, the cap on the workgroup count and the back-to-front walk take more than one trip).  Inputs
come from numpy.random.RandomState(seed); only C entries are used, so the file runs against any build of the library."""
import argparse
import ctypes as C
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SMALL, LARGE = (2, 13, 21), (1, 365, 363)


def cases():
    """(name, dict): fmt f16 / bf16 / f32, C, size, pooled, skip (channel-slice same-size sources), plain (own same-size sources), pad
    (an F.pad-shifted channel-slice source), res, relu, bn, pool_first, entry"""
    out = []

    def add(name, **kw):
        d = dict(fmt='f16', Cc=32, size=SMALL, pooled=False, skip=0, plain=0, pad=False, res=False, relu=1, bn=True, pool_first=True,
                 entry='fused')
        d.update(kw)
        out.append((name, d))
    for fmt in ('f16', 'bf16', 'f32'):
        for n in (1, 2, 3):
            for res in (False, True):
                add('flat %s ngin=%d res=%d' % (fmt, n, res), fmt=fmt, plain=n, res=res)
    for fmt in ('f16', 'bf16', 'f32'):
        add('flat %s relu=2' % fmt, fmt=fmt, plain=1, res=True, relu=2)
    for fmt in ('f16', 'f32'):
        add('flat %s relu=0' % fmt, fmt=fmt, plain=1, relu=0)
    for fmt in ('f16', 'f32'):
        for nf in (0, 1, 2):
            for first in (True, False):
                add('window %s nflat=%d pool_first=%d' % (fmt, nf, first), fmt=fmt, pooled=True, skip=nf, pool_first=first)
    for fmt in ('f16', 'f32'):
        add('generic %s pad' % fmt, fmt=fmt, pad=True)
        add('generic %s pool+pad' % fmt, fmt=fmt, pooled=True, pad=True)
        add('generic %s pad res' % fmt, fmt=fmt, pad=True, res=True)
        add('generic %s pool+pad res' % fmt, fmt=fmt, pooled=True, pad=True, res=True)
        add('C=48 flat %s' % fmt, fmt=fmt, Cc=48, plain=1)
        add('C=48 generic %s' % fmt, fmt=fmt, Cc=48, pad=True)
        add('no BatchNorm %s' % fmt, fmt=fmt, plain=2, bn=False)
    add('split stats+apply f16', plain=1, entry='stats')
    add('split stats+finalize+apply f16', plain=1, entry='finalize')
    add('split apply f32', fmt='f32', plain=1, entry='apply32')
    for fmt in ('f16', 'f32'):
        add('large flat %s' % fmt, fmt=fmt, size=LARGE, plain=1)
        add('large flat %s res' % fmt, fmt=fmt, size=LARGE, plain=2, res=True)
        add('large window %s' % fmt, fmt=fmt, size=LARGE, pooled=True, skip=1)
        add('large generic %s' % fmt, fmt=fmt, size=LARGE, pooled=True, pad=True)
    return out


def run_case(d, seed):
    import torch
    from cdnet_amd import _lib, trainer
    rs = np.random.RandomState(seed)
    f32 = d['fmt'] == 'f32'
    raw_dt = {'f16': torch.float16, 'bf16': torch.bfloat16, 'f32': torch.float32}[d['fmt']]
    act_dt = torch.float32 if f32 else torch.bfloat16
    (N, H, W), Cc = d['size'], d['Cc']

    def rand(shape, dt=act_dt):
        return torch.from_numpy(rs.standard_normal(shape).astype(np.float32)).to(dt).cuda()
    raw = rand((N, H, W, Cc), raw_dt)
    res = None
    if d['res']:
        res = rand((N, H, W, Cc), act_dt if d['relu'] == 2 else raw_dt)      # relu = 2: the stored (bf16 / fp32) output of the unit
    gamma = torch.from_numpy(((rs.rand(Cc) + 0.5) * np.where(np.arange(Cc) % 4 == 0, -1, 1)).astype(np.float32)).cuda()
    beta = rand((Cc,), torch.float32) * 0.2
    x = raw.float().reshape(-1, Cc)
    mean = x.mean(0)
    invstd = 1.0 / torch.sqrt(x.var(0, unbiased=False) + 1e-5)
    scale = (gamma * invstd).contiguous()
    shift = (beta - mean * scale).contiguous()
    gins = []
    if d['pooled']:
        gins.append(trainer._G(rand((N, H // 2, W // 2, Cc)), H // 2, W // 2, pooled=1))
    for _ in range(d['skip']):
        gins.append(trainer._G(rand((N, H, W, Cc + 16)), H, W, coff=16, cstride=Cc + 16))
    for _ in range(d['plain']):
        gins.append(trainer._G(rand((N, H, W, Cc)), H, W))
    if not d['pool_first']:
        gins = gins[1:] + gins[:1]
    if d['pad']:
        gins.append(trainer._G(rand((N, H + 1, W + 3, Cc + 16)), H + 1, W + 3, oy=1, ox=2, coff=8, cstride=Cc + 16))
    A = trainer.BnBwdArgs()
    A.raw, A.res = raw.data_ptr(), (res.data_ptr() if res is not None else None)
    if d['bn']:
        A.scale, A.shift, A.mean, A.invstd = scale.data_ptr(), shift.data_ptr(), mean.data_ptr(), invstd.data_ptr()
    A.ngin = len(gins)
    for k, gi in enumerate(gins):
        A.gin[k].g = gi.t.data_ptr()
        A.gin[k].Hg, A.gin[k].Wg, A.gin[k].oy, A.gin[k].ox = gi.Hg, gi.Wg, gi.oy, gi.ox
        A.gin[k].pooled, A.gin[k].coff, A.gin[k].cstride = gi.pooled, gi.coff, gi.cstride or Cc
    A.f16 = {'bf16': 0, 'f16': 1, 'f32': 2}[d['fmt']]
    A.relu, A.N, A.H, A.W, A.C = d['relu'], N, H, W, Cc
    lib = _lib.load()
    ws = torch.zeros((lib.cdnet_bn_backward_workspace_floats(Cc),), dtype=torch.float32, device='cuda')
    dgamma, dbeta = torch.zeros(Cc, device='cuda'), torch.zeros(Cc, device='cuda')
    draw = torch.zeros((N, H, W, Cc), dtype=act_dt, device='cuda')
    dz = torch.zeros((N, H, W, Cc), dtype=act_dt, device='cuda')
    st = _lib.stream_ptr()
    bn = d['bn']
    if d['entry'] in ('fused', 'apply32'):
        _lib.call('cdnet_bn_backward', C.byref(A), _lib.ptr(gamma) if bn else None, _lib.ptr(dgamma) if bn else None,
                  _lib.ptr(dbeta) if bn else None, _lib.ptr(ws), ws.numel(), _lib.ptr(draw), _lib.ptr(dz) if d['res'] else None, st)
        if d['entry'] == 'apply32':
            # (the fp32 apply entry has no stats twin: the coefficients of the fused call, rows 4..6 of a ktab)
            nb = max(1, min(512, -(-N * H * W // ((256 // (Cc // 4)) * 4))))
            ktab = torch.zeros((7, Cc), dtype=torch.float32, device='cuda')
            ktab[4:] = ws[nb * 2 * Cc: nb * 2 * Cc + 3 * Cc].reshape(3, Cc)
            draw.zero_()
            _lib.call('cdnet_bn_backward_apply', C.byref(A), _lib.ptr(ktab), _lib.ptr(draw), st)
    else:
        ktab = torch.zeros((7, Cc), dtype=torch.float32, device='cuda')
        _lib.call('cdnet_bn_backward_stats', C.byref(A), _lib.ptr(gamma), _lib.ptr(dgamma), _lib.ptr(dbeta), _lib.ptr(ws), ws.numel(),
                  _lib.ptr(ktab), st)
        if d['entry'] == 'finalize':
            nb = max(1, min(512, -(-N * H * W // ((256 // (Cc // 8)) * 4))))
            ktab.zero_(); dgamma.zero_(); dbeta.zero_()
            _lib.call('cdnet_bn_backward_finalize', C.byref(A), _lib.ptr(gamma), _lib.ptr(dgamma), _lib.ptr(dbeta), _lib.ptr(ws), nb,
                      _lib.ptr(ktab), st)
        _lib.call('cdnet_bn_backward_apply', C.byref(A), _lib.ptr(ktab), _lib.ptr(draw), st)
    torch.cuda.synchronize()
    keep = (raw, res, gins, scale, shift, mean, invstd)           # (alive until the kernels are done)
    del keep
    return draw, dz, dgamma, dbeta


def digest(t):
    import torch
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lines = []
    for i, (name, d) in enumerate(cases()):
        outs = run_case(d, seed=1000 + i)
        lines.append('%-40s draw %s  dz %s  dgamma %s  dbeta %s' % ((name,) + tuple(digest(t) for t in outs)))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
