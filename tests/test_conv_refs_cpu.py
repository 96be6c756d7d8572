"""CPU side of the exact convolution tests (tests/_conv_cases.py): the float64 reference of every row kind is pinned to PyTorch
(F.conv2d, F.conv_transpose2d, torch.nn.grad.conv2d_input, autograd of conv_transpose2d, F.max_pool2d with ceil_mode, F.pad, torch.cat) -
equality is exact on lattice data in float64 - and `guard` runs for every row, so the whole table is proven to be in the exact regime
without a GPU."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _conv_cases as cc  # noqa: E402
import _wgrad_cases as wc  # noqa: E402

_RUNS = cc.runs()
_IDS = ['%s-%s' % (r.id, lat) for r, lat in _RUNS]


def test_row_ids_are_unique_and_every_row_names_a_form():
    assert len(cc.ROW_BY_ID) == len(cc.ROWS)
    for r in cc.ROWS:
        assert r.form in cc.REACHABLE, (r.id, cc.form_str(r.form))
        assert (r.form & 15) in (cc.FWD, cc.WS, cc.WS16, cc.F32K, cc.STREAM, cc.WS32), r.id
        assert r.kind in cc.KINDS and r.prec in ('16', '32') and all(lat in ('L0', 'L1', 'L2', 'LS') for lat in r.lattices), r.id
        assert not r.stats or r.lattices == ('LS',), r.id
        assert r.persistent == ((r.form & 15) in (cc.WS16, cc.WS32)), r.id


def test_form_count():
    """the table reaches every form the launchers can record but the ones listed with a reason"""
    assert cc.table_forms() | set(cc.NOT_COVERED) == cc.REACHABLE
    assert not (cc.table_forms() & set(cc.NOT_COVERED))
    assert len(cc.REACHABLE) == 152 and len(cc.table_forms()) == 149
    for f in cc.REACHABLE:                       # the decoder names every field it packs
        assert cc.form_str(f).split('<')[0] != '?'


def _torch_layer(row, data):
    """the bias-free accumulators through PyTorch's own operators: F.pad / torch.cat of the transformed sources, then the layer"""
    r = wc.rounded(dict(src=data['src'], g=torch.zeros(1, dtype=torch.float64), lattice=data['lattice']), row, row.prec)
    N, H, W = row.shape
    Ws = cc.stored_weights(row, data)
    if row.kind in ('bwdT4', 'bwdT2'):
        k = Ws[0].shape[2]
        x = torch.zeros((N, row.Cout, H, W), dtype=torch.float64, requires_grad=True)
        F.conv_transpose2d(x, Ws[0], None, stride=2, padding=1 if k == 4 else 0).backward(r['src'][0]['x'])
        return x.grad
    parts = []
    for s, d in zip(row.srcs, r['src']):
        t = d['x']
        if d['scale'] is not None:
            t = t * d['scale'].view(1, -1, 1, 1) + d['shift'].view(1, -1, 1, 1)
        if d['res'] is not None:
            t = t + d['res']
        if s.relu:
            t = F.relu(t)
        if s.pool:
            t = F.max_pool2d(t, 2, ceil_mode=(s.pool == 2))
        t = t[:, :, :H - s.off[0], :W - s.off[1]]
        parts.append(F.pad(t, (s.off[1], W - t.shape[3] - s.off[1], s.off[0], H - t.shape[2] - s.off[0])))
    if row.kind == 'mix':
        return F.conv2d(parts[0], Ws[0], None, padding=1) + F.conv2d(parts[1], Ws[1], None)
    A = torch.cat(parts, 1)
    if row.kind in ('conv3', 'conv1'):
        return F.conv2d(A, Ws[0], None, padding=Ws[0].shape[2] // 2)
    if row.kind in ('convT4', 'convT2'):
        k = Ws[0].shape[2]
        return F.conv_transpose2d(A, Ws[0], None, stride=2, padding=1 if k == 4 else 0)
    assert row.kind in ('bwd3', 'bwd1')
    k = Ws[0].shape[2]
    return torch.nn.grad.conv2d_input((N, row.Cout, H, W), Ws[0], A, padding=k // 2)


@pytest.mark.parametrize('run', _RUNS, ids=_IDS)
def test_reference_equals_pytorch_and_row_is_exact(run):
    row, lat = run
    data = cc.make_data(row, lat)
    ref = cc.reference(row, data)
    cc.guard(row, data, ref)
    N, H, W = row.shape
    Ho, Wo = cc.out_hw(row)
    assert tuple(ref['acc'].shape) == (N, row.Cout, Ho, Wo)
    if N * Ho * Wo <= 100000:                     # (the two large rows repeat the kinds of smaller ones)
        want = _torch_layer(row, data)
        assert torch.equal(ref['acc'], want), row.id
    # the epilogue and the pooled output, restated with PyTorch's operators
    v = lambda t: t.view(1, -1, 1, 1)
    x = ref['acc']
    if data['bias'] is not None:
        x = x + v(data['bias'])
    if data['oscale'] is not None:
        x = x * v(data['oscale'])
    if data['oshift'] is not None:
        x = x + v(data['oshift'])
    if row.orelu:
        x = F.relu(x)
    if data['eres'] is not None:
        e = data['eres'] if data['eres_scale'] is None else data['eres'] * v(data['eres_scale']) + v(data['eres_shift'])
        x = e + (x.half().double() if row.prec == '16' else x)
        x = F.relu(x) if row.eres_relu else x
    want_out = x.to(cc.out_dtype(row)).permute(0, 2, 3, 1)
    assert torch.equal(ref['out'], want_out), row.id
    if row.pool_out:
        assert torch.equal(ref['pool'], F.max_pool2d(want_out.permute(0, 3, 1, 2).float(), 2).to(want_out.dtype).permute(0, 2, 3, 1)), row.id
    # the data are what the lattice says: lo halves of the bf16 split present where the lattice needs them
    if lat == 'L1':
        xs = data['src'][0]['x']
        assert float((xs - xs.bfloat16().double()).abs().max()) > 0.0
    if lat == 'L2':
        w = data['w'][0]
        assert float((w - w.bfloat16().double()).abs().max()) > 0.0


def test_reference_is_sensitive():
    """one dropped tap or one shifted weight moves the reference by at least a lattice unit somewhere"""
    row = cc.ROW_BY_ID['fwd-conv3-t16-ck16-bn32']
    data = cc.make_data(row, 'L0')
    acc = cc.reference(row, data)['acc']
    w = data['w'][0].clone()
    w[:, :, 0, 2] = 0.0
    d2 = dict(data, w=[w])
    assert float((cc.reference(row, d2)['acc'] - acc).abs().max()) >= cc.unit('L0')
    w = data['w'][0].clone()
    w[5, 3, 1, 1] += 1.0
    d3 = dict(data, w=[w])
    assert float((cc.reference(row, d3)['acc'] - acc).abs().max()) >= cc.unit('L0')
