"""What a training forward leaves on the tape (runtime.ConvRecord / FuseRecord) and what the tape walk leaves behind: records in execution
order, the residual units' annotations under both settings of runtime.RU_FUSE, one set of records per forward, nothing pending after a
step, and no state that survives on layers between steps.  rev1 DAM-Unet at 2 x 64 x 64 and HRNet18_rev1 at the 2 x 64 x 64 of
tests/test_gpu_hrnet_train.py, both precision modes."""
import pytest

pytestmark = pytest.mark.gpu


class _Opt:
    model = {'out_c': 3}


@pytest.fixture(params=['fp32', 'bf16'])
def precision(request):
    import cdnet_amd
    before = cdnet_amd.get_precision()
    cdnet_amd.set_precision(request.param)
    yield request.param
    cdnet_amd.set_precision(before)


def _trainer(net, seed=3):
    import torch
    from cdnet_amd import trainer
    torch.manual_seed(seed)
    if net == 'rev1':
        from cdnet_amd.models.dam.model_unet_rev1 import Unet
        m = Unet(backbone_name='vgg16_bn', pretrained=False, classes=3)
    else:
        from cdnet_amd.models.dam.seg_hrnet_rev1 import HighResolutionNet
        m = HighResolutionNet(_Opt())
    return trainer.Trainer(m.cuda())


def _batch(seed=11):
    import torch
    from cdnet_amd import trainer
    return trainer.synthetic_batch(2, torch.device('cuda:0'), seed=seed, H=64, W=64)


def _conv_records(tape):
    from cdnet_amd import runtime
    return [r for r in tape if isinstance(r, runtime.ConvRecord)]


def _check_execution_order(tape):
    """every stored tensor a record reads (as a source, a residual branch, a fuse term or through a materialised copy's grad_to) that some
    record wrote was written by an EARLIER record"""
    from cdnet_amd import runtime
    pos = {}
    for k, r in enumerate(tape):
        assert isinstance(r, (runtime.ConvRecord, runtime.FuseRecord)), type(r)
        pos.setdefault(id(r.out), k)                 # (HRNet's concatenation buffer has four writers: the first one counts)
    for k, r in enumerate(tape):
        reads = r.terms if isinstance(r, runtime.FuseRecord) else r.srcs
        for s in reads:
            for t in (s.x, s.res, None if s.grad_to is None else s.grad_to[0]):
                if t is not None and id(t) in pos and t is not r.out:
                    assert pos[id(t)] < k, (k, getattr(r, 'layer', getattr(r, 'node', None)).name)


@pytest.mark.parametrize('fuse', [True, False])
@pytest.mark.parametrize('net', ['rev1', 'hrnet'])
def test_forward_leaves_records_in_execution_order(net, fuse, precision, monkeypatch):
    import torch
    from cdnet_amd import runtime
    monkeypatch.setattr(runtime, 'RU_FUSE', fuse)
    tr = _trainer(net)
    m = tr.model
    tr.forward(_batch()[0])
    torch.cuda.synchronize()
    tape = list(tr.tape)
    recs = _conv_records(tape)
    assert recs and runtime.TAPE is None
    _check_execution_order(tape)
    by_layer = {id(r.layer): r for r in recs}
    assert len(by_layer) == len(recs)                          # one record per layer and forward
    assert all(r.layer.rec is r for r in recs)
    assert all(r.deferred is None and r.res_grad_to is None for r in recs)
    if net == 'rev1':
        units = [u.layers() for u in m._rt['ru']]
        order = [L.name for L in m.conv_layers()]
        if not fuse:                                           # the 1x1 branch runs first there
            for c1, c2, cr in units:
                i = order.index(c1.name)
                order[i:i + 3] = [cr.name, c1.name, c2.name]
        assert [r.layer.name for r in tape] == order
    else:
        assert any(isinstance(r, runtime.FuseRecord) for r in tape)
    assert len(m._rt['ru']) == 3
    for u in m._rt['ru']:
        r1, r2, rr = (by_layer[id(L)] for L in (u.c1, u.c2, u.cr))
        assert r1.relu is True and r1.res is None and r1.fused_res_of is None and r2.fused_res_of is None
        if fuse:
            assert rr.fused_res_of is r2 and r2.relu == 2 and r2.res is rr.out
            assert tape.index(r1) < tape.index(r2) < tape.index(rr)
        else:
            assert rr.fused_res_of is None and r2.relu is True and r2.res is rr.out
        assert rr.relu is False and rr.res is None


@pytest.mark.parametrize('net', ['rev1', 'hrnet'])
def test_every_forward_has_its_own_records(net, precision):
    import torch
    from cdnet_amd import runtime
    tr = _trainer(net)
    tr.forward(_batch(11)[0])
    first = list(tr.tape)
    outs = [r.out for r in first]
    last = first[-1].out.clone()
    tr.forward(_batch(12)[0])
    torch.cuda.synchronize()
    second = list(tr.tape)
    assert len(first) == len(second)
    for a, b, o in zip(first, second, outs):
        assert a is not b and type(a) is type(b) and a.out is o
        if isinstance(a, runtime.ConvRecord):
            assert a.layer is b.layer and b.layer.rec is b
        own = isinstance(a, runtime.ConvRecord) or a.out.shape[3] == a.C          # (not a slice of HRNet's kept concatenation buffer)
        if own:
            assert a.out is not b.out and a.out.data_ptr() != b.out.data_ptr()
    assert torch.equal(first[-1].out, last) and not torch.equal(second[-1].out, last)


@pytest.mark.parametrize('net', ['rev1', 'hrnet'])
def test_a_step_leaves_nothing_pending_and_no_state_on_layers(net, precision):
    import torch

    def run():
        tr = _trainer(net)
        batch = _batch()
        losses = [tr.train_step(*batch).clone() for _ in range(2)]
        torch.cuda.synchronize()
        return tr, tr.flat.P.clone(), torch.stack(losses)

    tr, p1, l1 = run()
    recs = _conv_records(tr.tape)
    assert recs and all(r.deferred is None and r.res_grad_to is None for r in recs)
    _, p2, l2 = run()
    assert bool(torch.isfinite(l1).all()) and torch.equal(p1, p2) and torch.equal(l1, l2)
