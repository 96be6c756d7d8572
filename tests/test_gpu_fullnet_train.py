"""FullNet training on the device (trainer.FullNetTrainer, fp32 precision mode) against the fp64 mirror tests/_fullnet_train_ref.py.

One step: logits, loss, every parameter's gradient and the running statistics of one forward + loss + backward.  Per tensor the error is
max|got - mirror| / max|mirror|; the bar is 3 x the envelope (the factor of tests/test_gpu_fp32.py), the mirror's own change when every
product site carries an independent relative 2^-16 U(-1, 1) error, maximum over 8 seeds - a CPU quantity.  The device hands the mirror
the dropout masks (cdnet_dropout_mask) and the LeakyReLU signs (z > 0 of its saved tensors); tools/fullnet_train_envelope.py checks
the bar on the CPU: with 4 seeds a fifth, independent one reached 1.4 - 2.6 envelopes per network, beyond the 1.5 asked for, so 8 seeds
are used; a ninth then reaches 1.4 - 1.9 (DESIGN.md section 4.9 has the table)."""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def fp32_mode():
    import cdnet_amd
    before = cdnet_amd.get_precision()
    cdnet_amd.set_precision('fp32')
    yield
    cdnet_amd.set_precision(before)


def _mask(key, layer, shape, p):
    import torch
    from cdnet_amd import _lib
    n = int(np.prod(shape))
    m = torch.empty((n,), dtype=torch.uint8, device='cuda')
    _lib.call('cdnet_dropout_mask', key, layer, n, p, _lib.ptr(m), _lib.stream_ptr())
    return m.view(shape).permute(0, 3, 1, 2).bool().cpu()


def _prefixes(model):
    """id(nn.Conv2d) -> the ConvLayer's name in the state dict"""
    from cdnet_amd.models.FullNet import ConvLayer
    return {id(mod.conv): name for name, mod in model.named_modules() if isinstance(mod, ConvLayer)}


@pytest.mark.parametrize('name', ['small-p0', 'small-p0.1', 'default', 'bottleneck'])
def test_one_step_against_the_mirror(name, fp32_mode):
    import torch
    import _fullnet_ref as fr
    import _fullnet_train_ref as tr
    from oracle import train as ot
    from cdnet_amd.models.FullNet import FullNet
    from cdnet_amd.trainer import FullNetTrainer
    kw, dil, shape = tr.CASES[name]
    k = list(tr.CASES).index(name)
    m = fr.randomize(FullNet(**kw), 60 + k).cuda()
    t = FullNetTrainer(m, seed=7)
    sd = {n: v.detach().cpu().clone() for n, v in m.state_dict().items()}
    x, label, weight = tr.batch(shape, 70 + k)
    logits = t.forward(x.cuda())
    dl = t.loss_and_grads(logits, label.cuda(), weight.cuda())
    t.backward(dl)
    torch.cuda.synchronize()
    rec = t.tape[-1]
    p = float(kw.get('drop_rate', 0.1))

    # the masks the device used
    names = _prefixes(m)
    convs = m._convs()
    signs = {names[id(c.conv)]: (rec.z[id(c)][..., :c.Cout] > 0).permute(0, 3, 1, 2).cpu() for c in convs if c.bn is not None}
    drops = {names[id(convs[li].conv)]: _mask(rec.key, li, shp, pd) for li, shp, pd in rec.drops}
    want_drops = [pre for pre, _, last in tr.conv_prefixes(sd, dil) if last] if p > 0 else []
    assert sorted(drops) == sorted(want_drops)
    for pre, mk in drops.items():
        kept = float(mk.double().mean())
        assert abs(kept - (1 - p)) <= 5 * np.sqrt(p * (1 - p) / mk.numel()), (pre, kept)

    got = {'logits': logits.cpu().double(), 'loss': t.mask_losses[0:1].cpu().double()}
    got.update({'grad ' + n: q.grad.detach().cpu().double().view(q.shape) for n, q in m.named_parameters()})
    got.update({n: b.detach().cpu().double() for n, b in m.named_buffers() if 'running_' in n})

    loss_fn = lambda lg: ot.unet_losses(lg, label, weight)['total']
    clean, env = tr.envelope(sd, x, dil, signs, drops, p, loss_fn, tr.ENVELOPE_SEEDS)
    want = tr.tensors(clean)
    assert sorted(got) == sorted(want)
    worst, rows = 0.0, []
    for n in want:
        assert got[n].shape == want[n].shape, n
        err = float((got[n] - want[n]).abs().max()) / float(want[n].abs().max())
        rows.append((err / env[n], n, err, env[n]))
    rows.sort(reverse=True)
    for ratio, n, err, e in rows[:8]:
        print('%s %-60s err %.3e envelope %.3e ratio %.2f' % (name, n, err, e, ratio))
    kinds = {'logits': [r for r in rows if r[1] == 'logits'], 'loss': [r for r in rows if r[1] == 'loss'],
             'gradients': [r for r in rows if r[1].startswith('grad ')], 'running statistics': [r for r in rows if 'running_' in r[1]]}
    for kind, rs in kinds.items():
        print('%s %s: worst err / envelope %.2f over %d tensors' % (name, kind, max(r[0] for r in rs), len(rs)))
    bad = [(n, err, e) for ratio, n, err, e in rows if not err <= 3 * e]
    assert not bad, '%d of %d tensors beyond 3 envelopes, worst %s' % (len(bad), len(rows), rows[0])


@functools.lru_cache(maxsize=None)
def _trained():
    """SMALL with drop_rate 0 after 10 Adam steps on one fixed batch (fp32 mode): (model, losses, batch)"""
    import torch
    import cdnet_amd
    import _fullnet_ref as fr
    import _fullnet_train_ref as tr
    from cdnet_amd.models.FullNet import FullNet
    from cdnet_amd.trainer import FullNetTrainer
    before = cdnet_amd.get_precision()
    cdnet_amd.set_precision('fp32')
    try:
        kw, dil, shape = tr.CASES['small-p0']
        m = fr.randomize(FullNet(**kw), 91).cuda()
        t = FullNetTrainer(m, seed=3, lr=1e-3)
        x, label, weight = (v.cuda() for v in tr.batch(shape, 92))
        losses = [float(t.train_step(x, label, weight)[0].item()) for _ in range(10)]
        t.write_bn_counters()
        torch.cuda.synchronize()
    finally:
        cdnet_amd.set_precision(before)
    return m, losses, x, dil


def test_ten_adam_steps_lower_the_loss():
    m, losses, x, dil = _trained()
    print('losses', ' '.join('%.4f' % v for v in losses))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert int(m.conv1.bn.num_batches_tracked) == 10


def test_eval_after_training_uses_the_trained_weights_and_statistics(fp32_mode):
    """stale packs or running statistics that were never written would show here: the eval-mode logits against the inference mirror on the
    trained state dict, within three inference envelopes (the rule of tests/test_gpu_fullnet.py)"""
    import torch
    import _fullnet_ref as fr
    import _fullnet_train_ref as tr
    m, losses, x, dil = _trained()
    m.eval()
    with torch.no_grad():
        got = m(x).cpu().double()
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    xc = x.cpu()
    want = fr.forward(sd, xc, dil)
    scale = float(want.abs().max())
    env = float((fr.forward(fr.perturbed(sd, 93), xc, dil) - want).abs().max()) / scale
    err = float((got - want).abs().max()) / scale
    print('eval after training: err %.3e, envelope %.3e, ratio %.2f' % (err, env, err / env))
    assert err <= 3 * env, (err, env)
    # the running statistics moved away from their initial values
    init = fr.randomize(type(m)(**tr.CASES['small-p0'][0]), 91).state_dict()
    assert not torch.equal(init['conv1.bn.running_mean'], sd['conv1.bn.running_mean'])
    assert not torch.equal(init['conv2.weight'], sd['conv2.weight'])


def test_same_seed_gives_the_same_bits(fp32_mode):
    import torch
    import _fullnet_ref as fr
    import _fullnet_train_ref as tr
    from cdnet_amd.models.FullNet import FullNet
    from cdnet_amd.trainer import FullNetTrainer
    kw, dil, shape = tr.CASES['small-p0.1']
    x, label, weight = (v.cuda() for v in tr.batch(shape, 95))
    flats = []
    for _ in range(2):
        t = FullNetTrainer(fr.randomize(FullNet(**kw), 94).cuda(), seed=11)
        for _ in range(2):
            t.train_step(x, label, weight)
        torch.cuda.synchronize()
        flats.append(t.flat.P.clone())
    assert torch.equal(flats[0].view(torch.int32), flats[1].view(torch.int32))
    # and another seed draws other masks
    t = FullNetTrainer(fr.randomize(FullNet(**kw), 94).cuda(), seed=12)
    for _ in range(2):
        t.train_step(x, label, weight)
    assert not torch.equal(t.flat.P, flats[0])


def test_bf16_mode_is_refused():
    import cdnet_amd
    import _fullnet_ref as fr
    from cdnet_amd.models.FullNet import FullNet
    from cdnet_amd.trainer import FullNetTrainer
    before = cdnet_amd.get_precision()
    cdnet_amd.set_precision('bf16')
    try:
        with pytest.raises(NotImplementedError, match='fp32 precision mode'):
            FullNetTrainer(FullNet(**fr.SMALL).cuda())
    finally:
        cdnet_amd.set_precision(before)
