"""FCN_pooling on the device (models/FullNet.py on csrc/dilated.hip, csrc/dilated_train.hip and csrc/resample.hip) against the fp64 mirror
tests/_fcn_pooling_ref.py, by the rules of tests/test_gpu_fullnet.py (eval) and tests/test_gpu_fullnet_train.py (one training step).

Eval: max|got - want| / max|want logit| within 3 envelopes - fp32 mode the mirror's own change under a relative 2^-16 U(-1, 1) perturbation
of every weight, bf16 mode the mirror with the convolution weights and every stored map (the upsampled ones included) rounded to bf16.
Training (fp32 mode): per tensor (logits, loss, every gradient, every running statistic) max|got - mirror| / max|mirror| within 3 envelopes
over 32 seeds (the default network: 16) of independent 2^-16 errors at every product site.  The device hands the mirror the LeakyReLU signs, the dropout masks and
the pools' arg-max indices (tools/fullnet_train_envelope.py --net FCN_pooling checks the bar on the CPU)."""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(params=['fp32', 'bf16'])
def precision(request):
    import cdnet_amd
    before = cdnet_amd.get_precision()
    cdnet_amd.set_precision(request.param)
    yield request.param
    cdnet_amd.set_precision(before)


@pytest.fixture
def fp32_mode():
    import cdnet_amd
    before = cdnet_amd.get_precision()
    cdnet_amd.set_precision('fp32')
    yield
    cdnet_amd.set_precision(before)


def _envelopes(sd, x, dil, want, seed):
    """(scale, fp32 envelope, bf16 envelope) of the eval logits"""
    import _fullnet_ref as fr
    import _fcn_pooling_ref as pr
    scale = float(want.abs().max())
    E = float((pr.forward(fr.perturbed(sd, seed), x, dil) - want).abs().max()) / scale
    E16 = float((pr.forward(sd, x, dil, quant=fr.bf16_round) - want).abs().max()) / scale
    return scale, E, E16


@functools.lru_cache(maxsize=None)
def _golden_case():
    import torch
    import _fcn_pooling_ref as pr
    from conftest import GOLDEN
    g = np.load(os.path.join(GOLDEN, 'fcn_pooling.npz'))
    sd = pr.golden_state(g)
    x, want = torch.from_numpy(g['small/x']), torch.from_numpy(g['small/logits64'])
    return (sd, x, want) + _envelopes(sd, x, pr.GOLDEN_DILATIONS, want, 5)


@functools.lru_cache(maxsize=None)
def _default_case():
    import _fullnet_ref as fr
    import _fcn_pooling_ref as pr
    from cdnet_amd.models.FullNet import FCN_pooling
    m = fr.randomize(FCN_pooling(3, 3), 21)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    x = fr.bf16_exact_input((2, 3, 32, 32), 22)
    want = pr.forward(sd, x, fr.DEFAULT_DILATIONS)
    return (sd, x, want) + _envelopes(sd, x, fr.DEFAULT_DILATIONS, want, 23)


@pytest.mark.parametrize('net', ['golden', 'default'])
def test_eval_logits_within_three_envelopes(net, precision):
    """golden: the reference class's own fp64 logits; default: the mirror's"""
    import torch
    import _fcn_pooling_ref as pr
    from cdnet_amd.models.FullNet import FCN_pooling
    sd, x, want, scale, E, E16 = _golden_case() if net == 'golden' else _default_case()
    m = FCN_pooling(**pr.GOLDEN) if net == 'golden' else FCN_pooling(3, 3)
    m.load_state_dict(sd, strict=True)
    with torch.no_grad():
        got = m.cuda().eval()(x.cuda()).cpu().double()
    assert got.shape == want.shape and bool(torch.isfinite(got).all())
    err = float((got - want).abs().max()) / scale
    env = E if precision == 'fp32' else E16
    print('FCN_pooling %s %s: err %.3e of max|logit| %.3g, envelope %.3e, ratio %.2f' % (net, precision, err, scale, env, err / env))
    assert err <= 3 * env, (precision, err, env)


def _mask(key, layer, shape, p):
    import torch
    from cdnet_amd import _lib
    n = int(np.prod(shape))
    m = torch.empty((n,), dtype=torch.uint8, device='cuda')
    _lib.call('cdnet_dropout_mask', key, layer, n, p, _lib.ptr(m), _lib.stream_ptr())
    return m.view(shape).permute(0, 3, 1, 2).bool().cpu()


def _prefixes(model):
    from cdnet_amd.models.FullNet import ConvLayer
    return {id(mod.conv): name for name, mod in model.named_modules() if isinstance(mod, ConvLayer)}


@pytest.mark.parametrize('name', ['golden-p0', 'golden-p0.1', 'default', 'bottleneck'])
def test_one_step_against_the_mirror(name, fp32_mode):
    import torch
    import _fullnet_ref as fr
    import _fullnet_train_ref as tr
    import _fcn_pooling_ref as pr
    from oracle import train as ot
    from cdnet_amd.models.FullNet import FCN_pooling
    from cdnet_amd.trainer import FullNetTrainer
    kw, dil, shape = pr.CASES[name]
    k = list(pr.CASES).index(name)
    m = fr.randomize(FCN_pooling(**kw), 160 + k).cuda()
    t = FullNetTrainer(m, seed=7)
    sd = {n: v.detach().cpu().clone() for n, v in m.state_dict().items()}
    x, label, weight = tr.batch(shape, 170 + k)
    logits = t.forward(x.cuda())
    dl = t.loss_and_grads(logits, label.cuda(), weight.cuda())
    t.backward(dl)
    torch.cuda.synchronize()
    rec = t.tape[-1]
    p = float(kw.get('drop_rate', 0.1))

    # what the device used: LeakyReLU signs, dropout masks, the pools' arg-max positions
    names = _prefixes(m)
    convs = m._convs()
    signs = {names[id(c.conv)]: (rec.z[id(c)][..., :c.Cout] > 0).permute(0, 3, 1, 2).cpu() for c in convs if c.bn is not None}
    drops = {names[id(convs[li].conv)]: _mask(rec.key, li, shp, pd) for li, shp, pd in rec.drops}
    want_drops = [pre for pre, _, last in tr.conv_prefixes(sd, dil) if last] if p > 0 else []
    assert sorted(drops) == sorted(want_drops)
    assert sorted(rec.pool_idx) == [0, 1, 2, 3]
    pools = {}
    for i, idx in rec.pool_idx.items():
        c = m._rt[1][i][1].Cout
        pools['blocks.pool%d' % (i + 1)] = idx[..., :c].permute(0, 3, 1, 2).cpu().long()
        assert tuple(idx.shape[1:3]) == (shape[2] >> (i + 1), shape[3] >> (i + 1)) and int(idx[..., :c].max()) <= 3
    # map sizes per block: H, H/2, H/4, H/8, H/16, H/4, H (and the dropout records follow them)
    assert [tuple(b.shape[1:3]) for b in rec.bufs] == [(shape[2] // d, shape[3] // d) for d in (1, 2, 4, 8, 16, 4, 1, 1)]

    got = {'logits': logits.cpu().double(), 'loss': t.mask_losses[0:1].cpu().double()}
    got.update({'grad ' + n: q.grad.detach().cpu().double().view(q.shape) for n, q in m.named_parameters()})
    got.update({n: b.detach().cpu().double() for n, b in m.named_buffers() if 'running_' in n})

    loss_fn = lambda lg: ot.unet_losses(lg, label, weight)['total']
    clean, env = pr.envelope(sd, x, dil, signs, drops, p, pools, loss_fn, pr.ENVELOPE_SEEDS[name])
    want = tr.tensors(clean)
    assert sorted(got) == sorted(want)
    rows = []
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
    """the golden network with drop_rate 0 after 10 Adam steps on one fixed batch (fp32 mode): (model, losses, x, dilations)"""
    import torch
    import cdnet_amd
    import _fullnet_ref as fr
    import _fullnet_train_ref as tr
    import _fcn_pooling_ref as pr
    from cdnet_amd.models.FullNet import FCN_pooling
    from cdnet_amd.trainer import FullNetTrainer
    before = cdnet_amd.get_precision()
    cdnet_amd.set_precision('fp32')
    try:
        kw, dil, shape = pr.CASES['golden-p0']
        m = fr.randomize(FCN_pooling(**kw), 191).cuda()
        t = FullNetTrainer(m, seed=3, lr=1e-3)
        x, label, weight = (v.cuda() for v in tr.batch(shape, 192))
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
    import torch
    import _fullnet_ref as fr
    import _fcn_pooling_ref as pr
    m, losses, x, dil = _trained()
    m.eval()
    with torch.no_grad():
        got = m(x).cpu().double()
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    xc = x.cpu()
    want = pr.forward(sd, xc, dil)
    scale = float(want.abs().max())
    env = float((pr.forward(fr.perturbed(sd, 193), xc, dil) - want).abs().max()) / scale
    err = float((got - want).abs().max()) / scale
    print('eval after training: err %.3e, envelope %.3e, ratio %.2f' % (err, env, err / env))
    assert err <= 3 * env, (err, env)
    init = fr.randomize(type(m)(**pr.CASES['golden-p0'][0]), 191).state_dict()
    assert not torch.equal(init['blocks.trans5.bn.running_mean'], sd['blocks.trans5.bn.running_mean'])
    assert not torch.equal(init['conv2.weight'], sd['conv2.weight'])


def test_same_seed_gives_the_same_bits(fp32_mode):
    import torch
    import _fullnet_ref as fr
    import _fullnet_train_ref as tr
    import _fcn_pooling_ref as pr
    from cdnet_amd.models.FullNet import FCN_pooling
    from cdnet_amd.trainer import FullNetTrainer
    kw, dil, shape = pr.CASES['golden-p0.1']
    x, label, weight = (v.cuda() for v in tr.batch(shape, 195))
    flats = []
    for _ in range(2):
        t = FullNetTrainer(fr.randomize(FCN_pooling(**kw), 194).cuda(), seed=11)
        for _ in range(2):
            t.train_step(x, label, weight)
        torch.cuda.synchronize()
        flats.append(t.flat.P.clone())
    assert torch.equal(flats[0].view(torch.int32), flats[1].view(torch.int32))
    t = FullNetTrainer(fr.randomize(FCN_pooling(**kw), 194).cuda(), seed=12)
    for _ in range(2):
        t.train_step(x, label, weight)
    assert not torch.equal(t.flat.P, flats[0])


def test_bf16_mode_training_is_refused():
    import cdnet_amd
    import _fcn_pooling_ref as pr
    from cdnet_amd.models.FullNet import FCN_pooling
    from cdnet_amd.trainer import FullNetTrainer
    before = cdnet_amd.get_precision()
    cdnet_amd.set_precision('bf16')
    try:
        with pytest.raises(NotImplementedError, match='fp32 precision mode'):
            FullNetTrainer(FCN_pooling(**pr.GOLDEN).cuda())
    finally:
        cdnet_amd.set_precision(before)


def test_checkpoint_round_trip_into_the_mirror(tmp_path, fp32_mode):
    """checkpoint.model_state -> file -> checkpoint.load_checkpoint into a fresh model: the same bits; the file's tensors through the
    plain-PyTorch mirror: the same logits within three envelopes"""
    import torch
    import _fullnet_ref as fr
    import _fcn_pooling_ref as pr
    from cdnet_amd import checkpoint
    from cdnet_amd.models.FullNet import FCN_pooling
    a = fr.randomize(FCN_pooling(**pr.GOLDEN), 151).cuda().eval()
    x = fr.bf16_exact_input((1, 3, 32, 32), 152)
    with torch.no_grad():
        want = a(x.cuda())
    state = {'epoch': 3, 'state_dict': checkpoint.model_state(a), 'best_iou': 0.0, 'best_loss': 1.0, 'optimizer': None}
    assert all(k.startswith('module.') for k in state['state_dict'])
    path = str(tmp_path / 'checkpoint_best.pth.tar')
    torch.save(state, path)
    b = FCN_pooling(**pr.GOLDEN).cuda().eval()
    with torch.no_grad():
        assert not torch.equal(b(x.cuda()), want)
    ck = checkpoint.load_checkpoint(path, b)
    assert ck['epoch'] == 3
    with torch.no_grad():
        assert torch.equal(b(x.cuda()).view(torch.int32), want.view(torch.int32))
    sd = {k[len('module.'):]: v.cpu() for k, v in torch.load(path, map_location='cpu')['state_dict'].items()}
    mirror = pr.forward(sd, x, pr.GOLDEN_DILATIONS)
    scale = float(mirror.abs().max())
    env = float((pr.forward(fr.perturbed(sd, 153), x, pr.GOLDEN_DILATIONS) - mirror).abs().max()) / scale
    err = float((want.cpu().double() - mirror).abs().max()) / scale
    print('checkpoint through the mirror: err %.3e, envelope %.3e, ratio %.2f' % (err, env, err / env))
    assert err <= 3 * env


def test_infer_image_mask_with_sliding_windows(precision):
    import torch
    import _fullnet_ref as fr
    import _fcn_pooling_ref as pr
    from cdnet_amd import pipeline, synth, utils
    from cdnet_amd.models.FullNet import FCN_pooling
    m = fr.randomize(FCN_pooling(**pr.GOLDEN), 141).cuda().eval()
    assert pipeline.mask_channels(m) == 3
    img = torch.from_numpy(synth.det_input((3, 96, 80), 8)).cuda()
    r = pipeline.infer_image_mask(m, img, tta=True, all_img_test=0, patch_size=64, overlap=16, model_mode='FCN_pooling')
    assert tuple(r['final'].shape) == (96, 80) and tuple(r['pred'].shape) == (96, 80) and r['final'].dtype == torch.int32
    assert int(r['pred'].max()) <= 2 and r['count'] >= 0
    views = utils.split_forward_views(m, img, 64, 16, (0, 5))
    assert tuple(views[0][0].shape) == (3, 96, 80) and tuple(views[1][0].shape) == (3, 80, 96)
    with pytest.raises(ValueError, match='multiples of 16'):
        utils.split_forward_views(m, img, 72, 16)
