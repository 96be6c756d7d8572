"""ImageNet encoder weights and encoder_freeze on the device (2 x 3 x 64 x 64 inputs, the shape of the training-entry tests).

  * a torchvision-layout file loaded into UNet_vgg16, eval forward against the plain-PyTorch mirror (tests/_backbone_unet_ref.py) under
    the bars tests/test_gpu_backbone_unet.py applies to that comparison; the same load into a model that already ran, and into one whose
    parameters are views of a trainer's flat buffer, gives the same bits (packs and BatchNorm folds are rebuilt);
  * one frozen training step against one unfrozen step from the same start: losses, every non-backbone gradient and stepped parameter
    bit-equal, the backbone's weights untouched, its running statistics tracked as in the unfrozen run;
  * the calls: the same forward list, and in backward not one call that names a backbone gradient, no backward-data pack for a backbone layer;
  * three frozen steps + save + load + two == five frozen steps, model and optimiser entry bit for bit;
  * the training entry with --pretrained-path and --encoder-freeze 1."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def precision(request):
    import cdnet_amd
    before = cdnet_amd.get_precision()
    cdnet_amd.set_precision(request.param)
    yield request.param
    cdnet_amd.set_precision(before)


def _torchvision_file(backbone, path):
    import torch
    sd = {'features.' + k: v.detach().clone() for k, v in backbone.state_dict().items()}
    for i in (0, 3, 6):
        sd['classifier.%d.weight' % i], sd['classifier.%d.bias' % i] = torch.zeros(2, 2), torch.zeros(2)
    torch.save(sd, path)
    return sd


# ---- the loader ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['fp32', 'bf16'], indirect=True)
def test_eval_forward_after_loading_a_torchvision_file(precision, tmp_path):
    import torch
    import _backbone_unet_ref as br
    from cdnet_amd import checkpoint, synth, trainer
    from cdnet_amd.models.model_unet import Unet
    from test_gpu_model import _check
    ref = br.det_model().eval()
    path = str(tmp_path / 'vgg16_bn-synthetic.pth')
    _torchvision_file(ref.backbone, path)

    def other_encoder():
        """the mirror's decoder and classifier around a random encoder with moved BatchNorm buffers"""
        torch.manual_seed(11)
        m = Unet(backbone_name='vgg16_bn', pretrained=False, classes=3)
        sd = m.state_dict()
        for k, v in ref.state_dict().items():
            if not k.startswith('backbone.'):
                sd[k] = v
            elif k.endswith('running_mean'):
                sd[k] = torch.full_like(v, 0.25)
        m.load_state_dict(sd)
        return m.cuda().eval()
    x = torch.from_numpy(synth.det_input((2, 3, 64, 64), 1))
    with torch.no_grad():
        want = ref(x).numpy()
        m = other_encoder()
        rep = checkpoint.load_backbone_weights(m, path)
        got = m(x.cuda())
        assert len(rep['loaded']) == 13 * 7 and len(rep['dropped']) == 6
        scale = np.abs(want).max()
        err = np.abs(got.cpu().numpy() - want)
        print('UNet_vgg16 eval after load %s: max %.3g mean %.3g of the scale %.3g' % (precision, err.max() / scale, err.mean() / scale, scale))
        if precision == 'bf16':
            _check(got, want, 'UNet_vgg16 eval after load')
        else:
            assert err.max() <= 5e-4 * scale, (err.max(), scale)
        # a model that has already run an eval forward: its packs and folds are of the other encoder
        m2 = other_encoder()
        before = m2(x.cuda())
        assert not torch.equal(before, got)
        checkpoint.load_backbone_weights(m2, path)
        assert torch.equal(m2(x.cuda()), got)
        # a model with a trainer: the parameters are views of FlatState.P and the copy lands there
        m3 = other_encoder()
        tr = trainer.BackboneUNetTrainer(m3)
        m3.eval()
        m3(x.cuda())
        checkpoint.load_backbone_weights(m3, path)
        off, n = tr.flat.offsets['backbone.0.weight']
        assert torch.equal(tr.flat.P[off:off + n].cpu(), ref.backbone[0].weight.detach().reshape(-1))
        assert torch.equal(m3(x.cuda()), got)


# ---- frozen against unfrozen step ------------------------------------------------------------------------------------------------
def _model(kind, freeze, seed=0):
    import importlib
    import torch
    mod = {'rev1': 'cdnet_amd.models.dam.model_unet_rev1', 'MandD': 'cdnet_amd.models.dam.model_unet_MandD',
           'plain': 'cdnet_amd.models.model_unet'}[kind]
    torch.manual_seed(seed)
    m = importlib.import_module(mod).Unet(backbone_name='vgg16_bn', pretrained=False, encoder_freeze=freeze, classes=3)
    for k in m.modules():
        if isinstance(k, torch.nn.BatchNorm2d):
            torch.nn.init.uniform_(k.weight, 0.5, 1.5)
            torch.nn.init.normal_(k.bias, 0, 0.2)
    return m.cuda()


def _batch(kind, seed=21):
    import torch
    from cdnet_amd import synth
    lab, dirn, point, weight = synth.train_targets(2, 64, 64, seed)
    x = torch.from_numpy(synth.det_input((2, 3, 64, 64), 9))
    t = [torch.from_numpy(a).cuda() for a in (lab, dirn, point, weight[:, 0].copy())]
    return (x.cuda(), t[0], t[3]) if kind == 'plain' else (x.cuda(), t[0], t[1], t[2], t[3])


def _trainer(m, **kw):
    from cdnet_amd import utils
    return utils.trainer_class(m)(m, weight_decay=1e-4, **kw)


def _fwd_bwd(tr, batch):
    out = tr.forward(batch[0])
    if len(batch) == 3:
        tr.backward(tr.loss_and_grads(out, *batch[1:]))
        return tr.unet_losses
    if type(tr).__name__ == 'AblationTrainer':                    # (takes the model's output tuple whole: two or three logits)
        g = tr.loss_and_grads(out, *batch[1:])
    else:
        g = tr.loss_and_grads(out[0], out[1], out[2], *batch[1:])
    tr.backward(*g)
    return tr.losses


def _step(kind, freeze):
    """one step from seed 0: losses, gradients, initial and stepped parameters, buffers"""
    import torch
    m = _model(kind, freeze)
    p0 = {n: p.detach().clone() for n, p in m.named_parameters()}
    tr = _trainer(m)
    losses = _fwd_bwd(tr, _batch(kind)).clone()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in m.named_parameters()}
    tr.allreduce_and_step()
    torch.cuda.synchronize()
    return dict(m=m, tr=tr, losses=losses, grads=grads, p0=p0, p1={n: p.detach().clone() for n, p in m.named_parameters()},
                bufs={n: b.detach().clone() for n, b in m.named_buffers()})


def _bits(a, b):
    import torch
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize('kind,precision', [('rev1', 'fp32'), ('MandD', 'fp32'), ('plain', 'fp32'), ('rev1', 'bf16')], indirect=['precision'])
def test_frozen_step_equals_unfrozen_step_outside_the_encoder(kind, precision):
    import torch
    u, u2, f = _step(kind, False), _step(kind, False), _step(kind, True)
    m = f['m']
    unused = tuple(m.UNUSED_PREFIXES)
    names = [n for n in f['p0'] if not n.startswith(unused)]
    enc = [n for n in names if n.startswith('backbone.')]
    dec = [n for n in names if not n.startswith('backbone.')]
    assert len(enc) == 52 and f['tr'].flat.frozen == enc and f['tr'].flat.n_used == sum(f['p0'][n].numel() for n in dec)
    assert all(_bits(u['p0'][n], f['p0'][n]) for n in f['p0'])                       # the same start
    # the unfrozen step against itself: what is bit-stable on this box (everything is expected to be)
    unstable = [n for n in names if not _bits(u['grads'][n], u2['grads'][n]) or not _bits(u['p1'][n], u2['p1'][n])]
    print('%s %s: %d of %d tensors differ between two unfrozen runs %s' % (kind, precision, len(unstable), len(names), unstable[:4]))
    assert _bits(u['losses'], f['losses']), (u['losses'], f['losses'])
    for n in dec:
        if n in unstable:
            for key in ('grads', 'p1'):
                tol = float((u[key][n] - u2[key][n]).abs().max())
                assert float((u[key][n] - f[key][n]).abs().max()) <= tol, (key, n)
            continue
        assert _bits(u['grads'][n], f['grads'][n]), 'gradient of ' + n
        assert _bits(u['p1'][n], f['p1'][n]), 'stepped ' + n
        assert not _bits(f['p0'][n], f['p1'][n]) or float(f['grads'][n].abs().max()) == 0.0, n + ' did not move'
    for n in enc:
        assert _bits(f['p0'][n], f['p1'][n]), n + ' moved'                          # no step, no weight decay
        assert float(f['grads'][n].abs().max()) == 0.0, n + ' received a gradient'
        assert not _bits(u['p0'][n], u['p1'][n]), n                                  # (the unfrozen encoder does train)
    assert not any(unstable), unstable
    # statistics are still tracked: every running_mean / running_var as in the unfrozen run
    stats = [n for n in f['bufs'] if n.endswith(('running_mean', 'running_var')) and not n.startswith(unused)]
    assert len([n for n in stats if n.startswith('backbone.')]) == 26
    for n in stats:
        assert _bits(u['bufs'][n], f['bufs'][n]), n
    assert float(f['bufs']['backbone.1.running_mean'].abs().max()) > 0.0
    # no moments for the frozen block, and the optimiser entry has state for the stepped parameters only
    fl = f['tr'].flat
    assert float(fl.M[fl.n_used:].abs().max()) == 0.0 and float(fl.V[fl.n_used:].abs().max()) == 0.0
    sd = f['tr'].state_dict()
    order = [n for n, _ in m.named_parameters()]
    assert {order[i] for i in sd['state']} == set(dec) and sd['param_groups'][0]['params'] == list(range(len(order)))
    with pytest.raises(RuntimeError, match='freeze first'):
        u['m'].freeze_encoder()


# ---- the calls -------------------------------------------------------------------------------------------------------------------
def _pointers(args):
    import ctypes as C
    out = []
    for a in args:
        if isinstance(a, C.c_void_p) and a.value:
            out.append(a.value)
        elif isinstance(a, int) and a > (1 << 32):
            out.append(a)
    return out


def _recorded_step(kind, freeze, monkeypatch):
    import torch
    from cdnet_amd import _lib
    m = _model(kind, freeze)
    tr = _trainer(m)
    batch = _batch(kind)
    calls, phase = [], ['forward']
    real = _lib.call

    def call(name, *args):
        calls.append((phase[0], name, _pointers(args)))
        return real(name, *args)
    monkeypatch.setattr(_lib, 'call', call)
    out = tr.forward(batch[0])
    phase[0] = 'loss'
    if len(batch) == 3:
        g = (tr.loss_and_grads(out, *batch[1:]),)
    else:
        g = tr.loss_and_grads(out[0], out[1], out[2], *batch[1:])
    phase[0] = 'backward'
    tr.backward(*g)
    torch.cuda.synchronize()
    monkeypatch.setattr(_lib, 'call', real)
    return m, tr, calls


@pytest.mark.parametrize('kind,precision', [('rev1', 'fp32'), ('plain', 'bf16')], indirect=['precision'])
def test_frozen_backward_issues_no_call_for_the_encoder(kind, precision, monkeypatch):
    mu, tru, cu = _recorded_step(kind, False, monkeypatch)
    mf, trf, cf = _recorded_step(kind, True, monkeypatch)
    names = lambda calls, ph: [n for p, n, _ in calls if p == ph]
    assert names(cf, 'forward') == names(cu, 'forward') and len(names(cf, 'forward')) > 40          # the forward does not change
    assert names(cf, 'loss') == names(cu, 'loss')

    def grad_range(tr, m):
        offs = [tr.flat.offsets[n] for n, _ in m.named_parameters() if n.startswith('backbone.')]
        lo, hi = min(o for o, _ in offs), max(o + s for o, s in offs)
        assert hi - lo == sum(s for _, s in offs)                          # one contiguous block of the flat buffers
        return tr.flat.G.data_ptr() + 4 * lo, tr.flat.G.data_ptr() + 4 * hi

    def touching(calls, rng):
        return [n for p, n, ptrs in calls if p == 'backward' and any(rng[0] <= q < rng[1] for q in ptrs)]
    hit_u, hit_f = touching(cu, grad_range(tru, mu)), touching(cf, grad_range(trf, mf))
    # unfrozen: 13 weight-gradient launches, their deferred reduce descriptors and the BatchNorm-backward calls of 13 layers name a
    # backbone gradient; frozen: not one call does
    assert hit_u.count('cdnet_conv_backward_weight') == 13 and sum(n.startswith('cdnet_bn_backward') for n in hit_u) >= 13
    assert hit_f == [], hit_f
    bu, bf = names(cu, 'backward'), names(cf, 'backward')
    gone = {n: bu.count(n) - bf.count(n) for n in sorted(set(bu))}
    print('%s %s: %d -> %d backward calls; gone: %s' % (kind, precision, len(bu), len(bf), {n: c for n, c in gone.items() if c}))
    print('backward-data launches that stop at the live channels:', trf.narrowed)
    assert sorted(trf.narrowed) == ['upsample_blocks.%d.conv2' % k for k in range(5)] and tru.narrowed == {}
    assert all(c >= 0 for c in gone.values()) and set(bf) <= set(bu)       # a subset of the unfrozen step's launches
    assert gone['cdnet_conv_backward_weight'] == 13
    # backward-data: 12 encoder layers (the stem never had one) and the first decoder block's transposed convolution
    assert gone['cdnet_conv_forward'] == 13
    enc_u = [L for k, L, _ in mu._rt['enc'] if k == 'conv']
    enc_f = [L for k, L, _ in mf._rt['enc'] if k == 'conv']
    assert all(L.wpb is not None for L in enc_u[1:]) and all(L.wpb is None for L in enc_f)          # no pack-for-backward either
    assert mf._rt['dec'][0][0].wpb is None and all(up.wpb is not None for up, _ in mf._rt['dec'][1:])
    assert all(c2.wpb is not None for _, c2 in mf._rt['dec'])


# ---- resume ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['fp32'], indirect=True)
def test_frozen_run_resumes_bit_identically(precision, tmp_path):
    import torch
    from cdnet_amd import checkpoint
    batches = [_batch('rev1', seed=30 + k) for k in range(5)]

    def run(m, tr, ks):
        for k in ks:
            tr.train_step(*batches[k])
        torch.cuda.synchronize()
    m5 = _model('rev1', True)
    t5 = _trainer(m5)
    run(m5, t5, range(5))
    m3 = _model('rev1', True)
    t3 = _trainer(m3)
    run(m3, t3, range(3))
    path = checkpoint.save_checkpoint(checkpoint.make_state(m3, t3, 0), 0, False, str(tmp_path), 'Main', 0)
    m2 = _model('rev1', True, seed=5)                                       # a fresh frozen model from another seed
    t2 = _trainer(m2)
    checkpoint.load_checkpoint(path, m2, t2)
    assert t2.flat.step_count == 3
    run(m2, t2, (3, 4))
    a, b = checkpoint.make_state(m5, t5, 0), checkpoint.make_state(m2, t2, 0)
    assert list(a['state_dict']) == list(b['state_dict'])
    for k, v in a['state_dict'].items():
        assert torch.equal(v, b['state_dict'][k]), k
    assert int(a['state_dict']['module.backbone.1.num_batches_tracked']) == 5
    assert sorted(a['optimizer']['state']) == sorted(b['optimizer']['state']) and a['optimizer']['param_groups'] == b['optimizer']['param_groups']
    for i, st in a['optimizer']['state'].items():
        for key, v in st.items():
            assert torch.equal(torch.as_tensor(v), torch.as_tensor(b['optimizer']['state'][i][key])), (i, key)
    enc0 = {n: p.detach().cpu() for n, p in _model('rev1', True).named_parameters() if n.startswith('backbone.')}
    assert all(torch.equal(a['state_dict']['module.' + n], v) for n, v in enc0.items())       # five steps later: the initial encoder


# ---- graph capture -----------------------------------------------------------------------------------------------------------------
def test_graphed_frozen_step_is_bit_identical_to_eager():
    """graphs.GraphedTrainStep captures whatever the walk issues: the shorter walk of a frozen model replays to the eager step's bits"""
    import torch
    from cdnet_amd.graphs import GraphedTrainStep
    batch = _batch('rev1')

    def run(graphed, steps=5):
        m = _model('rev1', True)
        tr = _trainer(m)
        if graphed:
            g = GraphedTrainStep(tr, batch, warmup=3)            # 3 eager steps + the first replayed one
            for _ in range(steps - 4):
                g(*batch)
        else:
            for _ in range(steps):
                tr.train_step(*batch)
        torch.cuda.synchronize()
        return tr.flat.P.clone(), tr.losses.clone(), m.state_dict()['backbone.1.running_mean'].clone(), tr._forwards
    p0, l0, rm0, f0 = run(False)
    p1, l1, rm1, f1 = run(True)
    assert torch.equal(p0, p1) and torch.equal(l0, l1) and torch.equal(rm0, rm1) and f0 == f1 == 5


# ---- the training entry ----------------------------------------------------------------------------------------------------------
def test_entry_point_with_pretrained_path_and_encoder_freeze(tmp_path):
    import torch
    from cdnet_amd import train
    from cdnet_amd.models.dam.model_unet_rev1 import vgg16_bn_features
    torch.manual_seed(123)
    enc = vgg16_bn_features()
    path = str(tmp_path / 'vgg16_bn-synthetic.pth')
    sd = _torchvision_file(enc, path)
    d = str(tmp_path / 'run')
    res = train.main(['--synthetic', '4', '--epochs', '1', '--batch-size', '2', '--pretrained-path', path, '--encoder-freeze', '1', '--save-dir', d])
    assert len(res) == 11 and np.isfinite(res).all()
    ck = torch.load(os.path.join(d, 'checkpoints', 'checkpoint.pth.tar'), map_location='cpu', weights_only=False)
    got = ck['state_dict']
    n = 0
    for k, v in sd.items():
        if k.startswith('features.') and k.endswith(('.weight', '.bias')):
            assert torch.equal(got['module.backbone.' + k[len('features.'):]], v), k
            n += 1
    assert n == 52
    assert not torch.equal(got['module.backbone.1.running_mean'], sd['features.1.running_mean'])      # statistics were tracked
    # the decoder trained: optimiser state for the stepped parameters only
    names =[k for k in got if not k.endswith(('running_mean', 'running_var', 'num_batches_tracked'))]
    stepped = {names[i][len('module.'):] for i in ck['optimizer']['state']}
    assert stepped and not any(s.startswith('backbone.') for s in stepped) and 'upsample_blocks.0.up.weight' in stepped
    assert all(int(s['step']) == 4 for s in ck['optimizer']['state'].values())
