"""ImageNet encoder weights and encoder_freeze, CPU side: checkpoint.load_backbone_weights on hand-built torchvision-layout dicts (the
shapes of the model's own backbone; tiny dummy classifier entries, which are dropped unread), `pretrained` = False / True / path in the
constructors, the two training options through chooseModel, and optim.FlatState / optim.stepper of a frozen model on CPU buffers.
No test looks for a real weights file."""
import copy
import logging
import os
import types

import pytest
import torch

from cdnet_amd import checkpoint, optim, utils
from cdnet_amd.models.dam.model_unet_rev1 import Unet, vgg16_bn_features
from cdnet_amd.options import Options

BUFFERS = ('weight', 'bias', 'running_mean', 'running_var', 'num_batches_tracked')


@pytest.fixture(scope='module')
def features():
    """the state of a second, differently seeded encoder with non-trivial BatchNorm buffers: 'N.*' keys (the bare .features layout)"""
    g = torch.Generator().manual_seed(77)
    sd = {}
    for k, v in vgg16_bn_features().state_dict().items():
        if k.endswith('num_batches_tracked'):
            sd[k] = torch.tensor(1000 + int(k.split('.')[0]))
        elif k.endswith('running_var'):
            sd[k] = torch.rand(v.shape, generator=g) + 0.5
        else:
            sd[k] = torch.randn(v.shape, generator=g) * 0.05
    return sd


def torchvision_layout(features):
    sd = {'features.' + k: v for k, v in features.items()}
    for i in (0, 3, 6):                                # the real classifier.0.weight is 411 MB: tiny stand-ins, dropped unread
        sd['classifier.%d.weight' % i] = torch.zeros(2, 2)
        sd['classifier.%d.bias' % i] = torch.zeros(2)
    return sd


def fresh(seed=3, cls=Unet, **kw):
    torch.manual_seed(seed)
    return cls(backbone_name='vgg16_bn', pretrained=kw.pop('pretrained', False), classes=3, **kw)


def same_state(a, b):
    a, b = a.state_dict(), b.state_dict()
    return list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_three_layouts_load_the_same_backbone_and_nothing_else(features, tmp_path):
    base = fresh()
    before = copy.deepcopy(base.state_dict())
    states = []
    path = str(tmp_path / 'vgg16_bn-synthetic.pth')
    torch.save(torchvision_layout(features), path)
    for source in (torchvision_layout(features), dict(features), {'backbone.' + k: v for k, v in features.items()}, path):
        m = fresh()
        rep = checkpoint.load_backbone_weights(m, source)
        states.append(m.state_dict())
        assert sorted(rep['loaded']) == sorted('backbone.' + k for k in features)
        assert sorted(rep['dropped']) == sorted(k for k in (source if isinstance(source, dict) else torchvision_layout(features))
                                                if k.startswith('classifier.'))
        assert rep['missing'] == [] and rep['zeroed'] == []
    for sd in states:
        for k, v in sd.items():
            if k.startswith('backbone.'):
                assert torch.equal(v, features[k[len('backbone.'):]]), k          # every buffer, num_batches_tracked included
            else:
                assert torch.equal(v, before[k]), k                               # nothing outside backbone. moved
    assert int(states[0]['backbone.1.num_batches_tracked']) == 1001
    assert {k.rsplit('.', 1)[1] for k in states[0] if k.startswith('backbone.')} == set(BUFFERS)


@pytest.mark.parametrize('case', ['missing', 'misshaped', 'unknown', 'one_counter_missing'])
def test_strict_errors_name_the_key_and_leave_the_model_untouched(features, case):
    sd = torchvision_layout(features)
    if case == 'missing':
        del sd['features.7.weight']
        named = 'backbone.7.weight'
    elif case == 'misshaped':
        sd['features.10.weight'] = torch.zeros(128, 64, 3, 3)
        named = 'features.10.weight'
    elif case == 'unknown':
        sd['avgpool.weight'] = torch.zeros(1)
        named = 'avgpool.weight'
    else:
        del sd['features.4.num_batches_tracked']
        named = 'backbone.4.num_batches_tracked'
    m = fresh()
    before = copy.deepcopy(m.state_dict())
    with pytest.raises(ValueError) as e:
        checkpoint.load_backbone_weights(m, sd)
    assert named in str(e.value)
    after = m.state_dict()
    assert all(torch.equal(after[k], before[k]) for k in before)
    # without strict the rest loads and the report says what was left
    rep = checkpoint.load_backbone_weights(m, sd, strict=False)
    if case in ('missing', 'one_counter_missing'):
        assert rep['missing'] == [named] and torch.equal(m.state_dict()[named], before[named])
    elif case == 'misshaped':
        assert rep['missing'] == ['backbone.10.weight']
    else:
        assert 'avgpool.weight' in rep['dropped'] and rep['missing'] == []
    assert torch.equal(m.state_dict()['backbone.0.weight'], features['0.weight'])


def test_file_from_before_batchnorm_counters_loads_with_zero_counters(features):
    """nn.BatchNorm2d reads a state without any num_batches_tracked as zero counters (its version-1 rule); so does the loader"""
    sd = {k: v for k, v in torchvision_layout(features).items() if not k.endswith('num_batches_tracked')}
    m = fresh()
    m.backbone[1].num_batches_tracked.fill_(5)
    rep = checkpoint.load_backbone_weights(m, sd)
    assert len(rep['zeroed']) == 13 and int(m.backbone[1].num_batches_tracked) == 0
    assert torch.equal(m.backbone[1].running_var, features['1.running_var'])


def test_pretrained_true_searches_the_cache_layout_and_never_fails(features, tmp_path, monkeypatch, caplog):
    monkeypatch.chdir(tmp_path)
    with caplog.at_level(logging.INFO):
        m = fresh(pretrained=True)
    lines = [r for r in caplog.records if r.name.startswith('cdnet_amd')]
    assert len(lines) == 1 and lines[0].levelno == logging.WARNING
    msg = lines[0].getMessage()
    assert 'pretrained_models/vgg16_bn/hub/checkpoints' in msg and 'pretrained_models/vgg16_bn/checkpoints' in msg and 'random' in msg
    assert same_state(m, fresh(pretrained=False))                         # the same numbers as before under the same seed
    # the second place searched, then the first one wins
    for sub, shift in (('pretrained_models/vgg16_bn/checkpoints', 0.0), ('pretrained_models/vgg16_bn/hub/checkpoints', 1.0)):
        os.makedirs(sub)
        sd = torchvision_layout(features)
        sd['features.0.bias'] = features['0.bias'] + shift
        torch.save(sd, os.path.join(sub, 'vgg16_bn-0123abcd.pth'))
        caplog.clear()
        with caplog.at_level(logging.INFO):
            m = fresh(pretrained=True)
        assert torch.equal(m.backbone[0].bias.detach(), features['0.bias'] + shift)
        assert torch.equal(m.backbone[40].weight.detach(), features['40.weight'])
        assert any(sub in r.getMessage() for r in caplog.records)
    assert same_state(fresh(pretrained=False), fresh(pretrained=0))


def test_pretrained_path_loads_and_a_missing_path_raises(features, tmp_path):
    from cdnet_amd.models.model_unet import Unet as BackboneUnet
    from cdnet_amd.models.dam.model_unet_MandD import Unet as MandD
    path = str(tmp_path / 'enc.pth')
    torch.save(torchvision_layout(features), path)
    for cls in (Unet, BackboneUnet, MandD):
        m = fresh(cls=cls, pretrained=path)
        assert torch.equal(m.backbone[0].weight.detach(), features['0.weight'])
        assert torch.equal(m.backbone[41].running_mean, features['41.running_mean'])
        with pytest.raises(FileNotFoundError):
            fresh(cls=cls, pretrained=str(tmp_path / 'nowhere.pth'))


def test_options_reach_the_model_through_chooseModel(features, tmp_path, monkeypatch, caplog):
    monkeypatch.chdir(tmp_path)
    path = str(tmp_path / 'enc.pth')
    torch.save(torchvision_layout(features), path)
    for name in ('UNet2RevA1_vgg16', 'UNet_vgg16', 'model_unet_MandD'):
        opt = Options(isTrain=True).parse(['--model-name', name, '--pretrained-path', path, '--encoder-freeze', '1'])
        assert opt.model['pretrained_path'] == path and opt.model['encoder_freeze'] == 1
        m = utils.chooseModel(opt)
        assert torch.equal(m.backbone[0].weight.detach(), features['0.weight'])
        assert {n for n, p in m.named_parameters() if not p.requires_grad} == {n for n, _ in m.named_parameters() if n.startswith('backbone.')}
    opt = Options(isTrain=True).parse([])
    assert opt.model['pretrained_path'] == '' and opt.model['encoder_freeze'] == 0
    assert all(p.requires_grad for p in utils.chooseModel(opt).parameters())
    # the test entries load a checkpoint over the model: no search (a file in the cache layout is not read, nothing is logged)
    os.makedirs('pretrained_models/vgg16_bn/hub/checkpoints')
    torch.save(torchvision_layout(features), 'pretrained_models/vgg16_bn/hub/checkpoints/vgg16_bn-0123abcd.pth')
    caplog.clear()
    with caplog.at_level(logging.INFO):
        torch.manual_seed(5)
        m = utils.chooseModel(Options(isTrain=False).parse([]))
    assert not [r for r in caplog.records if r.name.startswith('cdnet_amd')]
    assert same_state(m, fresh(seed=5))
    torch.manual_seed(5)
    assert torch.equal(utils.chooseModel(Options(isTrain=True).parse([])).backbone[0].weight.detach(), features['0.weight'])


def test_parameter_partition_follows_the_reference_rule():
    m = fresh()
    pre, rnd = list(m.get_pretrained_parameters()), list(m.get_random_initialized_parameters())
    assert iter(m.get_pretrained_parameters()) is not None and not isinstance(m.get_pretrained_parameters(), (list, tuple))
    named = dict(m.named_parameters())
    assert [id(p) for p in pre] == [id(p) for n, p in named.items() if n.startswith('backbone.')]
    assert [id(p) for p in rnd] == [id(p) for n, p in named.items() if not n.startswith('backbone.')]
    assert len(pre) + len(rnd) == len(named) and len(pre) == 52


@pytest.mark.parametrize('rule', ['adam', 'sgd', 'ranger'])
def test_flat_state_keeps_frozen_parameters_out_of_the_step(rule):
    m = fresh(encoder_freeze=True)
    named = dict(m.named_parameters())
    flat = optim.FlatState(m, rule)
    frozen = [n for n in named if n.startswith('backbone.')]
    unused = [n for n in named if n.startswith(m.UNUSED_PREFIXES)]
    head = list(optim.HEAD_PARAMS)
    rest = [n for n in named if n not in head and n not in frozen and n not in unused]
    assert flat.order == head + rest + frozen + unused and flat.frozen == frozen
    assert flat.n_head == 855 and flat.n_used == sum(named[n].numel() for n in head + rest)
    lo, hi = flat.offsets[frozen[0]][0], sum(flat.offsets[frozen[-1]])
    assert lo == flat.n_used and hi - lo == sum(named[n].numel() for n in frozen)
    assert flat.S is None or flat.S.numel() == flat.n_used               # no slow weights for the frozen block
    assert all(named[n].data_ptr() == flat.P.data_ptr() + 4 * flat.offsets[n][0] for n in named)       # the parameters are views
    g = torch.Generator().manual_seed(1)
    flat.G.copy_(torch.randn(flat.G.shape, generator=g))                 # non-zero gradients everywhere, the frozen range included
    flat.M.copy_(torch.randn(flat.M.shape, generator=g) * 0.01)
    if flat.V is not None:
        flat.V.copy_(torch.rand(flat.V.shape, generator=g) * 0.01)
    keep = [None if t is None else t.clone() for t in (flat.P, flat.M, flat.V)]
    tr = types.SimpleNamespace(flat=flat, optimizer=rule, lr=1e-2, wd=1e-2, betas=(0.9, 0.99), eps=None if rule != 'adam' else 1e-8,
                               momentum=0.95, dev=flat.P.device)
    if rule == 'ranger':
        tr.eps = optim.RANGER_EPS
    flat.step_count = 6                                                  # (Ranger's lookahead step: the slow weights move too)
    optim.stepper(tr, 1.0)(0, flat.n_used)
    for now, was in zip((flat.P, flat.M, flat.V), keep):
        if now is None:
            continue
        assert torch.equal(now[flat.n_used:], was[flat.n_used:])         # frozen (and never-used) range: bit-unchanged
        assert not torch.equal(now[:flat.n_used], was[:flat.n_used])
    assert (flat.P[:flat.n_used] != keep[0][:flat.n_used]).float().mean() > 0.99
    # an unfrozen model keeps the layout it had
    flat0 = optim.FlatState(fresh(), rule)
    assert flat0.frozen == [] and flat0.order == head + [n for n in named if n not in head and n not in unused] + unused


def test_optimizer_state_lists_every_parameter_and_holds_state_for_stepped_ones_only():
    m = fresh(encoder_freeze=True)
    flat = optim.FlatState(m, 'adam')
    flat.step_count = 2
    tr = types.SimpleNamespace(flat=flat, model=m, optimizer='adam', lr=1e-3, wd=1e-4, betas=(0.9, 0.99), eps=1e-8, momentum=0.95)
    sd = optim.state_dict(tr)
    names = [n for n, _ in m.named_parameters()]
    assert sd['param_groups'][0]['params'] == list(range(len(names)))
    stepped = {names[i] for i in sd['state']}
    assert stepped == {n for n in names if not n.startswith('backbone.') and not n.startswith(m.UNUSED_PREFIXES)}
    flat.M.fill_(1.0)
    optim.load_state_dict(tr, sd)                                        # round trip: the stepped range from the entry, zeros elsewhere
    assert float(flat.M.abs().sum()) == 0.0 and flat.step_count == 2
    bad = copy.deepcopy(sd)
    bad['state'][names.index('backbone.0.weight')] = bad['state'][names.index('upsample_blocks.0.up.weight')]
    with pytest.raises(AssertionError):
        optim.load_state_dict(tr, bad)


def test_freeze_after_a_trainer_exists_raises():
    m = fresh()
    m._trainer_bound = True                                              # what Trainer.__init__ leaves (tests/test_gpu_encoder_freeze.py builds one)
    with pytest.raises(RuntimeError, match='freeze first'):
        m.freeze_encoder()
    assert all(p.requires_grad for p in m.parameters())
