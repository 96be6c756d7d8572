"""The reference's other optimisers on the GPU (csrc/optim.hip: cdnet_moment_step, cdnet_sgd_step) and the schedulers in the training
entry point.

  1. the kernels through the C ABI walk every trajectory of tests/golden/optim*.npz (the reference's own optimiser objects);
  2. `Trainer` with each optimiser, 14 steps on a small DAM network: every step against the host restatement of the rule;
  3. a checkpoint written by the reference at step 7 continues to step 14 on the kernels; state_dict layouts;
  4. `train.main` with --optimizer radam --scheduler StepLR: the rate per epoch, the checkpoint, a resume;
  5. the default Adam path is bit-identical to calling cdnet_adam_step on the same gradients.

The number everywhere is the displacement-relative error || p_t - ref_t || / || ref_t - p_start || with the bar 2e-5
(_optim_cases.BAR); steps that must not move anything are compared exactly."""
import logging
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _optim_cases as oc  # noqa: E402

pytestmark = pytest.mark.gpu
TRAINER_RULES = ('sgd', 'radam', 'radam4s', 'adamw', 'ranger')


@pytest.mark.parametrize('setting', oc.SETTINGS)
@pytest.mark.parametrize('key', oc.RULES)
def test_kernels_walk_the_reference_trajectory(golden, setting, key):
    """the whole trajectory from p0 through the ABI; buffers one element off a 16-byte boundary (scalar head, vector body, tail)"""
    import torch
    case = oc.load_case(golden, setting, key)
    errs, dev = oc.walk(oc.DeviceDriver, case)
    print(setting, key, {t: '%.2e' % e for t, e in errs.items()})
    assert max(errs.values()) <= oc.BAR, errs
    # the kernels and their host restatement do the same operations in the same order: equal bit for bit, for every alignment
    _, host = oc.walk(oc.HostDriver, case)
    for shift in (0, 3):
        _, d2 = oc.walk(oc.DeviceDriver, case, shift=shift)
        assert np.array_equal(d2.params(), host.params()), shift
    assert np.array_equal(dev.params(), host.params()) and np.array_equal(dev.from_buf(dev.m), host.m)
    torch.cuda.synchronize()


@pytest.mark.parametrize('key', ['sgd', 'radam', 'radam4s', 'adamw4k', 'ranger'])
def test_reference_checkpoint_state_continues_on_the_kernels(golden, key):
    """the reference's state after step 7 (what its checkpoint holds) + the parameters of step 7 -> steps 8..14 on the kernels land on
    the reference's parameters of steps 12 and 14"""
    case = oc.load_case(golden, 'default', key)
    st = golden('optim_state')
    pre = 'default/%s/at7/' % key
    state = {k[len(pre):]: st[k] for k in st.files if k.startswith(pre)}
    t7 = case['t0'] + 7
    assert key == 'sgd' or int(state['step']) == t7
    d = oc.DeviceDriver(case['rule'], case['lr'], case['wd'], case['momentum'], case['snaps'][7], t0=t7, state=state)
    errs = {}
    for k in range(7, 14):
        d.step(case['grads'][k])
        if k + 1 in case['snaps']:
            errs[k + 1] = oc.rel_error(d.params(), case['snaps'][k + 1], case['p_start'])
    print(key, errs)
    assert sorted(errs) == [12, 14] and max(errs.values()) <= oc.BAR, errs
    fin = 'default/%s/final/' % key
    mkey = 'momentum_buffer' if key == 'sgd' else 'exp_avg'
    assert oc.rel_error(d.from_buf(d.m), st[fin + mkey], np.zeros_like(st[fin + mkey])) <= oc.BAR
    if key == 'ranger':
        assert oc.rel_error(d.from_buf(d.slow), st[fin + 'slow_buffer'], case['p_start']) <= oc.BAR


def _dam(seed=3):
    import torch
    from cdnet_amd.models.dam.model_unet_rev1 import Unet
    torch.manual_seed(seed)
    return Unet(backbone_name='vgg16_bn', pretrained=False, classes=3).cuda()


def _args(name, scheduler='None'):
    from cdnet_amd.options import Options
    opt = Options(isTrain=True)
    opt.train['optimizer'], opt.train['scheduler'] = name, scheduler
    return opt


@pytest.mark.parametrize('rule', TRAINER_RULES)
def test_trainer_steps_match_the_host_restatement(golden, rule):
    import torch
    from cdnet_amd import trainer, utils
    dev = torch.device('cuda:0')
    m = _dam()
    tr, sched = utils.get_optimizer(_args(rule.upper()), m)
    assert sched is None and type(tr) is trainer.Trainer and tr.optimizer == rule
    f = tr.flat
    n = f.n_used
    assert 0 < n < f.P.numel()
    batch = trainer.synthetic_batch(2, dev, seed=7, H=64, W=64)
    unused0 = f.P[n:].clone()
    host = oc.HostDriver(rule, tr.lr, tr.wd, tr.momentum, f.P[:n].cpu().numpy())
    worst = 0.0
    for t in range(1, 15):
        before = f.P.clone()
        mask, point, direction = tr.forward(batch[0])
        tr.backward(*tr.loss_and_grads(mask, point, direction, *batch[1:]))
        g = f.G[:n].cpu().numpy()
        tr.allreduce_and_step()
        torch.cuda.synchronize()
        host.p[:] = before[:n].cpu().numpy()             # each step is judged on its own: from the trainer's own parameters
        host.step(g)
        after = f.P[:n].cpu().numpy()
        err = oc.rel_error(after, host.params(), before[:n].cpu().numpy())
        worst = max(worst, err)
        assert err <= oc.BAR, (t, err)
        assert torch.equal(f.P[n:], unused0), 'never-used parameters were stepped'
        if rule == 'radam4s' and t <= 4:
            assert torch.equal(f.P, before), 'RAdam_4step moved the parameters at step %d' % t
        elif np.isfinite(g).all():
            assert not torch.equal(f.P[:n], before[:n])
        if rule == 'ranger' and t in (6, 12):
            assert torch.equal(f.P[:n], f.S), 'P != slow after the lookahead sync of step %d' % t
        if rule == 'ranger' and t == 5:
            assert not torch.equal(f.P[:n], f.S)
    print(rule, 'worst step error', worst)
    assert np.array_equal(f.M[:n].cpu().numpy(), host.m)
    # the checkpoint entry has the layout of the reference's object and continues bit for bit in a fresh trainer
    z = golden('optim')
    sd = tr.state_dict()
    assert sorted(sd['param_groups'][0]) == list(z[rule + '/group_keys'])
    names = [k for k, _ in m.named_parameters()]
    assert sorted(sd['state']) == [i for i, k in enumerate(names) if f.offsets[k][0] < n]
    assert all(sorted(st) == list(z[rule + '/state_keys']) for st in sd['state'].values())
    m2 = _dam(seed=4)
    m2.load_state_dict(m.state_dict())
    tr2, _ = utils.get_optimizer(_args(rule), m2)
    tr2.load_state_dict(sd)
    tr2.refresh_parameters()
    assert tr2.flat.step_count == (1 if rule == 'sgd' else 14) and torch.equal(tr2.flat.P, f.P)
    for bn_a, bn_b in zip((x for x in m.modules() if isinstance(x, torch.nn.BatchNorm2d)),
                          (x for x in m2.modules() if isinstance(x, torch.nn.BatchNorm2d))):
        assert torch.equal(bn_a.running_mean, bn_b.running_mean)
    for t_ in (tr, tr2):
        t_.train_step(*batch)
    torch.cuda.synchronize()
    assert torch.equal(tr.flat.P, tr2.flat.P) and torch.equal(tr.flat.M, tr2.flat.M)
    with pytest.raises(ValueError, match='layout'):
        trainer.Trainer(_dam(seed=5)).load_state_dict(sd)


def test_entry_point_radam_steplr_rates_checkpoint_and_resume(tmp_path, monkeypatch, caplog):
    """lr, lr/2, lr/4 over three epochs; the scheduler steps before the checkpoint is written (train.py:404-428), so the file carries
    the NEXT epoch's rate lr/8, and a resumed fourth epoch trains at it"""
    import torch
    from cdnet_amd import train, train_util_dam
    seen = []
    real = train_util_dam.train

    def spy(loader, model, trainer, *a, **kw):
        seen.append((trainer.optimizer, trainer.lr, trainer.flat.step_count))
        return real(loader, model, trainer, *a, **kw)
    monkeypatch.setattr(train_util_dam, 'train', spy)
    caplog.set_level(logging.INFO, logger='cdnet_amd.train')
    d = str(tmp_path / 'radam')
    res = train.main(['--synthetic', '4', '--epochs', '3', '--optimizer', 'radam', '--scheduler', 'StepLR', '--step', '1', '--lr_decay', '0.5',
                      '--save-dir', d])
    assert np.isfinite(res).all()
    lr = 1e-3
    assert seen == [('radam', lr, 0), ('radam', lr * 0.5, 4), ('radam', lr * 0.25, 8)]
    msgs = [r.getMessage() for r in caplog.records if 'Updating learning rate' in r.getMessage()]
    assert len(msgs) == 3 and 'from {} to {}'.format(lr, lr * 0.5) in msgs[0] and 'from {} to {}'.format(lr * 0.25, lr * 0.125) in msgs[2]
    path = os.path.join(d, 'checkpoints', 'checkpoint.pth.tar')
    ck = torch.load(path, map_location='cpu', weights_only=False)
    group = ck['optimizer']['param_groups'][0]
    assert group['lr'] == lr * 0.125 and sorted(group) == ['betas', 'eps', 'lr', 'params', 'weight_decay']
    assert ck['epoch'] == 3 and all(st['step'] == 12 and sorted(st) == ['exp_avg', 'exp_avg_sq', 'step'] for st in ck['optimizer']['state'].values())
    res2 = train.main(['--synthetic', '4', '--epochs', '4', '--optimizer', 'radam', '--scheduler', 'StepLR', '--step', '1', '--lr_decay', '0.5',
                       '--save-dir', d, '--checkpoint-path', path])
    assert np.isfinite(res2).all() and seen[3:] == [('radam', lr * 0.125, 12)]
    ck2 = torch.load(path, map_location='cpu', weights_only=False)
    assert ck2['epoch'] == 4 and ck2['optimizer']['param_groups'][0]['lr'] == lr * 0.0625
    assert all(st['step'] == 16 for st in ck2['optimizer']['state'].values())
    # a run of another optimiser does not silently continue this state
    with pytest.raises(ValueError, match='layout'):
        train.main(['--synthetic', '1', '--epochs', '5', '--optimizer', 'adamw', '--save-dir', d, '--checkpoint-path', path])


def test_entry_point_ranger_cosine_and_plain_unet_sgd(tmp_path, caplog):
    """Ranger with CosineAnnealingWarmRestarts writes Ranger's checkpoint keys and logs the rate; the plain UNet's trainer is built
    through the same selection"""
    import torch
    from cdnet_amd import train
    caplog.set_level(logging.INFO, logger='cdnet_amd.train')
    d = str(tmp_path / 'ranger')
    res = train.main(['--synthetic', '3', '--epochs', '2', '--batch-size', '2', '--optimizer', 'ranger', '--scheduler',
                      'CosineAnnealingWarmRestarts', '--save-dir', d])
    assert len(res) == 11 and np.isfinite(res).all()
    assert sum('Updating learning rate' in r.getMessage() for r in caplog.records) == 2
    ck = torch.load(os.path.join(d, 'checkpoints', 'checkpoint.pth.tar'), map_location='cpu', weights_only=False)
    group = ck['optimizer']['param_groups'][0]
    assert sorted(group) == ['N_sma_threshhold', 'alpha', 'betas', 'eps', 'k', 'lr', 'params', 'step_counter', 'weight_decay']
    assert group['eps'] == 1e-5 and 0 < group['lr'] < 1e-3
    assert all(sorted(st) == ['exp_avg', 'exp_avg_sq', 'slow_buffer', 'step'] and st['step'] == 6 for st in ck['optimizer']['state'].values())
    du = str(tmp_path / 'unet')
    res_u = train.main(['--synthetic', '2', '--epochs', '1', '--batch-size', '2', '--model-name', 'UNet', '--optimizer', 'sgd', '--momentum', '0.8',
                        '--save-dir', du])
    assert len(res_u) == 3 and np.isfinite(res_u).all()
    cku = torch.load(os.path.join(du, 'checkpoints', 'checkpoint.pth.tar'), map_location='cpu', weights_only=False)
    gu = cku['optimizer']['param_groups'][0]
    assert gu['momentum'] == 0.8 and gu['nesterov'] is False and all(sorted(st) == ['momentum_buffer'] for st in cku['optimizer']['state'].values())


def test_default_adam_path_is_bit_identical_to_cdnet_adam_step():
    """--optimizer adam, scheduler 'None': three steps of the trainer == cdnet_adam_step called here on the same gradients with the
    arguments the trainer has always passed"""
    import torch
    from cdnet_amd import _lib, trainer, utils
    dev = torch.device('cuda:0')
    m = _dam()
    tr, sched = utils.get_optimizer(_args('adam'), m)
    assert sched is None and tr.optimizer == 'adam' and (tr.lr, tr.wd, tr.betas, tr.eps) == (1e-3, 1e-4, (0.9, 0.99), 1e-8)
    f = tr.flat
    n = f.n_used
    batch = trainer.synthetic_batch(2, dev, seed=7, H=64, W=64)
    p, mm, vv = f.P.clone(), f.M.clone(), f.V.clone()
    p_start = f.P.clone()
    for t in range(1, 4):
        assert torch.equal(f.P, p)
        mask, point, direction = tr.forward(batch[0])
        tr.backward(*tr.loss_and_grads(mask, point, direction, *batch[1:]))
        g = f.G.clone()
        tr.allreduce_and_step()
        assert utils.adjust_learning_rate(_args('adam'), tr, t) == 1e-3 and tr.lr == 1e-3
        _lib.call('cdnet_adam_step', _lib.ptr(p), _lib.ptr(g), _lib.ptr(mm), _lib.ptr(vv), n, 1e-3, 0.9, 0.99, 1e-8, 1e-4, t, 1.0,
                  _lib.stream_ptr())
        torch.cuda.synchronize()
    assert torch.equal(f.P, p) and torch.equal(f.M, mm) and torch.equal(f.V, vv) and not torch.equal(p, p_start)
    sd = tr.state_dict()
    assert sorted(sd['param_groups'][0]) == sorted(['lr', 'betas', 'eps', 'weight_decay', 'amsgrad', 'maximize', 'foreach', 'capturable',
                                                     'differentiable', 'fused', 'params'])
    assert all(float(st['step']) == 3.0 for st in sd['state'].values())


@pytest.mark.parametrize('rule', TRAINER_RULES)
def test_stepping_in_bucket_ranges_with_grad_scale(rule):
    """behind the all-reduce the optimiser follows the collectives bucket by bucket: the kernels get slices [a, b) of the flat buffers
    at arbitrary element offsets and grad_scale = 1 / world.  Ranges with odd boundaries + grad_scale 0.5 == one host step on g / 2."""
    import torch
    from cdnet_amd import trainer

    class Tiny(torch.nn.Module):
        UNUSED_PREFIXES = ('unused.',)

        def __init__(self):
            super().__init__()
            torch.manual_seed(3)
            self.conv = torch.nn.Conv2d(3, 8, 3)
            self.bn = torch.nn.BatchNorm2d(8)
            self.unused = torch.nn.Conv2d(1, 2, 1)
    tr = trainer.Trainer(Tiny().cuda(), optimizer=rule, lr=1e-2, weight_decay=0.1)
    f = tr.flat
    n = f.n_used
    assert n == 240 and f.P.numel() > n
    p0 = f.P.clone()
    host = oc.HostDriver(rule, tr.lr, tr.wd, tr.momentum, p0[:n].cpu().numpy())
    rs = np.random.RandomState(11)
    for t in range(1, 15):
        g = (0.1 * rs.randn(f.P.numel())).astype(np.float32)
        f.G.copy_(torch.from_numpy(g))
        f.step_count += 1
        step = tr._rule_stepper(0.5)
        for a, b in ((130, 240), (7, 130), (0, 7)):      # top-down, as the buckets are released
            step(a, b)
        torch.cuda.synchronize()
        host.step(g[:n] * np.float32(0.5))
        assert np.array_equal(f.P[:n].cpu().numpy(), host.params()), t
        assert torch.equal(f.P[n:], p0[n:])
    assert np.array_equal(f.M[:n].cpu().numpy(), host.m) and not torch.equal(f.P[:n], p0[:n])
