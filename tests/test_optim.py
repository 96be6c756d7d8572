"""The reference's other optimisers and LR schedulers (utils.py:907-977), CPU side: the host restatement of the update kernels
against trajectories of the reference's own optimiser objects (tests/golden/optim*.npz), the library's argument validation, the
schedulers against torch's own, and the selection in utils.get_optimizer on a CPU-constructible model."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _optim_cases as oc  # noqa: E402


@pytest.mark.parametrize('setting', oc.SETTINGS)
@pytest.mark.parametrize('key', oc.RULES)
def test_host_restatement_matches_reference_trajectory(golden, setting, key):
    case = oc.load_case(golden, setting, key)
    errs, _ = oc.walk(oc.HostDriver, case)
    print(setting, key, {t: '%.2e' % e for t, e in errs.items()})
    assert max(errs.values()) <= oc.BAR, errs


def test_step_scalars_follow_the_rules_table():
    """the facts the fixtures rest on: N_sma crosses 5 between steps 5 and 6 at beta2 = 0.99 (4.96 / 5.94), RAdam_4step moves from
    step 5 on with a positive N - 4, AdamW's warm-up ends at step 4000, Ranger syncs at 6 and 12 with eps 1e-5"""
    from cdnet_amd import optim
    lr, wd = 1e-3, 1e-4
    for t in range(1, 15):
        r, r4, rg = (optim.moment_scalars(n, t, lr, wd) for n in ('radam', 'radam4s', 'ranger'))
        assert r['rect'] == rg['rect'] == int(t >= 6) and r['move'] == 1
        assert r4['move'] == int(t > 4) and (t <= 4 or (r4['rect'] == 1 and r4['step_size'] > 0 and r4['v_div'] == math.sqrt(1 - 0.99 ** t)))
        assert rg['sync'] == int(t in (6, 12)) and rg['eps'] == 1e-5 and r['eps'] == 1e-8 and rg['alpha'] == 0.5
        assert r['decay'] == wd * lr and r['v_div'] == 1.0
    a = optim.moment_scalars('adamw', 1, lr, wd)
    assert a['decay'] == wd * (1e-6 + (lr - 1e-6) / 4000) and a['step_size'] == (1e-6 + (lr - 1e-6) / 4000) * math.sqrt(1 - 0.99) / (1 - 0.9)
    assert optim.moment_scalars('adamw', 3999, lr, wd)['decay'] < wd * lr
    assert optim.moment_scalars('adamw', 4000, lr, wd)['decay'] == wd * lr


def test_argument_validation_without_gpu():
    """bad arguments return the error code with cdnet_last_error set before any HIP call"""
    from cdnet_amd import _lib
    lib = _lib.load()
    buf = np.zeros(16, np.float32)
    q = buf.ctypes.data                                   # (host memory: never dereferenced, every call below is refused)
    ok = dict(move=1, rect=1, decay=0.0, step=1e-3, vdiv=1.0, eps=1e-8, sync=0, alpha=0.5)

    def moment(p=q, g=q, m=q, v=q, slow=None, n=16, b1=0.9, b2=0.99, **kw):
        a = dict(ok, **kw)
        return lib.cdnet_moment_step(p, g, m, v, slow, n, b1, b2, 1.0, a['move'], a['rect'], a['decay'], a['step'], a['vdiv'], a['eps'],
                                     a['sync'], a['alpha'], None)
    for bad in (dict(p=None), dict(g=None), dict(m=None), dict(v=None)):
        assert moment(**bad) == 1 and b'null pointer' in lib.cdnet_last_error()
    assert moment(sync=1) == 1 and b'slow' in lib.cdnet_last_error()
    assert moment(move=2) == 1 and moment(rect=-1) == 1 and moment(sync=3, slow=q) == 1
    assert moment(b2=1.0) == 1 and b'betas' in lib.cdnet_last_error()
    assert moment(vdiv=0.0) == 1 and moment(alpha=1.5, sync=1, slow=q) == 1
    assert moment(p=q + 2) == 1 and b'aligned' in lib.cdnet_last_error()
    assert moment(n=(1 << 40) + 1) == 1 and b'out of range' in lib.cdnet_last_error()
    assert moment(n=0) == 0                               # nothing to do is not an error (cdnet_adam_step's convention)

    def sgd(p=q, g=q, b=q, n=16, step=1, momentum=0.95, wd=1e-4):
        return lib.cdnet_sgd_step(p, g, b, n, 1e-3, momentum, wd, step, 1.0, None)
    for bad in (dict(p=None), dict(g=None), dict(b=None)):
        assert sgd(**bad) == 1 and b'null pointer' in lib.cdnet_last_error()
    assert sgd(step=0) == 1 and b'1-based' in lib.cdnet_last_error()
    assert sgd(momentum=-0.1) == 1 and sgd(b=q + 1) == 1 and sgd(n=(1 << 40) + 1) == 1
    assert sgd(n=0) == 0


EPOCHS = 40
PLATEAU = [1.0, 0.9, 0.8] + [0.8] * 9 + [0.7] + [0.75] * 12 + [0.5, 0.6] + [0.6] * 13        # improvements, two plateaus, a late best


@pytest.mark.parametrize('name,step,decay', [('StepLR', 5, 0.995), ('StepLR', 1, 0.5), ('ExponentialLR', 5, 0.9), ('ReduceLROnPlateau', 3, 0.5),
                                             ('CosineAnnealingWarmRestarts', 5, 0.995)])
def test_scheduler_rates_match_torch(name, step, decay):
    """utils.get_optimizer's scheduler + the epoch loop's call (train.py:404-413) against torch's scheduler of the same arguments on a
    dummy optimiser, 40 epochs, exact"""
    from cdnet_amd import optim, utils
    lr = 1e-3
    dummy = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=lr)
    S = torch.optim.lr_scheduler
    ref = {'StepLR': lambda: S.StepLR(dummy, step_size=step, gamma=decay), 'ExponentialLR': lambda: S.ExponentialLR(dummy, gamma=decay),
           'ReduceLROnPlateau': lambda: S.ReduceLROnPlateau(dummy, 'min', factor=decay, patience=step),
           'CosineAnnealingWarmRestarts': lambda: S.CosineAnnealingWarmRestarts(dummy, T_0=step, T_mult=2, eta_min=0)}[name]()

    class Args:
        train = dict(optimizer='radam', scheduler=name, step=step, lr_decay=decay, lr=lr, weight_decay=1e-4)
        momentum = 0.95
    tr, sched = utils.get_optimizer(Args, _TinyNet())
    assert isinstance(sched, optim.LRSchedule) and tr.lr == lr
    assert len(PLATEAU) == EPOCHS
    got, want = [], []
    for epoch in range(EPOCHS):
        dummy.step()
        ref.step(PLATEAU[epoch]) if name == 'ReduceLROnPlateau' else ref.step()
        want.append(dummy.param_groups[0]['lr'])
        tr.lr = sched.step(tr.lr, PLATEAU[epoch])
        got.append(tr.lr)
    assert got == want
    assert len(set(want)) > 2                           # the rate really moves in every case


def test_unnamed_scheduler_falls_back_and_none_keeps_the_rate():
    """utils.adjust_learning_rate (utils.py:965-977): 'None' keeps the rate, any other unrecognised name decays by 0.9 every `step`"""
    from cdnet_amd import utils

    class Args:
        train = dict(optimizer='ranger', scheduler='cosine', step=5, lr_decay=0.995, lr=1e-3, weight_decay=1e-4)
        momentum = 0.95
    tr, sched = utils.get_optimizer(Args, _TinyNet())
    assert sched is None
    for epoch in range(EPOCHS):
        assert utils.adjust_learning_rate(Args, tr, epoch) == 1e-3 * (0.9 ** (epoch // 5)) == tr.lr
    assert tr.lr == 1e-3 * 0.9 ** 7
    Args.train['scheduler'] = 'None'
    tr.lr = 0.25
    assert utils.adjust_learning_rate(Args, tr, 17) == 0.25 and tr.lr == 0.25


class _TinyNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        torch.manual_seed(3)
        self.conv = torch.nn.Conv2d(3, 8, 3)
        self.bn = torch.nn.BatchNorm2d(8)
        self.unused = torch.nn.Conv2d(1, 2, 1)
    UNUSED_PREFIXES = ('unused.',)


def _args(name):
    class Args:
        train = dict(optimizer=name, scheduler='None', step=5, lr_decay=0.995, lr=1e-3, weight_decay=1e-4)
        momentum = 0.9
    return Args


@pytest.mark.parametrize('name', ['SGD', 'adam', 'RAdam', 'radam4s', 'AdamW', 'Ranger'])
def test_get_optimizer_builds_every_optimizer(golden, name):
    """every name of utils.py:910-935, case-insensitively, on a CPU model: buffers per rule, the reference objects' state_dict layout
    (key names recorded in the fixture), and - the trainer's buffers being on the CPU - 14 steps that equal the flat-vector driver"""
    from cdnet_amd import utils
    rule = name.lower()
    m = _TinyNet()
    tr, sched = utils.get_optimizer(_args(name), m)
    f = tr.flat
    assert sched is None and tr.optimizer == rule and (tr.lr, tr.wd, tr.momentum) == (1e-3, 1e-4, 0.9)
    assert (f.V is None) == (rule == 'sgd') and (f.S is None) == (rule != 'ranger')
    assert f.S is None or f.S.numel() == f.n_used < f.P.numel()
    if rule == 'adam':
        return                                           # (steps through cdnet_adam_step only: the GPU tests)
    z = golden('optim')
    p0 = f.P.clone()
    drv = oc.HostDriver(rule, tr.lr, tr.wd, tr.momentum, p0[:f.n_used].numpy())
    rs = np.random.RandomState(5)
    for t in range(1, 15):
        g = (0.1 * rs.randn(f.P.numel())).astype(np.float32)
        f.G.copy_(torch.from_numpy(g))
        tr.allreduce_and_step()
        drv.step(g[:f.n_used])
        assert np.array_equal(f.P[:f.n_used].numpy(), drv.params()), t
        assert torch.equal(f.P[f.n_used:], p0[f.n_used:])                   # the never-used parameters are never stepped
        if rule == 'radam4s' and t <= 4:
            assert torch.equal(f.P, p0)
        if rule == 'ranger' and t in (6, 12):
            assert torch.equal(f.P[:f.n_used], f.S)
    assert not torch.equal(f.P[:f.n_used], p0[:f.n_used])
    sd = tr.state_dict()
    assert sorted(sd['param_groups'][0]) == list(z[rule + '/group_keys'])
    n_params = len(list(m.parameters()))
    assert sd['param_groups'][0]['params'] == list(range(n_params)) and sorted(sd['state']) == [0, 1, 2, 3]       # conv w, b, bn w, b
    for st in sd['state'].values():
        assert sorted(st) == list(z[rule + '/state_keys'])
        assert rule == 'sgd' or (type(st['step']) is int and st['step'] == 14)
    # the state continues in a fresh trainer; one of another optimiser is refused
    tr2, _ = utils.get_optimizer(_args(name), _TinyNet())
    tr2.flat.P.copy_(f.P)
    tr2.load_state_dict(sd)
    g = (0.1 * rs.randn(f.P.numel())).astype(np.float32)
    for t_ in (tr, tr2):
        t_.flat.G.copy_(torch.from_numpy(g))
        t_.allreduce_and_step()
    assert torch.equal(tr.flat.P, tr2.flat.P) and torch.equal(tr.flat.M, tr2.flat.M)
    other = 'radam' if rule != 'radam' else 'adamw'
    tr3, _ = utils.get_optimizer(_args(other), _TinyNet())
    m_before = tr3.flat.M.clone()
    if rule == 'radam4s':
        tr3.load_state_dict(sd)                          # RAdam and RAdam_4step share one layout
    else:
        with pytest.raises(ValueError, match='layout'):
            tr3.load_state_dict(sd)
        assert torch.equal(tr3.flat.M, m_before)
    adam, _ = utils.get_optimizer(_args('adam'), _TinyNet())
    with pytest.raises(ValueError, match='layout'):
        adam.load_state_dict(sd)
    with pytest.raises(ValueError, match='layout'):
        tr.load_state_dict(adam.state_dict())


def test_unknown_optimizer_is_a_value_error():
    from cdnet_amd import trainer, utils
    with pytest.raises(ValueError, match='lamb'):
        utils.get_optimizer(_args('lamb'), _TinyNet())
    with pytest.raises(ValueError, match='lamb'):
        trainer.Trainer(_TinyNet(), optimizer='lamb')
