"""Host side of the reference's optimisers and learning-rate schedulers (utils.py:907-977).

  FlatState                           the flat fp32 buffers of a trainer: parameters, gradients, the optimiser's state
  stepper(tr, grad_scale)             step(a, b) of the trainer's rule over a range of the flat buffers: cdnet_adam_step (csrc/optim.hip),
                                      cdnet_sgd_step / cdnet_moment_step (csrc/optim.hip)
  state_dict / load_state_dict        the optimiser entry of a checkpoint in the layout of the reference's object for the rule
  moment_scalars(rule, t, lr, wd)     the host scalars of step t of 'radam' / 'radam4s' / 'adamw' / 'ranger', computed in
                                      Python float like the reference's math.sqrt / ** (hhl_utils/radam.py, hhl_utils/ranger.py);
                                      cdnet_moment_step (csrc/optim.hip) takes them as float
  adam_step_host,
  moment_step_host / sgd_step_host    the kernels restated over flat fp32 numpy vectors, operation for operation: what
                                      the tests compare the kernels with, and how a trainer whose buffers live on the CPU steps
  LRSchedule                          the four torch schedulers of utils.py:941-957 over a one-parameter proxy optimiser
"""
import math

import numpy as np
import torch

from . import _lib

OPTIMIZERS = ('sgd', 'adam', 'radam', 'radam4s', 'adamw', 'ranger')            # utils.py:910-935, matched case-insensitively
MOMENT_RULES = ('radam', 'radam4s', 'adamw', 'ranger')
SCHEDULERS = ('StepLR', 'ExponentialLR', 'ReduceLROnPlateau', 'CosineAnnealingWarmRestarts')      # utils.py:941-957
BETAS = (0.9, 0.99)                                                             # utils.py:917-935: every rule
ADAMW_WARMUP = 4000                                                             # utils.py:930
RANGER_K, RANGER_ALPHA, RANGER_THRESHOLD, RANGER_EPS = 6, 0.5, 5, 1e-5          # ranger.py:28 (the class defaults)


def moment_scalars(rule, t, lr, wd, betas=BETAS, eps=None):
    """host scalars of the 1-based step `t`: dict(move, rect, decay, step_size, v_div, eps, sync, alpha)"""
    assert rule in MOMENT_RULES and t >= 1, (rule, t)
    b1, b2 = betas
    b2t = b2 ** t
    bc1 = 1 - b1 ** t
    n_max = 2 / (1 - b2) - 1
    n_sma = n_max - 2 * t * b2t / (1 - b2t)
    s = dict(move=1, rect=1, decay=wd * lr, step_size=0.0, v_div=1.0, eps=1e-8 if eps is None else eps, sync=0, alpha=RANGER_ALPHA)
    if rule == 'adamw':                                     # radam.py:235-246
        lr_t = 1e-6 + t * (lr - 1e-6) / ADAMW_WARMUP if ADAMW_WARMUP > t else lr
        s['step_size'] = lr_t * math.sqrt(1 - b2t) / bc1
        s['decay'] = wd * lr_t
        return s
    if rule == 'radam4s':                                   # radam.py:133-162 with update_all = additional_four = False
        if t <= 4:
            s['move'] = 0
            return s
        s['step_size'] = lr * math.sqrt((n_sma - 4) / (n_max - 4) * (n_sma - 2) / n_sma * n_max / (n_max - 2)) / bc1
        s['v_div'] = math.sqrt(1 - b2t)
        return s
    # radam.py:55-77 / ranger.py:137-154 (threshold strict, eps 1e-5, lookahead every k steps)
    ranger = rule == 'ranger'
    s['rect'] = int(n_sma > RANGER_THRESHOLD if ranger else n_sma >= 5)
    if s['rect']:
        s['step_size'] = lr * math.sqrt((1 - b2t) * (n_sma - 4) / (n_max - 4) * (n_sma - 2) / n_sma * n_max / (n_max - 2)) / bc1
    else:
        s['step_size'] = lr / bc1
    if ranger:
        if eps is None:
            s['eps'] = RANGER_EPS
        s['sync'] = int(t % RANGER_K == 0)
    return s


def _np32(a):
    """the fp32 numpy view of a flat CPU vector (torch tensor or numpy array), updated in place"""
    a = a.numpy() if hasattr(a, 'numpy') else a
    assert a.dtype == np.float32 and a.ndim == 1
    return a


def moment_step_host(p, g, m, v, slow, s, betas=BETAS, grad_scale=1.0):
    """moment_kernel (csrc/optim.hip) in numpy fp32, in place: the same operations in the same order, nothing contracted"""
    f = np.float32
    p, g, m, v = _np32(p), _np32(g), _np32(m), _np32(v)
    b1, b2, omb1, omb2 = f(betas[0]), f(betas[1]), f(1.0 - betas[0]), f(1.0 - betas[1])
    g = g * f(grad_scale)
    v[:] = v * b2 + omb2 * (g * g)
    m[:] = m * b1 + omb1 * g
    if s['move']:
        p[:] = p + f(-s['decay']) * p
        if s['rect']:
            p[:] = p + f(-s['step_size']) * (m / (np.sqrt(v) / f(s['v_div']) + f(s['eps'])))
        else:
            p[:] = p + f(-s['step_size']) * m
    if s['sync']:
        slow = _np32(slow)
        slow[:] = slow + f(s['alpha']) * (p - slow)
        p[:] = slow


def sgd_step_host(p, g, buf, t, lr, momentum, wd, grad_scale=1.0):
    """sgd_kernel (csrc/optim.hip) in numpy fp32, in place: torch.optim.SGD with dampening 0 and no Nesterov"""
    f = np.float32
    p, g, buf = _np32(p), _np32(g), _np32(buf)
    g = g * f(grad_scale)
    g = g + f(wd) * p
    buf[:] = g if t == 1 else buf * f(momentum) + g
    p[:] = p + f(-lr) * buf


def adam_step_host(p, g, m, v, t, lr, betas, eps, wd, grad_scale=1.0):
    """adam_kernel (csrc/optim.hip) in numpy fp32, in place (the kernel's fused multiply-add of the weight decay through float64)"""
    f = np.float32
    p, g, m, v = _np32(p), _np32(g), _np32(m), _np32(v)
    b1, b2 = f(betas[0]), f(betas[1])
    bc1, bc2_sqrt = f(1.0 - float(betas[0]) ** t), f(math.sqrt(1.0 - float(betas[1]) ** t))
    g = (np.float64(f(wd)) * p + np.float64(1.0) * (g * f(grad_scale))).astype(f)
    m[:] = m + (g - m) * (f(1.0) - b1)
    v[:] = v * b2 + (f(1.0) - b2) * g * g
    p[:] = p - (f(lr) / bc1) * (m / (np.sqrt(v) / bc2_sqrt + f(eps)))


# the order of cdnet_dam_head_backward's weight block (csrc/head_bwd.hip), which FlatState puts first
HEAD_PARAMS = ['point_conv.weight', 'direction_conv.weight', 'mask_conv.weight', 'point_conv.bias',
               'direction_conv.bias', 'mask_conv.bias', 'directionAtt.Conv1x1.weight', 'maskAtt.Conv1x1.weight']


class FlatState:
    """fp32 flat buffers: parameters, gradients, Adam moments.  Head parameters first (in the kernel's block layout),
    then every other parameter that takes part in forward, then the frozen ones (requires_grad False), then the reference's
    never-used parameters (no gradient, never stepped - torch.optim.Adam skips parameters whose .grad is None): `n_used` ends
    in front of the frozen block.
    The state buffers follow the optimiser: M is the first moment (SGD: the momentum buffer), V the second moment (none for SGD),
    S Ranger's slow weights over the stepped parameters (none otherwise)."""

    def __init__(self, model, optimizer='adam'):
        # a model that computes on zero-padded parameter copies (HRNet) hands those over; its own parameters stay views
        named = model.trainer_named_parameters() if hasattr(model, 'trainer_named_parameters') else dict(model.named_parameters())
        unused = [n for n in named if n.startswith(tuple(getattr(model, 'UNUSED_PREFIXES', ())))]
        # frozen parameters (requires_grad False, Unet.freeze_encoder): behind the stepped range like the never-used ones - no gradient, no
        # step, no weight decay, no moments, no slow weights, in no all-reduce bucket.  Read here, once
        real = dict(model.named_parameters())          # (the flag lives on the module's own parameters, not on padded compute copies)
        frozen = [n for n in named if n in real and not real[n].requires_grad and n not in unused]
        head = [n for n in HEAD_PARAMS if n in named and n not in unused and n not in frozen]
        rest = [n for n in named if n not in head and n not in unused and n not in frozen]
        self.frozen = frozen
        self.order = head + rest + frozen + unused
        sizes = [named[n].numel() for n in self.order]
        total = sum(sizes)
        dev = next(model.parameters()).device
        self.P = torch.empty((total,), dtype=torch.float32, device=dev)
        self.G = torch.zeros((total,), dtype=torch.float32, device=dev)
        self.M = torch.zeros((total,), dtype=torch.float32, device=dev)
        self.V = None if optimizer == 'sgd' else torch.zeros((total,), dtype=torch.float32, device=dev)
        self.S = None
        self.offsets = {}
        off = 0
        with torch.no_grad():
            for n, sz in zip(self.order, sizes):
                p = named[n]
                self.P[off:off + sz].copy_(p.detach().reshape(-1))         # one-time host-side setup
                p.data = self.P[off:off + sz].view(p.shape)
                p.grad = self.G[off:off + sz].view(p.shape)
                self.offsets[n] = (off, sz)
                off += sz
        if hasattr(model, 'rebind_views'):
            model.rebind_views()
        self.n_used = sum(named[n].numel() for n in head + rest)
        self.n_head = sum(named[n].numel() for n in head)
        if optimizer == 'ranger':
            self.S = self.P[:self.n_used].clone()            # (taken again when the first step starts, ranger.py:113-114)
        self.step_count = 0


def stepper(tr, grad_scale):
    """step(a, b): step `tr.flat.step_count` of the trainer's rule over the range [a, b) of its flat buffers, the gradients times
    grad_scale.  `tr` gives flat, optimizer, lr, wd, betas, eps, momentum and dev.  The step's host scalars are computed once
    (moment_scalars).  Buffers on the CPU take the host restatement of cdnet_sgd_step / cdnet_moment_step."""
    f, rule, t = tr.flat, tr.optimizer, tr.flat.step_count
    on_host = tr.dev.type == 'cpu'
    if rule == 'adam':
        def step(a, b):
            if on_host:
                return adam_step_host(f.P[a:b], f.G[a:b], f.M[a:b], f.V[a:b], t, tr.lr, tr.betas, tr.eps, tr.wd, grad_scale)
            _lib.call('cdnet_adam_step', _lib.ptr(f.P[a:b]), _lib.ptr(f.G[a:b]), _lib.ptr(f.M[a:b]), _lib.ptr(f.V[a:b]), b - a, tr.lr,
                      tr.betas[0], tr.betas[1], tr.eps, tr.wd, t, grad_scale, _lib.stream_ptr())
        return step
    if rule == 'sgd':
        def step(a, b):
            if on_host:
                sgd_step_host(f.P[a:b], f.G[a:b], f.M[a:b], t, tr.lr, tr.momentum, tr.wd, grad_scale)
            else:
                _lib.call('cdnet_sgd_step', _lib.ptr(f.P[a:b]), _lib.ptr(f.G[a:b]), _lib.ptr(f.M[a:b]), b - a, tr.lr, tr.momentum,
                          tr.wd, t, grad_scale, _lib.stream_ptr())
        return step
    s = moment_scalars(rule, t, tr.lr, tr.wd, tr.betas, tr.eps)
    if rule == 'ranger' and t == 1:
        f.S.copy_(f.P[:f.n_used])                    # the slow weights start as the parameters of the first step

    def step(a, b):
        slow = f.S[a:b] if s['sync'] else None
        if on_host:
            moment_step_host(f.P[a:b], f.G[a:b], f.M[a:b], f.V[a:b], slow, s, tr.betas, grad_scale)
        else:
            _lib.call('cdnet_moment_step', _lib.ptr(f.P[a:b]), _lib.ptr(f.G[a:b]), _lib.ptr(f.M[a:b]), _lib.ptr(f.V[a:b]), _lib.ptr(slow),
                      b - a, tr.betas[0], tr.betas[1], grad_scale, s['move'], s['rect'], s['decay'], s['step_size'], s['v_div'], s['eps'],
                      s['sync'], s['alpha'], _lib.stream_ptr())
    return step


# ----------------------------------------------------------------------------------------------------------
# Optimiser state in the state_dict format of the reference's optimiser object (what the reference stores under
# checkpoint['optimizer'], train.py:421-427, and reads back at :302): parameter indices follow model.parameters(); parameters that
# never received a gradient have no entry (the optimisers create state lazily).  `tr` is the trainer that owns the flat buffers.
def _real_pieces(tr, buf, name, p):
    """[(index into the real parameter, view of `buf`)] covering parameter `name` (the model's own shape), whether the flat
    storage holds it as is, zero-padded (leading corner) or scattered over channel segments (HRNet)"""
    off, sz = tr.flat.offsets[name]
    slots = {id(real): (pp, segs) for real, pp, segs in getattr(tr.model, '_slots', [])}
    if id(p) not in slots:
        return [(Ellipsis, buf[off:off + sz].view(p.shape))]
    pp, segs = slots[id(p)]
    full = buf[off:off + sz].view(pp.shape)
    if segs is None:
        return [(Ellipsis, full[tuple(slice(0, n) for n in p.shape)])]
    return [((slice(None), slice(r0, r0 + n)), full[:, p0:p0 + n]) for r0, n, p0 in segs]


def _gather(tr, buf, n, p):
    """CPU copy, in the model's own shape, of parameter `n`'s part of the flat state buffer `buf`"""
    t = torch.empty(p.shape, dtype=torch.float32)
    for idx, piece in _real_pieces(tr, buf, n, p):
        t[idx] = piece.cpu()
    return t


def _scatter(tr, buf, n, p, value):
    for idx, piece in _real_pieces(tr, buf, n, p):
        piece.copy_(value[idx])


def _state_buffers(tr):
    """state buffers of one parameter under the reference classes' own key names (torch.optim.SGD, hhl_utils/radam.py, ranger.py)"""
    f = tr.flat
    if tr.optimizer == 'sgd':
        return [('momentum_buffer', f.M)]
    return [('exp_avg', f.M), ('exp_avg_sq', f.V)] + ([('slow_buffer', f.S)] if tr.optimizer == 'ranger' else [])


def state_dict(tr):
    """the optimiser entry of a checkpoint in the layout of the reference's object for this optimiser: torch.optim.Adam / SGD,
    RAdam, RAdam_4step, AdamW (hhl_utils/radam.py) or Ranger (hhl_utils/ranger.py).  'step' is a tensor for Adam (torch's own
    format) and an int for the reference's classes; torch's SGD keeps no step (see load_state_dict)."""
    f = tr.flat
    params = list(tr.model.named_parameters())
    state = {}
    rule = tr.optimizer
    if f.step_count > 0:
        for i, (n, p) in enumerate(params):
            if f.offsets[n][0] >= f.n_used:
                continue                                        # frozen and never-used parameters: no gradient, no state (listed in the group)
            st = {} if rule == 'sgd' else {'step': torch.tensor(float(f.step_count)) if rule == 'adam' else int(f.step_count)}
            for key, buf in _state_buffers(tr):
                st[key] = _gather(tr, buf, n, p)
            state[i] = st
    ids = list(range(len(params)))
    if rule == 'adam':
        group = dict(lr=tr.lr, betas=tuple(tr.betas), eps=tr.eps, weight_decay=tr.wd, amsgrad=False, maximize=False, foreach=None,
                     capturable=False, differentiable=False, fused=None, params=ids)
    elif rule == 'sgd':
        # torch's own group, whatever keys the installed torch writes
        group = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=tr.lr, momentum=tr.momentum,
                                weight_decay=tr.wd).state_dict()['param_groups'][0]
        group['params'] = ids
    else:
        group = dict(lr=tr.lr, betas=tuple(tr.betas), eps=tr.eps, weight_decay=tr.wd)
        if rule == 'adamw':
            group.update(use_variance=True, warmup=ADAMW_WARMUP)
        if rule == 'ranger':
            group.update(alpha=RANGER_ALPHA, k=RANGER_K, step_counter=0, N_sma_threshhold=RANGER_THRESHOLD)
        group['params'] = ids
    return {'state': state, 'param_groups': [group]}


def _layout_of(sd):
    """which optimiser family wrote `sd`: read off the keys only that family's object has"""
    group = sd['param_groups'][0]
    keys = set(group)
    for st in sd['state'].values():
        keys |= set(st)
        break
    if 'momentum_buffer' in keys or 'nesterov' in keys:
        return 'sgd'
    if 'slow_buffer' in keys or 'N_sma_threshhold' in keys:
        return 'ranger'
    if 'warmup' in keys:
        return 'adamw'
    if 'amsgrad' in keys:
        return 'adam'
    return 'radam' if 'betas' in keys else 'unknown'


def load_state_dict(tr, sd):
    """Takes the state of the reference's object for THIS optimiser (RAdam and RAdam_4step share one layout); a state written by
    another optimiser raises instead of silently starting from zero moments.  The loaded group's lr, weight decay, betas, eps and
    momentum become the trainer's.  torch.optim.SGD stores no step count and the rule only asks whether a momentum buffer exists yet
    (buf = g on the very first step): a loaded SGD state with momentum buffers continues at step_count 1, one without them at 0."""
    f = tr.flat
    params = list(tr.model.named_parameters())
    group = sd['param_groups'][0]
    assert len(sd['param_groups']) == 1 and len(group['params']) == len(params), 'optimizer state of a different model'
    rule = tr.optimizer
    mine, theirs = ('radam' if rule == 'radam4s' else rule), _layout_of(sd)
    if theirs != mine:
        raise ValueError("optimizer state with the layout of '{}' cannot continue a '{}' run (param group keys: {})".format(
            theirs, rule, ', '.join(sorted(k for k in group if k != 'params'))))
    if rule == 'sgd':
        tr.lr, tr.wd, tr.momentum = group['lr'], group['weight_decay'], group['momentum']
    else:
        tr.lr, tr.betas, tr.eps, tr.wd = group['lr'], tuple(group['betas']), group['eps'], group['weight_decay']
    bufs = _state_buffers(tr)
    for _, buf in bufs:
        if buf is not f.S:
            buf.zero_()
    if f.S is not None:
        f.S.copy_(f.P[:f.n_used])
    steps = set()
    for i, st in sd['state'].items():
        n, p = params[int(i)]
        assert f.offsets[n][0] < f.n_used, 'state for a parameter that is never stepped: ' + n
        for key, buf in bufs:
            if key not in st or st[key] is None:
                raise ValueError("optimizer state of parameter {} lacks '{}': not a state of '{}'".format(n, key, rule))
            _scatter(tr, buf, n, p, st[key])
        steps.add(1 if rule == 'sgd' else int(st['step']))
    assert len(steps) <= 1, 'per-parameter step counts differ: not a state of one optimiser over the whole model'
    f.step_count = steps.pop() if steps else 0


class LRSchedule:
    """One of the four torch schedulers utils.get_optimizer builds (utils.py:941-957), torch's own object over a one-parameter proxy
    optimiser.  `step` is the reference's once-per-epoch call (train.py:406-411): it returns the rate that goes into `trainer.lr`.
    The scheduler state is not saved (the reference does not save it either): a resumed run starts a fresh schedule that acts on
    the checkpoint's rate, as the reference's fresh scheduler acts on the loaded param group."""

    def __init__(self, name, lr, step=5, lr_decay=0.995):
        assert name in SCHEDULERS, name
        self.name = name
        self._proxy = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr)
        S = torch.optim.lr_scheduler
        if name == 'StepLR':
            self.torch_scheduler = S.StepLR(self._proxy, step_size=step, gamma=lr_decay)
        elif name == 'ExponentialLR':
            self.torch_scheduler = S.ExponentialLR(self._proxy, gamma=lr_decay)
        elif name == 'ReduceLROnPlateau':
            self.torch_scheduler = S.ReduceLROnPlateau(self._proxy, 'min', factor=lr_decay, patience=step)
        else:
            self.torch_scheduler = S.CosineAnnealingWarmRestarts(self._proxy, T_0=step, T_mult=2, eta_min=0)

    def step(self, current_lr, val_loss=None):
        """current_lr: the rate the trainer holds now (the scheduler's param group in the reference); val_loss: the epoch's validation
        loss, read by ReduceLROnPlateau only"""
        self._proxy.param_groups[0]['lr'] = current_lr
        self._proxy.step()                                 # (nothing to update: keeps torch's call-order warning quiet)
        if self.name == 'ReduceLROnPlateau':
            self.torch_scheduler.step(val_loss)
        else:
            self.torch_scheduler.step()
        return self._proxy.param_groups[0]['lr']
