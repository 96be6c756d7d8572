"""Host side of the reference's optimisers and learning-rate schedulers (utils.py:907-977).

  moment_scalars(rule, t, lr, wd)     the host scalars of step t of 'radam' / 'radam4s' / 'adamw' / 'ranger', computed in
                                      Python float like the reference's math.sqrt / ** (hhl_utils/radam.py, hhl_utils/ranger.py);
                                      cdnet_moment_step (csrc/optim.hip) takes them as float
  moment_step_host / sgd_step_host    the two kernels restated over flat fp32 numpy vectors, operation for operation: what
                                      the tests compare the kernels with, and how a trainer whose buffers live on the CPU steps
  LRSchedule                          the four torch schedulers of utils.py:941-957 over a one-parameter proxy optimiser
"""
import math

import numpy as np

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


class LRSchedule:
    """One of the four torch schedulers utils.get_optimizer builds (utils.py:941-957), torch's own object over a one-parameter proxy
    optimiser.  `step` is the reference's once-per-epoch call (train.py:406-411): it returns the rate that goes into `trainer.lr`.
    The scheduler state is not saved (the reference does not save it either): a resumed run starts a fresh schedule that acts on
    the checkpoint's rate, as the reference's fresh scheduler acts on the loaded param group."""

    def __init__(self, name, lr, step=5, lr_decay=0.995):
        import torch
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
