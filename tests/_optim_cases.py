"""Shared by test_optim.py (CPU) and test_gpu_optim.py: the cases of tests/golden/optim*.npz (trajectories of the reference's own
optimiser objects, tests/golden/make_golden_optim.py) and two drivers that walk them - the host restatement and the C ABI."""
import numpy as np

RULES = ('sgd', 'radam', 'radam4s', 'adamw', 'adamw4k', 'ranger')         # 'adamw4k': AdamW from step 3995, across the warm-up's end
SETTINGS = ('default', 'stress')
# displacement-relative error || p_t - ref_t || / || ref_t - p_start ||: measured on the CPU against the reference, a reordered fp32
# restatement of each rule sits at 1.4e-7 .. 2.4e-6 and the smallest wrong rule (L2 instead of decoupled decay at the default
# setting) at 6.9e-5.  The bar is about ten times the floor and below every wrong rule.
BAR = 2e-5


def load_case(golden, setting, key):
    """dict(rule, lr, wd, momentum, p_start, grads, t0, snaps {t: parameters after t steps of the segment})"""
    z, zs = golden('optim'), golden('optim' if setting == 'default' else 'optim_stress')
    lr, wd = [float(v) for v in zs['lr_wd']]
    snaps = {int(t): zs['%s/p%d' % (key, t)] for t in z['snapshots'] if '%s/p%d' % (key, t) in zs.files}
    c = dict(rule='adamw' if key == 'adamw4k' else key, lr=lr, wd=wd, momentum=float(z['momentum']), grads=z['grads'], snaps=snaps,
             p_start=z['p0'], t0=0, state=None)
    if key == 'adamw4k':
        st = golden('optim_state')
        c.update(p_start=zs['adamw4k/start'], t0=3995, state={k: st['%s/adamw/final/%s' % (setting, k)] for k in ('exp_avg', 'exp_avg_sq')})
    assert len(snaps) == (4 if key == 'adamw' else 7)
    return c


def rel_error(p, ref, p_start):
    """the displacement-relative error; a snapshot the reference did not move (radam4s, steps 1-4) must be bit-identical instead"""
    p, ref, p_start = (np.asarray(a, np.float64) for a in (p, ref, p_start))
    den = np.linalg.norm(ref - p_start)
    if den == 0:
        assert np.array_equal(p, ref), 'parameters moved on a step the reference leaves them alone'
        return 0.0
    return float(np.linalg.norm(p - ref) / den)


class HostDriver:
    """one flat vector stepped by cdnet_amd.optim's restatement of the kernels"""

    def __init__(self, rule, lr, wd, momentum, p, t0=0, state=None):
        self.rule, self.lr, self.wd, self.momentum, self.t = rule, lr, wd, momentum, t0
        self.p = self.to_buf(p)
        st = state or {}
        self.m = self.to_buf(st.get('momentum_buffer' if rule == 'sgd' else 'exp_avg', np.zeros_like(p)))
        self.v = None if rule == 'sgd' else self.to_buf(st.get('exp_avg_sq', np.zeros_like(p)))
        self.slow = self.to_buf(st.get('slow_buffer', p)) if rule == 'ranger' else None

    def to_buf(self, a):
        return np.array(a, dtype=np.float32)

    def from_buf(self, b):
        return b

    def params(self):
        return self.from_buf(self.p)

    def sgd(self, g):
        from cdnet_amd import optim
        optim.sgd_step_host(self.p, g, self.m, self.t, self.lr, self.momentum, self.wd)

    def moment(self, g, s):
        from cdnet_amd import optim
        optim.moment_step_host(self.p, g, self.m, self.v, self.slow, s)

    def step(self, g):
        from cdnet_amd import optim
        self.t += 1
        g = self.to_buf(g)
        if self.rule == 'sgd':
            return self.sgd(g)
        self.moment(g, optim.moment_scalars(self.rule, self.t, self.lr, self.wd))


class DeviceDriver(HostDriver):
    """the same through cdnet_sgd_step / cdnet_moment_step.  Every buffer starts `shift` elements behind a 16-byte boundary, so that
    with n = 4099 the kernels' scalar head, vector body and scalar tail all run."""

    def __init__(self, *a, shift=1, **kw):
        self.shift = shift
        super().__init__(*a, **kw)

    def to_buf(self, a):
        import torch
        a = np.asarray(a, np.float32)
        big = torch.zeros(a.size + 8, dtype=torch.float32, device='cuda')
        b = big[self.shift:self.shift + a.size]
        b.copy_(torch.from_numpy(a.copy()))
        assert b.data_ptr() % 16 == 4 * self.shift % 16
        return b

    def from_buf(self, b):
        return b.cpu().numpy()

    def sgd(self, g):
        from cdnet_amd import _lib
        _lib.call('cdnet_sgd_step', _lib.ptr(self.p), _lib.ptr(g), _lib.ptr(self.m), self.p.numel(), self.lr, self.momentum, self.wd,
                  self.t, 1.0, _lib.stream_ptr())

    def moment(self, g, s):
        from cdnet_amd import _lib
        _lib.call('cdnet_moment_step', _lib.ptr(self.p), _lib.ptr(g), _lib.ptr(self.m), _lib.ptr(self.v), _lib.ptr(self.slow),
                  self.p.numel(), 0.9, 0.99, 1.0, s['move'], s['rect'], s['decay'], s['step_size'], s['v_div'], s['eps'], s['sync'],
                  s['alpha'], _lib.stream_ptr())


def walk(driver_cls, case, **kw):
    """run the case's whole segment; returns {t: relative error of the parameters after t steps}"""
    d = driver_cls(case['rule'], case['lr'], case['wd'], case['momentum'], case['p_start'], t0=case['t0'], state=case['state'], **kw)
    errs = {}
    for k in range(max(case['snaps'])):
        d.step(case['grads'][k])
        if k + 1 in case['snaps']:
            errs[k + 1] = rel_error(d.params(), case['snaps'][k + 1], case['p_start'])
    return errs, d
