"""Regenerate tests/golden/optim.npz, optim_stress.npz and optim_state.npz: trajectories of the reference's own optimiser objects
(utils.py:907-939: torch.optim.SGD, hhl_utils/radam.py RAdam / RAdam_4step / AdamW, hhl_utils/ranger.py Ranger) on one flat
parameter vector.

CONTAINER-ONLY: imports the reference's classes from /root/reference (read-only, never copied).  The fixtures hold data only.

    python tests/golden/make_golden_optim.py

  optim.npz         p0 = 0.05 randn(4099) (weight-sized: at |p| ~ 1 an fp32 ulp is already 1 % of AdamW's warm-up step), 14 gradients
                    0.1 randn (gradient TINY_AT is 1e-6 randn), the key names of every object's state / param group, and the DEFAULT
                    setting's parameters (lr 1e-3, weight decay 1e-4) after steps 1, 4, 5, 6, 7, 12, 14 as '<optimiser>/p<step>'
  optim_stress.npz  the same snapshots at lr 1e-2, weight decay 0.1 (at 1e-4 the kind of decay is invisible)
  optim_state.npz   '<setting>/<optimiser>/final/<key>' the state tensors after the last step (both settings) and
                    'default/<optimiser>/at7/<key>' the state after step 7 (what a checkpoint written there would hold)
AdamW runs two segments: 'adamw' steps 1-6 from zero state (deep in the warm-up), and 'adamw4k' 14 steps that start from the end of
the first segment with the step counter set to 3995, i.e. steps 3996-4009 across the warm-up boundary (snapshots are numbered
1..14 within the segment; 'adamw4k/start' is its starting parameter vector = 'adamw/p6').
Three files instead of one keep every file below the repository's 1 MiB limit.
"""
import os
import sys

import numpy as np
import torch

REF = '/root/reference'
HERE = os.path.dirname(os.path.abspath(__file__))
N, STEPS, TINY_AT = 4099, 14, 9
SNAPSHOTS = (1, 4, 5, 6, 7, 12, 14)
SETTINGS = {'default': (1e-3, 1e-4), 'stress': (1e-2, 0.1)}
MOMENTUM = 0.95                                        # options.py:28


def make(name, params, lr, wd):
    """utils.py:910-935"""
    sys.path.insert(0, REF)
    from hhl_utils.radam import AdamW, RAdam, RAdam_4step
    from hhl_utils.ranger import Ranger
    if name == 'sgd':
        return torch.optim.SGD(params, lr=lr, momentum=MOMENTUM, weight_decay=wd)
    if name == 'radam':
        return RAdam(params, lr=lr, betas=(0.9, 0.99), weight_decay=wd)
    if name == 'radam4s':
        return RAdam_4step(params, lr=lr, betas=(0.9, 0.99), weight_decay=wd, update_all=False, additional_four=False)
    if name.startswith('adamw'):
        return AdamW(params, lr=lr, betas=(0.9, 0.99), weight_decay=wd, warmup=4000)
    return Ranger(params, lr, betas=(0.9, 0.99), weight_decay=wd)


def state_arrays(opt, p):
    out = {}
    for k, v in opt.state[p].items():
        out[k] = v.detach().numpy().copy() if torch.is_tensor(v) else np.array(int(v), np.int64)
    return out


def run(name, p0, grads, lr, wd, steps, start=None):
    """snapshots {step: p}, state after step 7 (None when the run is shorter), final state, the object"""
    p = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = make(name, [p], lr, wd)
    if start is not None:
        opt.state[p].update(step=start['step'], exp_avg=torch.from_numpy(start['exp_avg'].copy()),
                            exp_avg_sq=torch.from_numpy(start['exp_avg_sq'].copy()))
    snaps, at7 = {}, None
    for t in range(1, steps + 1):
        p.grad = torch.from_numpy(grads[t - 1].copy())
        opt.step()
        if t in SNAPSHOTS:
            snaps[t] = p.detach().numpy().copy()
        if t == 7:
            at7 = state_arrays(opt, p)
    return snaps, at7, state_arrays(opt, p), opt


def main():
    rs = np.random.RandomState(2025)
    p0 = (0.05 * rs.randn(N)).astype(np.float32)
    grads = (0.1 * rs.randn(STEPS, N)).astype(np.float32)
    grads[TINY_AT] = (1e-6 * rs.randn(N)).astype(np.float32)
    files = {'default': {'p0': p0, 'grads': grads, 'snapshots': np.array(SNAPSHOTS), 'momentum': np.array(MOMENTUM),
                         'torch_version': np.array(torch.__version__)}, 'stress': {}}
    states = {}
    for setting, (lr, wd) in SETTINGS.items():
        out = files[setting]
        out['lr_wd'] = np.array([lr, wd], np.float64)
        for name in ('sgd', 'radam', 'radam4s', 'adamw', 'ranger'):
            steps = 6 if name == 'adamw' else STEPS
            snaps, at7, final, opt = run(name, p0, grads, lr, wd, steps)
            runs = [(name, snaps, at7, final)]
            if name == 'adamw':
                start = dict(final, step=3995)
                out['adamw4k/start'] = snaps[6]
                runs.append(('adamw4k',) + run('adamw4k', snaps[6], grads, lr, wd, STEPS, start=start)[:3])
            for key, sn, a7, fin in runs:
                for t, v in sn.items():
                    out['%s/p%d' % (key, t)] = v
                for k, v in fin.items():
                    states['%s/%s/final/%s' % (setting, key, k)] = v
                if setting == 'default' and a7 is not None:
                    for k, v in a7.items():
                        states['default/%s/at7/%s' % (key, k)] = v
            if setting == 'default':
                sd = opt.state_dict()
                out[name + '/group_keys'] = np.array(sorted(sd['param_groups'][0]))
                out[name + '/state_keys'] = np.array(sorted(sd['state'][0]))
    np.savez_compressed(os.path.join(HERE, 'optim.npz'), **files['default'])
    np.savez_compressed(os.path.join(HERE, 'optim_stress.npz'), **files['stress'])
    np.savez_compressed(os.path.join(HERE, 'optim_state.npz'), **states)


if __name__ == '__main__':
    main()
