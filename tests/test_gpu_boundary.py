"""The boundary / focal term (--boundary-loss 1|2|3) on the GPU: cdnet_boundary_loss against the reference's BoundaryLoss / FocalLoss2d /
RobustFocalLoss2d evaluated in float64 (tests/golden/boundary.npz, written by tests/golden/make_golden_boundary.py from the reference itself),
and the term inside the trainers, validate() and the training entry.

The bar of every float comparison is FACTOR x max(yardstick, 2^-23): the yardstick is the reference's OWN float32 error against float64 on the
same inputs (`eloss32`, `egrad32` of the fixture), FACTOR = 4 is the project's allowance for another summation order and the device's exp
(tests/test_gpu_variance.py), and 2^-23 is the spacing of the fp32 number the result is stored in - some yardsticks fall below it by luck of
cancellation.  Kind 3 (the robust focal form) is held to kind 2's fixture: the reference returns bitwise equal results for the two.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
from conftest import ROOT

pytestmark = pytest.mark.gpu

FACTOR = 4.0
ULP = 2.0 ** -23
CASES = [(c, s) for c in ('A', 'B', 'C', 'T') for s in ('s3', 's005')]


def _entry(logits, label, kind, beta=1.0, dmask=None, total=None):
    """cdnet_boundary_loss on device tensors -> loss tensor [1]"""
    import torch
    from cdnet_amd import _lib
    B, K, H, W = logits.shape
    need = _lib.load().cdnet_boundary_loss_workspace_bytes(kind, B, K, H, W)
    assert need > 0
    ws = torch.empty(((need + 3) // 4,), dtype=torch.float32, device=logits.device)
    out = torch.full((1,), -7.0, dtype=torch.float32, device=logits.device)
    _lib.call('cdnet_boundary_loss', _lib.ptr(logits), _lib.ptr(label), kind, B, K, H, W, float(beta), _lib.ptr(ws), need, _lib.ptr(out),
              _lib.ptr(total), _lib.ptr(dmask), _lib.stream_ptr())
    return out


def _value_and_grad(logits, label, kind, beta=1.0):
    import torch
    dmask = torch.zeros_like(logits)
    out = _entry(logits, label, kind, beta, dmask)
    torch.cuda.synchronize()
    return out, dmask


def _case(golden, case, scale):
    import torch
    g = golden('boundary')
    dev = torch.device('cuda:0')
    return g, torch.from_numpy(g['%s/%s/logits' % (case, scale)]).to(dev), torch.from_numpy(g[case + '/label']).to(dev)


@pytest.mark.parametrize('kind', [1, 2, 3])
@pytest.mark.parametrize('case,scale', CASES)
def test_loss_and_gradient_against_float64(golden, case, scale, kind):
    """every fixture case; T is the one that fails when a tie of either pool goes to another pixel than the first in raster order"""
    g, logits, label = _case(golden, case, scale)
    key = '%s/%s/k%d/' % (case, scale, min(kind, 2))
    loss64, grad64 = float(g[key + 'loss64']), g[key + 'grad64']
    eloss32, egrad32 = float(g[key + 'eloss32']), float(g[key + 'egrad32'])
    out, dmask = _value_and_grad(logits, label, kind)
    eloss = abs(float(out[0]) - loss64) / abs(loss64)
    egrad = np.abs(dmask.cpu().numpy().astype(np.float64) - grad64).max() / np.abs(grad64).max()
    print('%s %s kind %d: eloss %.3e (reference float32 %.3e)  egrad %.3e (reference float32 %.3e)' % (case, scale, kind, eloss, eloss32, egrad, egrad32))
    assert eloss <= FACTOR * max(eloss32, ULP), (eloss, eloss32)
    assert egrad <= FACTOR * max(egrad32, ULP), (egrad, egrad32)


@pytest.mark.parametrize('kind', [2, 3])
def test_saturated_sigmoid_follows_the_float32_reference(golden, kind):
    """case S, logits randn * 12: float32's clamp bound 1 - 1e-8 is 1 and 1 - sigmoid is 0 from z = 17 on, so the reference's float32 value
    (not float64, 3e-3 away) is what a float32 training run sees"""
    import torch
    g, logits, label = _case(golden, 'S', 's12')
    want = float(g['S/s12/k2/loss32'])
    out, dmask = _value_and_grad(logits, label, kind)
    err = abs(float(out[0]) - want) / abs(want)
    print('S kind %d: loss %.9e, reference float32 %.9e, relative %.3e' % (kind, float(out[0]), want, err))
    assert err <= FACTOR * ULP, (float(out[0]), want)
    assert bool(torch.isfinite(dmask).all())


def test_constant_logits_give_loss_one_and_no_gradient(golden):
    import torch
    _, logits, label = _case(golden, 'A', 's3')
    flat = torch.full_like(logits, 0.25)
    flat[:, 1] = -1.5                                                      # constant per channel: p is constant, pr_b = 0 everywhere
    out, dmask = _value_and_grad(flat, label, 1)
    assert float(out[0]) == 1.0
    assert not bool(dmask.any())


def test_all_background_sample_contributes_one_per_class(golden):
    """sample 1 of A has no boundary: R = 0, BF1 = 0 for each class - exactly 3 / (B K) of the loss, and no gradient"""
    import torch
    _, logits, label = _case(golden, 'A', 's3')
    assert not bool(label[1].any())
    alone, dalone = _value_and_grad(logits[1:].contiguous(), label[1:].contiguous(), 1)
    assert float(alone[0]) == 1.0                                          # B = 1: 3 / (1 * 3)
    assert not bool(dalone.any())
    first, _ = _value_and_grad(logits[:1].contiguous(), label[:1].contiguous(), 1)
    both, dboth = _value_and_grad(logits, label, 1)
    # B = 2: (sum over sample 0's classes + 3) / 6 with sample 0's three values as the B = 1 call forms them; one rounding each side
    want = (3.0 * float(first[0]) + 3.0) / 6.0
    assert abs(float(both[0]) - want) <= 2 * float(np.spacing(np.float32(want))), (float(both[0]), want)
    assert not bool(dboth[1].any())


@pytest.mark.parametrize('case,scale', [('A', 's3'), ('T', 's005'), ('S', 's12')])
def test_robust_focal_is_bitwise_the_focal_term(golden, case, scale):
    import torch
    _, logits, label = _case(golden, case, scale)
    o2, d2 = _value_and_grad(logits, label, 2)
    o3, d3 = _value_and_grad(logits, label, 3)
    assert float(o2[0]) > 0 and torch.equal(o2, o3) and torch.equal(d2, d3)


@pytest.mark.parametrize('kind', [1, 2])
def test_accumulates_into_dmask_and_total(golden, kind):
    import torch
    _, logits, label = _case(golden, 'A', 's3')
    out, grad = _value_and_grad(logits, label, kind)
    gen = torch.Generator().manual_seed(5)
    prefill = (torch.randn(logits.shape, generator=gen) * 1e-3).to(logits.device)
    dmask = prefill.clone()
    total = torch.full((1,), 3.0, dtype=torch.float32, device=logits.device)
    out2 = _entry(logits, label, kind, 1.0, dmask, total)
    out3 = _entry(logits, label, kind, 1.0, None, None)
    torch.cuda.synchronize()
    assert float(out[0]) > 0 and torch.equal(out, out2) and torch.equal(out, out3)
    # one float32 addition per element / for the total: the float32 rounding of the sum and nothing else
    assert torch.equal(dmask, prefill + grad)
    assert torch.equal(total, torch.full_like(total, 3.0) + out)
    # beta scales what is added, not the value
    half = torch.zeros_like(logits)
    total = torch.full((1,), 3.0, dtype=torch.float32, device=logits.device)
    out4 = _entry(logits, label, kind, 0.5, half, total)
    torch.cuda.synchronize()
    assert torch.equal(out4, out)
    assert torch.equal(total, torch.full_like(total, 3.0) + 0.5 * out)
    scale = float(grad.abs().max())
    assert float((half - 0.5 * grad).abs().max()) <= 2.0 ** -23 * scale      # the product is rounded once, from double


@pytest.mark.parametrize('kind,case', [(1, 'A'), (1, 'C'), (2, 'C')])
def test_two_calls_are_bit_identical(golden, kind, case):
    import torch
    _, logits, label = _case(golden, case, 's005')
    runs = [_value_and_grad(logits, label, kind) for _ in range(2)]
    assert float(runs[0][0][0]) > 0
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_gradient_kernel_uses_no_scratch():
    from cdnet_amd import _lib
    assert _lib.load().cdnet_boundary_loss_scratch_bytes() == 0


@pytest.mark.parametrize('kind', [1, 2])
def test_label_out_of_range_gives_nan(golden, kind):
    """argument handling, as cdnet_dam_loss: a label above 2 matches no class and indexes nothing; the value is NaN"""
    import torch
    _, logits, label = _case(golden, 'B', 's3')
    bad = label.clone()
    bad[0, 6, 6] = 3
    out, _ = _value_and_grad(logits, bad, kind)
    assert bool(torch.isnan(out[0]))
    good, _ = _value_and_grad(logits, label, kind)
    assert bool(torch.isfinite(good[0]))


# --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def fp32():
    import cdnet_amd
    old = cdnet_amd.get_precision()
    cdnet_amd.set_precision('fp32')
    yield
    cdnet_amd.set_precision(old)


class _Opt:
    model = {'out_c': 3}


def _make(which, seed=3):
    """(trainer, step) of one of the four trainers on fresh, equally seeded weights; step(batch) -> (mask logits, dmask, total [1])"""
    import torch
    from cdnet_amd import trainer
    torch.manual_seed(seed)
    if which == 'unet':
        from cdnet_amd.models.unet import UNet
        tr = trainer.UNetTrainer(UNet(num_classes=3).cuda())

        def step(b):
            logits = tr.forward(b[0])
            return logits, tr.loss_and_grads(logits, b[1], b[4]), tr.unet_losses[0:1]
    elif which == 'MandD':
        from cdnet_amd.models.dam.model_unet_MandD import Unet
        tr = trainer.AblationTrainer(Unet(backbone_name='vgg16_bn', pretrained=False, classes=3).cuda())

        def step(b):
            out = tr.forward(b[0])
            return out[0], tr.loss_and_grads(out, *b[1:])[0], tr.losses[0:1]
    else:
        if which == 'hrnet':
            from cdnet_amd.models.dam.seg_hrnet_rev1 import HighResolutionNet
            model = HighResolutionNet(_Opt()).cuda()
        else:
            from cdnet_amd.models.dam.model_unet_rev1 import Unet
            model = Unet(backbone_name='vgg16_bn', pretrained=False, classes=3).cuda()
        tr = trainer.Trainer(model)

        def step(b):
            out = tr.forward(b[0])
            return out[0], tr.loss_and_grads(out[0], out[1], out[2], *b[1:])[0], tr.losses[0:1]
    return tr, step


def _batch(B=2, S=64, seed=2022):
    import torch
    from cdnet_amd import synth
    return synth.synthetic_batch(B, torch.device('cuda:0'), seed=seed, H=S, W=S)


def _run(which, boundary, alpha=0.0):
    import torch
    tr, step = _make(which)
    tr.boundary, tr.alpha = boundary, alpha
    batch = _batch()
    mask, dmask, total = step(batch)
    torch.cuda.synchronize()
    return dict(mask=mask.clone(), dmask=dmask.clone(), total=float(total[0]), lb=float(tr.loss_boundary[0]), lv=float(tr.loss_var[0]),
                label=batch[1])


@pytest.mark.parametrize('which,kind', [('rev1', 1), ('rev1', 2), ('rev1', 3), ('unet', 1), ('MandD', 2), ('hrnet', 1)])
def test_trainers_add_the_term_to_total_and_mask_gradient(fp32, which, kind):
    import torch
    off, on = _run(which, 0), _run(which, kind)
    assert torch.equal(off['mask'], on['mask'])
    assert off['lb'] == 0.0 and on['lb'] > 0.0
    # the total: one float32 addition in the entry (and one more for the plain UNet's own total): two roundings of the total
    assert abs((on['total'] - off['total']) - on['lb']) <= 2 * float(np.spacing(np.float32(on['total']))), (off['total'], on['total'], on['lb'])
    out, grad = _value_and_grad(on['mask'], on['label'], kind)
    assert float(out[0]) == on['lb']
    assert float(grad.abs().max()) > 0
    assert torch.equal(on['dmask'], off['dmask'] + grad)                  # one float32 addition per element


def test_no_boundary_entry_is_called_when_the_option_is_off(fp32, monkeypatch):
    import torch
    from cdnet_amd import _lib
    seen = []
    real = _lib.call

    def recorder(name, *args):
        seen.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, 'call', recorder)
    tr, _ = _make('rev1')
    batch = _batch()
    tr.train_step(*batch)
    torch.cuda.synchronize()
    assert 'cdnet_dam_loss_classes' in seen and not [n for n in seen if 'boundary' in n]
    del seen[:]
    tr.boundary = 1
    tr.train_step(*batch)
    torch.cuda.synchronize()
    assert seen.count('cdnet_boundary_loss') == 1


def test_boundary_and_variance_terms_add_up(fp32):
    import torch
    off, var, bnd, both = _run('rev1', 0), _run('rev1', 0, 1.0), _run('rev1', 1), _run('rev1', 1, 1.0)
    assert both['lv'] == var['lv'] > 0 and both['lb'] == bnd['lb'] > 0
    assert abs((both['total'] - off['total']) - (both['lv'] + both['lb'])) <= 3 * float(np.spacing(np.float32(both['total'])))
    # the variance term is added first, then the boundary term: one float32 addition each
    assert torch.equal(both['dmask'], var['dmask'] + _value_and_grad(both['mask'], both['label'], 1)[1])
    assert torch.equal(bnd['dmask'], off['dmask'] + _value_and_grad(both['mask'], both['label'], 1)[1])


def test_graphed_step_with_the_term_is_bit_identical_to_eager(fp32):
    """the term's two launches (no host synchronisation) replay from cdnet_amd.graphs.GraphedTrainStep's graph"""
    import torch
    from cdnet_amd.graphs import GraphedTrainStep
    batch = _batch()
    res = []
    for graphed in (False, True):
        tr, _ = _make('rev1')
        tr.boundary = 1
        if graphed:
            g = GraphedTrainStep(tr, batch, warmup=2)            # 2 eager steps + the first replayed one
            g(*batch)
        else:
            for _ in range(4):
                tr.train_step(*batch)
        torch.cuda.synchronize()
        res.append((tr.losses.clone(), tr.loss_boundary.clone(), tr.flat.P.clone()))
    assert float(res[0][1][0]) > 0
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)


def test_validate_adds_the_value_whole_and_split(fp32, golden):
    """validate() with boundary_loss = 1: slot 0 = the boundary_loss = 0 value + the entry's loss on the logits validate saw - the eval forward
    of the whole tile, and split_forward_dam's stitched logits (the validate fixture's geometry: 96 x 96, windows of 64, overlap 16)"""
    import torch
    from cdnet_amd import synth, train_util_dam, utils
    from cdnet_amd.models.dam.model_unet_rev1 import Unet
    from cdnet_amd.options import Options
    z = golden('validate')
    B, _, H, W, seed = [int(v) for v in z['x_cfg']]
    size, ov = [int(v) for v in z['win_cfg']]
    lab, dirn, point, weight = synth.train_targets(B, H, W, int(z['tgt_cfg'][3]))
    x = torch.from_numpy(synth.det_input((B, 3, H, W), seed))
    torch.manual_seed(3)
    m = Unet(backbone_name='vgg16_bn', pretrained=False, classes=3).cuda()
    target0 = torch.from_numpy(lab.astype(np.int64) * 127 + (lab == 2)).unsqueeze(1)
    sample = (x, torch.from_numpy(weight), target0, torch.from_numpy(point), torch.from_numpy(dirn))
    label = torch.from_numpy(lab).cuda()

    def run(kind, smp, whole):
        opt = Options(isTrain=True).parse([])
        opt.train['input_size'], opt.train['val_overlap'], opt.model['boundary_loss'] = size, ov, kind
        return train_util_dam.validate([smp], m, None, opt, None, all_img_test=1 if whole else 0)
    m.eval()
    with torch.no_grad():
        mask = m(x.cuda())[0].contiguous()
    want = float(_entry(mask, label, 1)[0])
    off, on = run(0, sample, True), run(1, sample, True)
    assert want > 0 and abs((on[0] - off[0]) - want) <= 1e-9 * abs(on[0]), (off[0], on[0], want)
    assert np.array_equal(off[1:], on[1:])
    one = tuple(t[:1] for t in sample)
    mask = utils.split_forward_dam(m, x[:1], size, ov, None)[0].contiguous()
    want = float(_entry(mask, label[:1].contiguous(), 1)[0])
    off, on = run(0, one, False), run(1, one, False)
    assert want > 0 and abs((on[0] - off[0]) - want) <= 1e-9 * abs(on[0]), (off[0], on[0], want)
    assert np.array_equal(off[1:], on[1:])


def test_train_entry_runs_with_the_option(tmp_path):
    """python -m cdnet_amd.train --boundary-loss 1 in a child process under its own time limit: finite losses, and another logged total than
    the --boundary-loss 0 run of the same seed (run here, in this process)"""
    from cdnet_amd import train
    args = ['--synthetic', '4', '--epochs', '1', '--batch-size', '2']
    cmd = ['timeout', '-k', '10', '300', sys.executable, '-m', 'cdnet_amd.train'] + args + ['--boundary-loss', '1', '--save-dir', str(tmp_path / 'on')]
    env = dict(os.environ)
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=330, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    logged = re.findall(r'^epoch 1: loss (\S+)', r.stdout, flags=re.M)
    assert len(logged) == 1, r.stdout[-2000:]
    avg = re.findall(r'Train Avg: Loss (\S+)\s+loss_CE (\S+)', r.stdout)
    assert len(avg) == 1 and all(np.isfinite(float(v)) for v in avg[0] + (logged[0],)), r.stdout[-2000:]
    off = train.main(args + ['--boundary-loss', '0', '--save-dir', str(tmp_path / 'off')])
    assert np.isfinite(off).all()
    # the boundary term starts near 1 (BF1 near 0 at initialisation); the other terms see the same first batch
    assert float(logged[0]) > float(off[0]) + 0.1, (logged[0], off[0])
