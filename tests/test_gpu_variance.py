"""The instance variance term (--alpha 1) on the GPU: cdnet_variance_loss against the reference's LossVariance evaluated in float64
(tests/golden/variance.npz, written by tests/golden/make_golden_variance.py from the reference itself), and the term inside the trainers.

The bar of every float comparison is the reference's OWN float32 error against float64 on the same inputs (`eloss32`, `egrad32`, stored in
the fixture or, for the trainer's logits, computed here from a float32 run of the restated formula on the CPU) times 4: another summation
order and the device's exp, a few ulp each.  Integer results (root map, instance counts) and everything the fixture holds as exactly 0 are exact.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = [(c, s) for c in ('A', 'A2', 'B', 'C') for s in ('s3', 's005')]
FACTOR = 4.0


def _variance(logits, label, alpha=1.0, dmask=None, total=None, want_roots=False):
    """cdnet_variance_loss on device tensors -> (loss_var tensor [1], root map or None, counts or None)"""
    import torch
    from cdnet_amd import _lib
    B, K, H, W = logits.shape
    need = _lib.load().cdnet_variance_loss_workspace_bytes(B, K, H, W)
    assert need > 0
    ws = torch.empty(((need + 3) // 4,), dtype=torch.float32, device=logits.device)
    out = torch.full((1,), -7.0, dtype=torch.float32, device=logits.device)
    roots = torch.full((B, H, W), -9, dtype=torch.int32, device=logits.device) if want_roots else None
    counts = torch.full((B,), -9, dtype=torch.int32, device=logits.device) if want_roots else None
    _lib.call('cdnet_variance_loss', _lib.ptr(logits), _lib.ptr(label), 1, B, K, H, W, float(alpha), _lib.ptr(ws), need, _lib.ptr(out),
              _lib.ptr(total), _lib.ptr(dmask), _lib.ptr(roots), _lib.ptr(counts), _lib.stream_ptr())
    return out, roots, counts


def _case(golden, case, scale):
    import torch
    g = golden('variance')
    dev = torch.device('cuda:0')
    logits = torch.from_numpy(g['%s/%s/logits' % (case, scale)]).to(dev)
    label = torch.from_numpy(g[case + '/label']).to(dev)
    return g, logits, label


@pytest.mark.parametrize('case', ['A', 'A2', 'B', 'C'])
def test_labelling_matches_the_reference(golden, case):
    import torch
    g, logits, label = _case(golden, case, 's3')
    _, roots, counts = _variance(logits, label, want_roots=True)
    torch.cuda.synchronize()
    assert np.array_equal(counts.cpu().numpy(), g[case + '/U'])
    assert np.array_equal(roots.cpu().numpy(), g[case + '/root'])


@pytest.mark.parametrize('case,scale', CASES)
def test_loss_and_gradient_against_float64(golden, case, scale):
    import torch
    g, logits, label = _case(golden, case, scale)
    key = '%s/%s/' % (case, scale)
    loss64, grad64 = float(g[key + 'loss64']), g[key + 'grad64']
    eloss32, egrad32 = float(g[key + 'eloss32']), float(g[key + 'egrad32'])
    dmask = torch.zeros_like(logits)
    total = torch.zeros((1,), dtype=torch.float32, device=logits.device)
    out, _, _ = _variance(logits, label, 1.0, dmask, total)
    torch.cuda.synchronize()
    lv, dm = float(out[0]), dmask.cpu().numpy().astype(np.float64)
    assert float(total[0]) == lv
    if loss64 == 0.0:
        assert eloss32 == 0.0 and egrad32 == 0.0
        assert lv == 0.0 and not dm.any()
        return
    eloss = abs(lv - loss64) / abs(loss64)
    egrad = np.abs(dm - grad64).max() / np.abs(grad64).max()
    print('%s %s: eloss %.3e (reference float32 %.3e)  egrad %.3e (reference float32 %.3e)' % (case, scale, eloss, eloss32, egrad, egrad32))
    for k in range(grad64.shape[0]):                      # a sample the fixture holds as exactly 0 (no foreground) stays exactly 0
        if not grad64[k].any():
            assert not dm[k].any(), k
    assert eloss <= FACTOR * eloss32, (eloss, eloss32)
    assert egrad <= FACTOR * egrad32, (egrad, egrad32)


def test_accumulates_into_dmask_and_total(golden):
    import torch
    _, logits, label = _case(golden, 'A', 's3')
    grad = torch.zeros_like(logits)
    out, _, _ = _variance(logits, label, 1.0, grad, None)
    gen = torch.Generator().manual_seed(5)
    prefill = (torch.randn(logits.shape, generator=gen) * 1e-3).to(logits.device)
    dmask = prefill.clone()
    total = torch.full((1,), 3.0, dtype=torch.float32, device=logits.device)
    out2, _, _ = _variance(logits, label, 1.0, dmask, total)
    out3, _, _ = _variance(logits, label, 1.0, None, None)
    torch.cuda.synchronize()
    assert float(out[0]) > 0 and torch.equal(out, out2) and torch.equal(out, out3)
    # one float32 addition per element / for the total: the float32 rounding of the sum and nothing else
    assert torch.equal(dmask, prefill + grad)
    assert torch.equal(total, torch.full_like(total, 3.0) + out)


@pytest.mark.parametrize('case', ['A', 'C'])
def test_two_calls_are_bit_identical(golden, case):
    import torch
    _, logits, label = _case(golden, case, 's005')
    runs = []
    for _ in range(2):
        dmask = torch.zeros_like(logits)
        out, _, _ = _variance(logits, label, 1.0, dmask, None)
        runs.append((out, dmask))
    torch.cuda.synchronize()
    assert float(runs[0][0][0]) > 0
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


# --------------------------------------------------------------------------------------------------------------------------
def _restated(logits, label, dtype):
    """the term as the issue states it, on the CPU in `dtype`: softmax, 8-connected instances of label == 1, unbiased variance per instance
    with n > 1 and channel, / (U + 1e-8), mean over the batch; -> (loss, d loss / d logits) as float64"""
    import torch
    from scipy import ndimage as ndi
    z = logits.detach().cpu().to(dtype).requires_grad_(True)
    p = torch.softmax(z, dim=1)
    lab = label.cpu().numpy()
    B = z.shape[0]
    loss = torch.zeros((), dtype=dtype)
    multi = []
    for k in range(B):
        L, U = ndi.label(lab[k] == 1, structure=np.ones((3, 3), dtype=int))
        s = torch.zeros((), dtype=dtype)
        multi.append(0)
        for i in range(1, U + 1):
            q = p[k][:, torch.from_numpy(L == i)]
            n = q.shape[1]
            if n > 1:
                multi[-1] += 1
                s = s + ((q - q.mean(dim=1, keepdim=True)) ** 2).sum() / (n - 1)
        loss = loss + s / (U + 1e-8)
    loss = loss / B
    loss.backward()
    return float(loss.detach().double()), z.grad.double().numpy(), multi


def _rev1(seed=3):
    import torch
    from cdnet_amd.models.dam.model_unet_rev1 import Unet
    torch.manual_seed(seed)
    return Unet(backbone_name='vgg16_bn', pretrained=False, classes=3).cuda()


def _batch(B=2, S=64, seed=2022):
    import torch
    from cdnet_amd import synth
    return synth.synthetic_batch(B, torch.device('cuda:0'), seed=seed, H=S, W=S)


def test_trainer_adds_the_term_to_loss_and_mask_gradient():
    import torch
    from cdnet_amd import trainer
    batch = _batch()
    res = {}
    for alpha in (0.0, 1.0):
        tr = trainer.Trainer(_rev1())
        tr.alpha = alpha
        out = tr.forward(batch[0])
        g = tr.loss_and_grads(out[0], out[1], out[2], *batch[1:])
        torch.cuda.synchronize()
        res[alpha] = dict(mask=out[0].clone(), dmask=g[0].clone(), losses=tr.losses.clone(), loss_var=tr.loss_var.clone())
    a0, a1 = res[0.0], res[1.0]
    assert torch.equal(a0['mask'], a1['mask'])
    assert float(a0['loss_var'][0]) == -1.0
    lv = float(a1['loss_var'][0])
    l0, l1 = float(a0['losses'][0]), float(a1['losses'][0])
    assert abs((l1 - l0) - lv) <= float(np.spacing(np.float32(l1)))          # one float32 addition into losses[0]
    assert float(a1['losses'][5]) == float(a0['losses'][5])                   # slot 5 is still the dice term
    loss64, grad64, multi = _restated(a1['mask'], batch[1], torch.float64)
    loss32, grad32, _ = _restated(a1['mask'], batch[1], torch.float32)
    assert min(multi) >= 2, multi                                             # the batch exercises the term in every sample
    eloss32 = abs(loss32 - loss64) / abs(loss64)
    egrad32 = np.abs(grad32 - grad64).max() / np.abs(grad64).max()
    eloss = abs(lv - loss64) / abs(loss64)
    diff = (a1['dmask'] - a0['dmask']).cpu().numpy().astype(np.float64)
    egrad = np.abs(diff - grad64).max() / np.abs(grad64).max()
    print('trainer: eloss %.3e (float32 restatement %.3e)  egrad %.3e (float32 restatement %.3e)' % (eloss, eloss32, egrad, egrad32))
    assert eloss <= FACTOR * eloss32, (eloss, eloss32)
    assert egrad <= FACTOR * egrad32, (egrad, egrad32)


def test_train_step_with_the_term_is_bit_identical_from_run_to_run():
    import torch
    from cdnet_amd import trainer
    batch = _batch()
    runs = []
    for _ in range(2):
        tr = trainer.Trainer(_rev1())
        tr.alpha = 1.0
        losses = tr.train_step(*batch).clone()
        torch.cuda.synchronize()
        runs.append((losses, tr.loss_var.clone(), tr.flat.P.clone()))
    assert float(runs[0][1][0]) > 0 and bool(torch.isfinite(runs[0][0]).all())
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)


def test_graphed_step_with_the_term_is_bit_identical_to_eager():
    """the term's launches (a memset node and six kernels, no host synchronisation) replay from cdnet_amd.graphs.GraphedTrainStep's graph"""
    import torch
    from cdnet_amd import trainer
    from cdnet_amd.graphs import GraphedTrainStep
    batch = _batch()
    res = []
    for graphed in (False, True):
        tr = trainer.Trainer(_rev1())
        tr.alpha = 1.0
        if graphed:
            g = GraphedTrainStep(tr, batch, warmup=2)            # 2 eager steps + the first replayed one
            g(*batch)
        else:
            for _ in range(4):
                tr.train_step(*batch)
        torch.cuda.synchronize()
        res.append((tr.losses.clone(), tr.loss_var.clone(), tr.flat.P.clone()))
    assert float(res[0][1][0]) > 0
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)


def test_train_entry_logs_the_term():
    """train_util_dam.train over two batches with alpha 1 and alpha 0.  The learning rate is 0 so that both runs see the same weights in the
    second batch too: only then is the difference of the two totals the variance term."""
    import torch
    from cdnet_amd import train_util_dam, utils
    from cdnet_amd.options import Options
    from cdnet_amd.train import _SyntheticLoader
    loader = _SyntheticLoader(2, 2, torch.device('cuda:0'), seed=2022, size=64)
    r = {}
    for alpha in (0, 1):
        opt = Options(isTrain=True)
        opt.train['alpha'], opt.train['lr'] = alpha, 0.0
        tr, _ = utils.get_optimizer(opt, _rev1())
        assert tr.alpha == alpha
        r[alpha] = train_util_dam.train(loader, tr.model, tr, None, 0, opt, None)
    assert r[0][5] == -1.0
    assert r[1][5] >= 0.0
    assert abs((r[1][0] - r[0][0]) - r[1][5]) <= 1e-6 * abs(r[1][0]), (r[0][0], r[1][0], r[1][5])
    assert r[1][5] > 0.0                                                      # the synthetic nuclei are not uniform in p at initialisation


def test_plain_unet_total_includes_the_term():
    import torch
    from cdnet_amd import trainer
    from cdnet_amd.models.unet import UNet
    torch.manual_seed(3)
    tr = trainer.UNetTrainer(UNet(num_classes=3).cuda())
    tr.alpha = 1.0
    x, lab, _, _, weight = _batch()
    u = tr.train_step(x, lab, weight).clone()
    torch.cuda.synchronize()
    lv = float(tr.loss_var[0])
    assert lv > 0.0
    want = np.float64(float(u[1])) + float(u[2]) + lv
    assert abs(float(u[0]) - want) <= 2 * float(np.spacing(np.float32(want))), (u.tolist(), lv)   # two float32 additions
