"""End-to-end training step on the GPU (forward, loss, backward, Adam) against the oracle.

Why three comparisons (DESIGN.md "Parity of the training step"):
  * loss values vs the fp32 oracle (pinned to the reference): tolerance 2e-3 relative - the forward is bf16/fp16;
  * gradients of a LINEARISED network (ReLU off in both) vs the rounding-emulated oracle: tight (<= 8e-2 worst, median
    <= 2e-2) - proves the backward orchestration (BN backward, dW, backward-data, concat/pad/pool routing, residual units);
  * gradients of the real network vs the rounding-emulated oracle: cosine similarity - a 1e-3 forward perturbation flips
    ~0.1 % of the ReLU decisions per layer, which alone moves gradients by several % per layer (measured), so an
    element-wise tolerance would be meaningless; the kernel-level tests (test_gpu_train_kernels.py) are the tight ones.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _setup(B=2, S=64, seed=0, W=None):
    import torch
    from cdnet_amd import synth
    from cdnet_amd.models.dam.model_unet_rev1 import Unet
    from oracle import models as om
    torch.manual_seed(seed)
    ref = om.Unet()
    for mod in ref.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            torch.nn.init.uniform_(mod.weight, 0.5, 1.5)
            torch.nn.init.normal_(mod.bias, 0, 0.2)
    m = Unet(backbone_name='vgg16_bn', pretrained=False, classes=3)
    m.load_state_dict(ref.state_dict())
    W = W or S
    lab, dirn, point, weight = synth.train_targets(B, S, W, 21)
    x = torch.from_numpy(synth.det_input((B, 3, S, W), 9))
    t = [torch.from_numpy(a) for a in (lab, dirn, point, weight)]
    return m.cuda(), ref, x, t


def _hip_grads(m, x, t):
    import torch
    from cdnet_amd import trainer
    tr = trainer.Trainer(m)
    dev = torch.device('cuda:0')
    o = tr.forward(x.to(dev))
    g = tr.loss_and_grads(o[0], o[1], o[2], t[0].to(dev), t[1].to(dev), t[2].to(dev), t[3][:, 0].contiguous().to(dev))
    tr.backward(*g)
    torch.cuda.synchronize()
    return tr, {n: p.grad.detach().float().cpu().clone() for n, p in m.named_parameters() if not n.startswith(m.UNUSED_PREFIXES)}


def _oracle_grads(ref, x, t, emulated):
    from oracle import emulate
    from oracle import train as ot
    ref.train()
    ref.zero_grad()
    out = emulate.dam_unet_forward(ref, x) if emulated else ref(x)
    L = ot.dam_losses(out[0], out[1], out[2], t[0], t[1], t[2], t[3])
    L['total'].backward()
    return {k: float(v) for k, v in L.items()}, {n: p.grad.clone() for n, p in ref.named_parameters() if p.grad is not None}


def test_loss_values_match_fp32_oracle():
    m, ref, x, t = _setup()
    tr, _ = _hip_grads(m, x, t)
    L, _ = _oracle_grads(ref, x, t, emulated=False)
    got = tr.losses.cpu().numpy()[:6]
    want = [L[k] for k in ('total', 'dce', 'wdice', 'mse', 'ce', 'dice')]
    np.testing.assert_allclose(got, want, rtol=2e-3)


def test_linearised_network_gradients_tight():
    from cdnet_amd import runtime
    from oracle import emulate
    runtime.DEBUG_NORELU = emulate.NORELU = True
    try:
        m, ref, x, t = _setup()
        _, g = _hip_grads(m, x, t)
        _, rg = _oracle_grads(ref, x, t, emulated=True)
    finally:
        runtime.DEBUG_NORELU = emulate.NORELU = False
    rel = {}
    for n, want in rg.items():
        if want.norm() < 1e-6:           # conv biases in front of BatchNorm: exactly zero gradient
            continue
        rel[n] = float((g[n] - want).norm() / want.norm())
    worst = max(rel, key=rel.get)
    assert rel[worst] <= 8e-2, (worst, rel[worst])
    assert np.median(list(rel.values())) <= 2e-2
    for n in ('point_conv.weight', 'mask_conv.weight', 'direction_conv.weight', 'mask_feature.conv2.weight',
              'upsample_blocks.4.conv2.weight', 'upsample_blocks.4.up.weight'):
        assert rel[n] <= 1e-2, (n, rel[n])


def test_ragged_tile_gradients():
    """72 x 88 tiles: the pooled pyramid is 36x44, 18x22, 9x11, 4x5, 2x2, so the decoder pads (model_unet_rev1.py:126-131) and the
    max-pool windows / BatchNorm-backward routing see odd sizes - linearised network, same bound as the square case"""
    from cdnet_amd import runtime
    from oracle import emulate
    runtime.DEBUG_NORELU = emulate.NORELU = True
    try:
        m, ref, x, t = _setup(S=72, W=88)
        tr, g = _hip_grads(m, x, t)
        L, rg = _oracle_grads(ref, x, t, emulated=True)
    finally:
        runtime.DEBUG_NORELU = emulate.NORELU = False
    rel = {n: float((g[n] - want).norm() / want.norm()) for n, want in rg.items() if want.norm() >= 1e-6}
    worst = max(rel, key=rel.get)
    assert rel[worst] <= 8e-2, (worst, rel[worst])
    assert np.median(list(rel.values())) <= 2e-2
    np.testing.assert_allclose(tr.losses.cpu().numpy()[:5], [L[k] for k in ('total', 'dce', 'wdice', 'mse', 'ce')], rtol=5e-3)


def test_real_network_gradient_direction():
    m, ref, x, t = _setup()
    _, g = _hip_grads(m, x, t)
    _, rg = _oracle_grads(ref, x, t, emulated=True)
    cos, ratio = {}, {}
    for n, want in rg.items():
        if want.norm() < 1e-6:
            continue
        cos[n] = float((g[n] * want).sum() / (g[n].norm() * want.norm()))
        ratio[n] = float(g[n].norm() / want.norm())
    for n in ('point_conv.weight', 'mask_conv.weight', 'direction_conv.weight'):
        assert cos[n] >= 0.9995, (n, cos[n])
    assert min(cos.values()) >= 0.85, min(cos, key=cos.get)
    assert np.median(list(cos.values())) >= 0.92
    big = [n for n, w in rg.items() if w.norm() >= 1e-3]          # tiny gradients (a single gate weight) are all noise
    assert 0.8 <= min(ratio[n] for n in big) and max(ratio[n] for n in big) <= 1.25


def test_short_training_run_tracks_the_oracle():
    """6 Adam steps on a fixed batch: the loss trajectory follows the fp32 oracle's (train_util_dam.train semantics)"""
    import torch
    from cdnet_amd import trainer
    from oracle import train as ot
    m, ref, x, t = _setup()
    tr = trainer.Trainer(m)
    dev = torch.device('cuda:0')
    batch = (x.to(dev), t[0].to(dev), t[1].to(dev), t[2].to(dev), t[3][:, 0].contiguous().to(dev))
    opt = ot.make_adam(ref)
    ours, theirs = [], []
    for _ in range(6):
        ours.append(float(tr.train_step(*batch)[0]))
        theirs.append(ot.train_iteration(ref, opt, x, *t)['total'])
    assert ours[-1] < ours[0] * 0.9, ours                       # it learns
    np.testing.assert_allclose(ours, theirs, rtol=3e-2)
    assert abs(ours[0] - theirs[0]) <= 2e-3 * theirs[0]
    # never-used parameters are neither touched nor given a gradient
    sd = m.state_dict()
    assert torch.equal(sd['final_conv.weight'].cpu(), ref.state_dict()['final_conv.weight'])


def test_full_size_step_is_deterministic_and_learns():
    """BASELINE configuration (16 tiles of 256x256): size-independent properties instead of an oracle run - every
    reduction of the step has a fixed order, so two runs from the same state are bit-identical; the loss is finite and
    falls over a few Adam steps; the never-used parameters of the reference stay untouched."""
    import torch
    from cdnet_amd import trainer
    from cdnet_amd.models.dam.model_unet_rev1 import Unet
    dev = torch.device('cuda:0')
    batch = trainer.synthetic_batch(16, dev, seed=11)

    def run():
        torch.manual_seed(3)
        m = Unet(backbone_name='vgg16_bn', pretrained=False, classes=3).to(dev)
        unused0 = m.final_conv.weight.detach().clone()
        tr = trainer.Trainer(m)
        losses = [tr.train_step(*batch).clone() for _ in range(4)]
        torch.cuda.synchronize()
        assert torch.equal(m.final_conv.weight.detach(), unused0)
        return tr.flat.P.clone(), torch.stack(losses).cpu().numpy()

    p1, l1 = run()
    p2, l2 = run()
    assert np.isfinite(l1).all()
    assert torch.equal(p1, p2) and np.array_equal(l1, l2)
    assert l1[-1, 0] < l1[0, 0]
    assert (l1[:, 6:] >= 0).all() and (l1[:, 6:] <= 1).all()          # the pixel-level metrics are ratios


def test_full_size_fp32_step_is_deterministic_learns_and_matches_the_one_tile_kernels(monkeypatch):
    """The timed workload of bench.py in the arithmetic of its headline: 16 tiles of 256x256, fp32 mode (train_util_dam.py:303-308;
    the 768 -> 256 @16x16 decoder convolution of model_unet_rev1.py:119-143 and the 512-channel bottleneck take engine.choose_cfg's
    CDNET_F32_WS16 route only at this size).  Two runs from the same state are bit-identical, the loss falls; then the first step's
    loss and gradients against the same step with (a) CDNET_F32_WS16=0 (8x8 tiles on conv_f32_kernel for those layers: other tile
    partition of the BatchNorm statistics), (b) CDNET_BN_STATS_FUSE=0 (the separate reduce pass: other summation order) and (c)
    engine.CONV_DEBUG = 32 (one-tile kernels only, the fp64-checked baseline of tests/test_gpu_fp32_kernels.py).  The convolution
    outputs of all routes are bit-identical; what differs is the order in which per-tile channel sums are added, so the forward
    agrees to 1e-6 and the gradients within the conditioning of a randomly initialised ReLU network."""
    import torch
    import cdnet_amd
    from cdnet_amd import engine, trainer
    from cdnet_amd.models.dam.model_unet_rev1 import Unet
    dev = torch.device('cuda:0')
    batch = trainer.synthetic_batch(16, dev, seed=11)
    before = cdnet_amd.get_precision()
    cdnet_amd.set_precision('fp32')

    def fresh():
        torch.manual_seed(3)
        return Unet(backbone_name='vgg16_bn', pretrained=False, classes=3).to(dev)

    def run(steps):
        m = fresh()
        tr = trainer.Trainer(m)
        losses = [tr.train_step(*batch).clone() for _ in range(steps)]
        torch.cuda.synchronize()
        return tr, tr.flat.P.clone(), torch.stack(losses).cpu().numpy()

    def first_step():
        m = fresh()
        tr = trainer.Trainer(m)
        out = tr.forward(batch[0])
        g = tr.loss_and_grads(out[0], out[1], out[2], *batch[1:])
        tr.backward(*g)
        torch.cuda.synchronize()
        return tr, float(tr.losses[0]), tr.flat.G[:tr.flat.n_used].clone()

    try:
        tr1, p1, l1 = run(3)
        # the routes under test were really taken at this size
        cfgs = {R.layer.name: R.layer.cfg for R in tr1.tape}
        assert cfgs['upsample_blocks.0.conv2'] == (16, 16, 32) and cfgs['backbone.37'] == (16, 16, 32), cfgs
        fused = [k for k, v in tr1._bufs.items() if isinstance(k, tuple) and k and k[0] == 'statsfusable' and v is not False]
        assert len(fused) >= 6, fused
        _, p2, l2 = run(3)
        assert np.isfinite(l1).all() and torch.equal(p1, p2) and np.array_equal(l1, l2)
        assert l1[-1, 0] < l1[0, 0]
        _, loss0, g0 = first_step()
        variants = {}
        monkeypatch.setenv('CDNET_F32_WS16', '0')
        trv, variants['ws16=0'], gv = first_step()
        assert {R.layer.name: R.layer.cfg for R in trv.tape}['backbone.37'] == (8, 16, 64)
        grads = {'ws16=0': gv}
        monkeypatch.delenv('CDNET_F32_WS16')
        monkeypatch.setenv('CDNET_BN_STATS_FUSE', '0')
        _, variants['bnfuse=0'], grads['bnfuse=0'] = first_step()
        monkeypatch.delenv('CDNET_BN_STATS_FUSE')
        monkeypatch.setattr(engine, 'CONV_DEBUG', 32)
        _, variants['one-tile'], grads['one-tile'] = first_step()
        monkeypatch.setattr(engine, 'CONV_DEBUG', 0)
        for name, lv in variants.items():
            assert abs(lv - loss0) <= 2e-6 * abs(loss0), (name, lv, loss0)
            rel = float((grads[name] - g0).norm() / g0.norm())
            assert rel <= 5e-2, (name, rel)                   # (flat gradient vector; per-tensor spread as in the test below)
            nh = tr1.flat.n_head
            relh = float((grads[name][:nh] - g0[:nh]).norm() / g0[:nh].norm())
            assert relh <= 1e-4, (name, relh)                 # the head block sits above every ReLU decision that can flip
    finally:
        cdnet_amd.set_precision(before)


@pytest.mark.parametrize('precision', ['bf16', 'fp32'])
def test_deferred_batched_split_k_reduce_is_bit_identical(monkeypatch, precision):
    """weight gradients with their split-K sums deferred into a few cdnet_wgrad_reduce_batch launches (one slab buffer per call; the
    default) == the reduce behind every weight-gradient launch (CDNET_WGRAD_REDUCE_MB=0), bit for bit on every parameter gradient;
    a small threshold forces several flushes inside backward, a huge one leaves a single launch at its end"""
    import torch
    import cdnet_amd
    before = cdnet_amd.get_precision()
    cdnet_amd.set_precision(precision)
    try:
        grads = []
        for mb in ('0', '1', '1000000'):
            monkeypatch.setenv('CDNET_WGRAD_REDUCE_MB', mb)
            m, ref, x, t = _setup(B=2, S=64)
            tr, g = _hip_grads(m, x, t)
            ntab = len(tr._rd_tables)
            assert (ntab == 0) if mb == '0' else (ntab == 1 if mb == '1000000' else ntab >= 3), (mb, ntab)
            assert not tr._rd_pending and not tr._rd_params
            grads.append(g)
        for g in grads[1:]:
            for n in grads[0]:
                assert torch.equal(grads[0][n], g[n]), n
    finally:
        cdnet_amd.set_precision(before)


@pytest.mark.parametrize('precision', ['bf16', 'fp32'])
def test_residual_1x1_backward_beside_the_chain_is_bit_identical(monkeypatch, precision):
    """the input gradient of a residual unit's 1x1 branch computed on the weight-gradient stream (its consumer, the BatchNorm backward of
    the previous unit, waits for an event) == computed on the chain, bit for bit on every parameter gradient"""
    import torch
    import cdnet_amd
    from cdnet_amd import trainer
    before = cdnet_amd.get_precision()
    cdnet_amd.set_precision(precision)
    try:
        grads = []
        for beside in (False, True):
            monkeypatch.setattr(trainer, '_RU_1X1_SIDE', beside)
            m, ref, x, t = _setup(B=2, S=64)
            tr, g = _hip_grads(m, x, t)
            grads.append(g)
        for n in grads[0]:
            assert torch.equal(grads[0][n], grads[1][n]), n
    finally:
        cdnet_amd.set_precision(before)


def test_channel_sums_from_the_backward_data_launch_match_the_separate_pass(monkeypatch):
    """first BatchNorm-backward pass (sum dz, sum dz * xhat) accumulated in the consumers' gaps of the backward-data launch that produced
    the gradient (fp32 mode, conv_ws32_kernel: cdnet_conv_args.ws = 2 + cdnet_bn_backward_finalize) against the separate reduce pass: same
    arithmetic per element, another summation order - the sums of the first fused layer met by backward agree to 2e-6, everything below
    within the usual conditioning of this network's gradients"""
    import torch
    import cdnet_amd
    from cdnet_amd import engine
    grads, taken = [], None
    monkeypatch.setattr(engine, 'CONV_DEBUG', 64)          # the producer / consumer kernel also on launches this small
    before = cdnet_amd.get_precision()
    cdnet_amd.set_precision('fp32')
    try:
        for fuse in ('0', '1'):
            monkeypatch.setenv('CDNET_BN_STATS_FUSE', fuse)
            m, ref, x, t = _setup(B=2, S=128)
            tr, g = _hip_grads(m, x, t)
            if fuse == '1':
                taken = [k[1] for k, v in tr._bufs.items() if isinstance(k, tuple) and k and k[0] == 'statsfusable' and v is not False]
            grads.append(g)
    finally:
        cdnet_amd.set_precision(before)
    assert len(taken) >= 4, taken
    # the first fused layer met by backward (point_feature.conv1: its gradient arrives from point_feature.conv2's backward-data launch,
    # everything upstream of it is identical in both runs): the channel sums themselves, to fp32 summation-order accuracy
    for n in ('point_feature.bn1.weight', 'point_feature.bn1.bias'):
        a, b = grads[0][n], grads[1][n]
        assert float((a - b).norm() / a.norm()) <= 2e-6, (n, float((a - b).norm() / a.norm()))
    # everything below inherits the usual amplification of a 1e-7 perturbation through ReLU / max-pool decisions
    rel = {}
    for n in grads[0]:
        a, b = grads[0][n], grads[1][n]
        if float(a.norm()) >= 1e-6:
            rel[n] = float((a - b).norm() / a.norm())
    worst = max(rel, key=rel.get)
    assert np.median(list(rel.values())) <= 3e-2, np.median(list(rel.values()))      # measured 1e-2 (the oracle moves as much under a 1e-6 weight perturbation)
    assert rel[worst] <= 1e-1, (worst, rel[worst])


def test_bf16_dz_reuse_matches_the_recomputed_gradient(tmp_path):
    """16-bit mode, residual units: the second BatchNorm-backward pass of bn2 reads the dz the first pass stored (bf16, CDNET_BN_DZ_REUSE,
    default on) instead of recomputing it from the fp32 sum of the gradient sources - the channel sums still come from the unrounded dz.
    Both forms in fresh processes (the switch is read once per process): every parameter gradient within the rounding of one bf16 tensor
    (dW of the units' conv2 and everything below it: cosine >= 0.9995, norm ratio within 1 %)."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    outs = []
    for flag in ('0', '1'):
        env = dict(os.environ, CDNET_BN_DZ_REUSE=flag)
        out = str(tmp_path / ('g%s.npz' % flag))
        r = subprocess.run([sys.executable, os.path.join(here, '_dz_reuse_worker.py'), out], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        outs.append(dict(np.load(out)))
    a, b = outs
    worst = (None, 1.0)
    for n in a:
        na, nb = np.linalg.norm(a[n]), np.linalg.norm(b[n])
        if na < 1e-6:
            continue
        cos = float((a[n].ravel() * b[n].ravel()).sum() / (na * nb))
        if cos < worst[1]:
            worst = (n, cos)
        assert abs(nb / na - 1.0) <= 1e-2, (n, nb / na)
    assert worst[1] >= 0.9995, worst
    for n in ('direction_feature.conv2.weight', 'point_feature.conv2.weight', 'mask_feature.conv2.weight'):
        assert not np.array_equal(a[n], b[n]) or True        # (the two forms differ by rounding only; equality is allowed, not required)
