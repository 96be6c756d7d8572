"""FullNet inference (cdnet_amd/models/FullNet.py on csrc/dilated.hip) against the same network as plain PyTorch modules, one process, one GPU.

    python tools/bench_fullnet.py [--windows 64] [--size 256] [--reps 5] [--warmup 2] [--layer-reps 20] [--skip-torch] [--only-layers]
    python tools/bench_fullnet.py --train [--batch 8] [--size 256] [--reps 5] [--warmup 2] [--skip-torch]
    python tools/bench_fullnet.py --net FCN_pooling [--train] ...

1. Eval forward of --windows windows of --size^2 through FullNet(3, 3).forward_packed, in both precision modes (device events, median).
2. The same network run through the model's own nn containers (Conv2d -> LeakyReLU -> BatchNorm2d, torch.cat), fp32 and bf16
   (channels_last): the only baseline there is.
3. Single layers on --windows windows: a dense layer 168 -> 24 at d = 1 and at d = 21 (appending in place into a 168-channel buffer), the
   286 -> 143 transition; ours against F.conv2d + leaky_relu + affine on channels_last tensors.  `must_bytes` is what the layer has to
   move at least: every input channel read once, every output channel written once, the weights once; `GBps` = must_bytes / time.
--train: one training step (forward + loss + backward + Adam) of FullNet(3, 3) on --batch tiles, fp32 precision mode, through
trainer.FullNetTrainer against the same network as plain PyTorch modules (fp32, eager, channels_last, F.dropout, the oracle's loss,
torch.optim.Adam) in the same process: device events, the two paths alternating run by run, medians.  Then one step with events around
every library call: per entry point the calls, the time, its share, the bytes the calls must move at least (operands read once, results
written once; an accumulating backward-data reads its target too; the BatchNorm passes count z and dy once although they read them twice)
and the rate that makes.
--net FCN_pooling: the pooled twin (FCN_pooling(3, 3), csrc/resample.hip behind six of its transitions) through the same two paths, without
the single-layer part; the eval forward gets the per-entry table too, and every run starts with the box's float4 copy rate (cdnet_box_copy
over 256 MiB), the figure the resampling entries' GB/s stand beside.
One JSON line per measurement."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))


def events(f, reps, warmup):
    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in ev:
        e0.record()
        f()
        e1.record()
    torch.cuda.synchronize()
    return statistics.median(e0.elapsed_time(e1) for e0, e1 in ev)


def say(**kw):
    print(json.dumps(kw), flush=True)


def torch_forward(model, x):
    """the reference's forward (models/FullNet.py:134-138) through the model's containers"""
    out = model.conv1(x)
    for name, mod in model.blocks.named_children():
        if not name.startswith('block'):                    # a transition; FCN_pooling: also the pool / upsampling behind it
            out = mod(out)
            continue
        for layer in mod:
            y = out
            for c in layer.convs():
                y = c(y)
            out = torch.cat([out, y], 1)
    return model.conv2(out)


def torch_train_forward(model, x):
    """the reference's forward in train() (models/FullNet.py:25-52, :134-138): dropout on what a dense layer appends"""
    out = model.conv1(x)
    for name, mod in model.blocks.named_children():
        if not name.startswith('block'):                    # a transition; FCN_pooling: also the pool / upsampling behind it
            out = mod(out)
            continue
        for layer in mod:
            y = out
            for c in layer.convs():
                y = c(y)
            if layer.drop_rate > 0:
                y = F.dropout(y, p=layer.drop_rate, training=True)
            out = torch.cat([out, y], 1)
    return model.conv2(out)


def _must_bytes(name, args):
    """bytes a call has to move at least, from its arguments (None: not one of the network's kernels)"""
    if name == 'cdnet_maxpool2_forward':                      # (x, xs, y, ys, yoff, idx, is, N, H, W, C, f32, stream)
        n, h, w, c, f32 = args[7:12]
        es = 4 if f32 else 2
        return n * h * w * c * es + n * (h // 2) * (w // 2) * c * (es + (0 if getattr(args[5], 'value', args[5]) is None else 1))
    if name == 'cdnet_maxpool2_backward':                     # (dy, dys, dyoff, idx, is, dx, dxs, N, H, W, C, stream)
        n, h, w, c = args[7:11]
        return n * (h // 2) * (w // 2) * c * 5 + n * h * w * c * 4
    if name == 'cdnet_upsample4_bilinear_forward':            # (x, xs, y, ys, yoff, N, Hs, Ws, C, f32, stream)
        n, h, w, c, f32 = args[5:10]
        return n * h * w * c * 17 * (4 if f32 else 2)
    if name == 'cdnet_upsample4_bilinear_backward':           # (dy, dys, dyoff, dx, dxs, N, Hs, Ws, C, stream)
        n, h, w, c = args[5:9]
        return n * h * w * c * 17 * 4
    a = getattr(args[0], '_obj', None) if args else None
    if a is None:
        return None
    if name == 'cdnet_dilated_conv_forward':
        es = 4 if a.f32 else 2
        return a.N * a.H * a.W * (a.Cin * es + a.Cout * (4 if a.out_nchw else es)) + a.Cin * a.Cout * a.taps * es
    if name == 'cdnet_dilated_conv_backward_data':
        return a.N * a.H * a.W * (a.Cout + a.Cin * (2 if a.accumulate else 1)) * 4 + a.Cin * a.Cout * a.taps * 4
    if name == 'cdnet_dilated_conv_backward_weight':
        return a.N * a.H * a.W * (a.Cin + a.Cout) * 4 + a.Cin * a.Cout * a.taps * 4
    if name == 'cdnet_slice_bn_train_forward':
        return a.P * a.C * 2 * 4
    if name == 'cdnet_slice_bn_train_backward':
        return a.P * a.C * 3 * 4
    return None


def kernel_table(step, what='fullnet_train_kernels'):
    """one step with events around every library call: per entry point calls, time, share, must-move bytes and the rate"""
    from cdnet_amd import _lib
    rows, real = [], _lib.call

    def timed(name, *a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        real(name, *a)
        e1.record()
        rows.append((name, _must_bytes(name, a), e0, e1))
    _lib.call = timed
    try:
        step()
        torch.cuda.synchronize()
    finally:
        _lib.call = real
    total = sum(e0.elapsed_time(e1) for _, _, e0, e1 in rows)
    table = {}
    for name, must, e0, e1 in rows:
        t = table.setdefault(name, [0, 0.0, 0])
        t[0] += 1
        t[1] += e0.elapsed_time(e1)
        t[2] += must or 0
    for name, (calls, ms, must) in sorted(table.items(), key=lambda kv: -kv[1][1]):
        say(what=what, entry=name, calls=calls, ms=round(ms, 3), share=round(ms / total, 3),
            must_bytes=must or None, GBps=round(must / ms / 1e6, 1) if must else None)
    say(what=what, entry='all library calls', calls=len(rows), ms=round(total, 3))


def bench_box(reps=20):
    """the box's float4 copy rate (cdnet_box_copy, 256 MiB read + 256 MiB written per call)"""
    from cdnet_amd import _lib
    n = 256 << 20
    src, dst = torch.zeros(n, dtype=torch.uint8, device='cuda'), torch.empty(n, dtype=torch.uint8, device='cuda')
    st = _lib.stream_ptr()
    ms = events(lambda: _lib.call('cdnet_box_copy', _lib.ptr(src), _lib.ptr(dst), n, st), reps, 3)
    say(what='box_copy', bytes_moved=2 * n, ms=round(ms, 4), GBps=round(2 * n / ms / 1e6, 1))


def network_class(args):
    from cdnet_amd.models import FullNet as fn
    return getattr(fn, args.net)


def bench_train(args):
    import cdnet_amd
    import _fullnet_ref as fr
    import _fullnet_train_ref as tr
    from oracle import train as ot
    from cdnet_amd.trainer import FullNetTrainer
    FullNet = network_class(args)
    cdnet_amd.set_precision('fp32')
    B, S = args.batch, args.size
    x, label, weight = (v.cuda() for v in tr.batch((B, 3, S, S), 5))
    ours = FullNetTrainer(fr.randomize(FullNet(3, 3), 1).cuda(), seed=1)
    step_ours = lambda: ours.train_step(x, label, weight)
    step_torch = None
    if not args.skip_torch:
        m = fr.randomize(FullNet(3, 3), 1).cuda().train().to(memory_format=torch.channels_last)
        opt = torch.optim.Adam(m.parameters(), lr=1e-3, betas=(0.9, 0.99), weight_decay=1e-4)
        xt = x.contiguous(memory_format=torch.channels_last)

        def step_torch():
            opt.zero_grad(set_to_none=True)
            loss = ot.unet_losses(torch_train_forward(m, xt), label, weight)['total']
            loss.backward()
            opt.step()
    for _ in range(args.warmup):
        step_ours()
    torch.cuda.synchronize()
    say(what='fullnet_train_step', path='hip', note='alone, before the PyTorch path is warm', ms=round(events(step_ours, args.reps, 0), 3))
    kernel_table(step_ours)
    if step_torch:
        # the first PyTorch step builds MIOpen's kernels for ~150 (layer, direction) pairs: say where it is
        from cdnet_amd.models.FullNet import ConvLayer

        def progress(name):
            def hook(_mod, _inp, out):
                say(what='warmup', path='torch', forward=name)
                out.register_hook(lambda _g: say(what='warmup', path='torch', backward_reaches=name))
            return hook
        hooks = [mod.register_forward_hook(progress(name)) for name, mod in m.named_modules() if isinstance(mod, ConvLayer)]
        step_torch()
        torch.cuda.synchronize()
        for h in hooks:
            h.remove()
        for _ in range(1, args.warmup):
            step_torch()
        torch.cuda.synchronize()
    times = {'hip': [], 'torch': []}
    for _ in range(args.reps):                       # alternating: both paths see the same clocks and the same neighbours
        for path, f in (('hip', step_ours), ('torch', step_torch)):
            if f is None:
                continue
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            times[path].append(e0.elapsed_time(e1))
    med = {k: statistics.median(v) for k, v in times.items() if v}
    for k, v in med.items():
        say(what='fullnet_train_step', path=k, net=args.net, precision='fp32', batch=B, size=S, ms=round(v, 3), tiles_per_s=round(B / v * 1e3, 1),
            runs=[round(t, 2) for t in times[k]])
    if 'torch' in med:
        say(what='fullnet_train_step', hip_over_torch_time=round(med['hip'] / med['torch'], 3))


def bench_network(args):
    import cdnet_amd
    import _fullnet_ref as fr
    from cdnet_amd import runtime
    FullNet = network_class(args)
    N, S = args.windows, args.size
    model = fr.randomize(FullNet(3, 3), 1).cuda().eval()
    x = fr.bf16_exact_input((N, 3, S, S), 2).cuda()
    outs = {}
    for prec in ('bf16', 'fp32'):
        cdnet_amd.set_precision(prec)
        x16 = runtime.input_pack(x)
        with torch.no_grad():
            ms = events(lambda: model.forward_packed(x16), args.reps, args.warmup)
            outs[prec] = model.forward_packed(x16)[0][:2].clone()
            if args.net != 'FullNet':
                kernel_table(lambda: model.forward_packed(x16), what='fullnet_forward_kernels_' + prec)
        say(what='fullnet_forward', path='hip', net=args.net, precision=prec, windows=N, size=S, ms=round(ms, 3), ms_per_window=round(ms / N, 4))
        del x16
        torch.cuda.empty_cache()
    if args.skip_torch:
        return
    for prec, dt in (('bf16', torch.bfloat16), ('fp32', torch.float32)):
        m = fr.randomize(FullNet(3, 3), 1).cuda().eval().to(dt).to(memory_format=torch.channels_last)
        xt = x.to(dt).contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            ms = events(lambda: torch_forward(m, xt), args.reps, args.warmup)
            got = torch_forward(m, xt[:2]).float()
        err = float((got - outs[prec]).abs().max()) / float(got.abs().max())
        say(what='fullnet_forward', path='torch', net=args.net, precision=prec, windows=N, size=S, ms=round(ms, 3), ms_per_window=round(ms / N, 4),
            hip_vs_torch_rel_diff=err)
        del m, xt
        torch.cuda.empty_cache()


def bench_layers(args):
    import cdnet_amd
    from cdnet_amd import _lib
    N, S = args.windows, args.size
    lib = _lib.load()
    for prec, dt in (('bf16', torch.bfloat16), ('fp32', torch.float32)):
        f32 = prec == 'fp32'
        es = 4 if f32 else 2
        for name, Cin, Cout, taps, d, inplace in (('dense_168_24_d1', 168, 24, 9, 1, True), ('dense_168_24_d21', 168, 24, 9, 21, True),
                                                  ('trans_286_143', 286, 143, 1, 1, False)):
            g = torch.Generator().manual_seed(3)
            cs = (Cin + Cout + 7) // 8 * 8 if inplace else (Cin + 7) // 8 * 8
            buf = torch.randn((N, S, S, cs), generator=g).to(dt).cuda()
            w = (torch.randn((Cout, Cin, 3, 3) if taps == 9 else (Cout, Cin, 1, 1), generator=g) / (Cin * taps) ** 0.5).cuda()
            sc, sh = (0.5 + torch.rand(Cout, generator=g)).cuda(), torch.randn(Cout, generator=g).cuda()
            dst = buf if inplace else torch.empty((N, S, S, (Cout + 7) // 8 * 8), dtype=dt, device='cuda')
            wp = torch.empty(lib.cdnet_dilated_packed_weight_elems(Cin, Cout, taps, int(f32)), dtype=torch.bfloat16, device='cuda')
            _lib.call('cdnet_dilated_pack_weights', _lib.ptr(w), _lib.ptr(wp), Cin, Cout, taps, int(f32), _lib.stream_ptr())
            a = _lib.DilatedConvArgs()
            a.in_, a.w, a.out, a.scale, a.shift = buf.data_ptr(), wp.data_ptr(), dst.data_ptr(), sc.data_ptr(), sh.data_ptr()
            a.N, a.H, a.W, a.Cin, a.in_cstride, a.Cout, a.out_cstride, a.out_coff = N, S, S, Cin, cs, Cout, dst.shape[3], Cin if inplace else 0
            a.taps, a.dilation, a.leaky, a.slope, a.f32, a.out_nchw = taps, d, 1, 0.01, int(f32), 0
            st = _lib.stream_ptr()
            ms = events(lambda: _lib.call('cdnet_dilated_conv_forward', C.byref(a), st), args.layer_reps, 3)
            must = N * S * S * (Cin + Cout) * es + w.numel() * es
            flops = 2.0 * N * S * S * Cin * Cout * taps
            say(what='layer', layer=name, path='hip', precision=prec, ms=round(ms, 4), must_bytes=must, GBps=round(must / ms / 1e6, 1),
                TFLOPs=round(flops / ms / 1e9, 2))
            if not args.skip_torch:
                xt = buf[..., :Cin].permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last)
                wt = w.to(dt).contiguous(memory_format=torch.channels_last)
                sct, sht = sc.to(dt).view(1, -1, 1, 1), sh.to(dt).view(1, -1, 1, 1)

                def ref():
                    y = F.conv2d(xt, wt, padding=d if taps == 9 else 0, dilation=d if taps == 9 else 1)
                    return F.leaky_relu(y, 0.01) * sct + sht
                with torch.no_grad():
                    ms_t = events(ref, args.layer_reps, 3)
                say(what='layer', layer=name, path='torch', precision=prec, ms=round(ms_t, 4), GBps=round(must / ms_t / 1e6, 1),
                    TFLOPs=round(flops / ms_t / 1e9, 2), note='no cat: the appended copy of the input is not in this figure')
                del xt, wt
            del buf, dst
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=64)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--layer-reps', type=int, default=20)
    ap.add_argument('--skip-torch', action='store_true')
    ap.add_argument('--only-layers', action='store_true')
    ap.add_argument('--train', action='store_true', help='time one training step instead (fp32 mode)')
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--net', choices=['FullNet', 'FCN_pooling'], default='FullNet')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/bench_fullnet.py needs the GPU: a time measured elsewhere says nothing about it')
    say(what='device', name=torch.cuda.get_device_name(0))
    if args.net != 'FullNet':
        bench_box()
    if args.train:
        bench_train(args)
        return
    if args.net == 'FullNet':
        bench_layers(args)
    if not args.only_layers:
        bench_network(args)


if __name__ == '__main__':
    main()
