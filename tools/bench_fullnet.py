"""FullNet inference (cdnet_amd/models/FullNet.py on csrc/dilated.hip) against the same network as plain PyTorch modules, one process, one GPU.

    python tools/bench_fullnet.py [--windows 64] [--size 256] [--reps 5] [--warmup 2] [--layer-reps 20] [--skip-torch] [--only-layers]

1. Eval forward of --windows windows of --size^2 through FullNet(3, 3).forward_packed, in both precision modes (device events, median).
2. The same network run through the model's own nn containers (Conv2d -> LeakyReLU -> BatchNorm2d, torch.cat), fp32 and bf16
   (channels_last): the only baseline there is.
3. Single layers on --windows windows: a dense layer 168 -> 24 at d = 1 and at d = 21 (appending in place into a 168-channel buffer), the
   286 -> 143 transition; ours against F.conv2d + leaky_relu + affine on channels_last tensors.  `must_bytes` is what the layer has to
   move at least: every input channel read once, every output channel written once, the weights once; `GBps` = must_bytes / time.
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
        if name.startswith('trans'):
            out = mod(out)
            continue
        for layer in mod:
            y = out
            for c in layer.convs():
                y = c(y)
            out = torch.cat([out, y], 1)
    return model.conv2(out)


def bench_network(args):
    import cdnet_amd
    import _fullnet_ref as fr
    from cdnet_amd import runtime
    from cdnet_amd.models.FullNet import FullNet
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
        say(what='fullnet_forward', path='hip', precision=prec, windows=N, size=S, ms=round(ms, 3), ms_per_window=round(ms / N, 4))
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
        say(what='fullnet_forward', path='torch', precision=prec, windows=N, size=S, ms=round(ms, 3), ms_per_window=round(ms / N, 4),
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
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/bench_fullnet.py needs the GPU: a time measured elsewhere says nothing about it')
    say(what='device', name=torch.cuda.get_device_name(0))
    bench_layers(args)
    if not args.only_layers:
        bench_network(args)


if __name__ == '__main__':
    main()
