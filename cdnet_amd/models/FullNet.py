"""`FullNet` - the dense dilated network of the reference (models/FullNet.py:90-138, Hui Qu), inference on the MI355X.

Same constructor, same module tree (so `state_dict()` has the reference's 301 keys and shapes at the defaults: conv1.conv.weight, conv1.bn.*,
blocks.block{i}.denselayer{j}.conv.conv.weight, blocks.trans{i}.conv.weight, ..., conv2.weight) and the same initialisation.  The nn modules
are parameter containers; the forward runs on cdnet_dilated_conv_forward (csrc/dilated.hip):

  * every ConvLayer (Conv2d -> LeakyReLU -> BatchNorm2d, :14-21) is one launch, the eval-mode BatchNorm as the scale / shift after the LeakyReLU;
  * a dense block lives in ONE NHWC buffer of in + n_layers * growth channels (stride rounded up to 8) in the reference's concatenated order,
    unpadded; every layer reads channels [0, Cin) and appends its growth_rate channels in place - torch.cat([x, out], 1) (:36, :52) is never a copy;
  * a transition reads the whole buffer and writes the base channels of the next block's buffer;
  * conv2 (no activation, no BatchNorm, no bias) stores the fp32 [N, K, H, W] logits directly (the entry's out_nchw store).

Training (fp32 precision mode, under a trainer's tape - cdnet_amd.trainer.FullNetTrainer): every ConvLayer is the same launch with the
LeakyReLU alone, its output z kept compact, then cdnet_slice_bn_train_forward (batch statistics, running statistics, the dense layers'
dropout) into the slice of the block buffer; backward mirrors the in-place append: a transition's backward-data stores the whole gradient
buffer of its block, the dense layers run in reverse order, each reading its own slice and accumulating into the channels in front of it
(cdnet_slice_bn_train_backward, cdnet_dilated_conv_backward_weight, cdnet_dilated_conv_backward_data).  Without a tape a forward in training
mode raises.

`FCN_pooling` (:141-193), a subclass, is the same network with a 2x2 max-pool behind trans1..trans4 and a 4x bilinear up-sampling behind trans5
and trans6 (csrc/resample.hip): the walks below carry a map size per block, which for FullNet is one size throughout.
"""
import ctypes as C
import math

import torch
import torch.nn as nn

from .. import _lib, runtime

LEAKY_SLOPE = 0.01                    # nn.LeakyReLU's default (:20)
WORKSPACE_BYTES = 4 << 30             # forward_packed runs sub-batches whose block buffers stay under this many bytes

# hybrid dilations of one dense block, by layers per block and the block's nominal dilation (the table of :67-76)
HYBRID_DILATIONS = {
    4: {1: (1, 1, 1, 1), 2: (1, 2, 3, 2), 4: (1, 2, 5, 9), 8: (3, 7, 10, 13), 16: (13, 15, 17, 19)},
    6: {1: (1, 1, 1, 1, 1, 1), 2: (1, 2, 3, 1, 2, 3), 4: (1, 2, 3, 5, 6, 7), 8: (2, 5, 7, 9, 11, 14), 16: (10, 13, 16, 17, 19, 21)},
}


def block_dilations(n_layers, schedule, is_hybrid):
    """per block the dilation of each of its layers (KeyError for a (n_layers, dilation) pair the hybrid table lacks, as in the reference)"""
    if is_hybrid:
        return [tuple(HYBRID_DILATIONS[n_layers][int(d)]) for d in schedule]
    return [(int(d),) * n_layers for d in schedule]


class ConvLayer(nn.Sequential):            # :14-21
    def __init__(self, in_channels, out_channels, kernel_size, padding=0, dilation=1):
        super().__init__()
        self.add_module('conv', nn.Conv2d(in_channels, out_channels, kernel_size=kernel_size, padding=padding, dilation=dilation, bias=False))
        self.add_module('relu', nn.LeakyReLU(inplace=True))
        self.add_module('bn', nn.BatchNorm2d(out_channels))


class BasicLayer(nn.Sequential):           # :25-36
    def __init__(self, in_channels, growth_rate, drop_rate, dilation=1):
        super().__init__()
        self.conv = ConvLayer(in_channels, growth_rate, 3, padding=dilation, dilation=dilation)
        self.drop_rate = drop_rate

    def convs(self):
        return [self.conv]


class BottleneckLayer(nn.Sequential):      # :39-52
    def __init__(self, in_channels, growth_rate, drop_rate, dilation=1):
        super().__init__()
        self.conv1 = ConvLayer(in_channels, 4 * growth_rate, 1)
        self.conv2 = ConvLayer(4 * growth_rate, growth_rate, 3, padding=dilation, dilation=dilation)
        self.drop_rate = drop_rate

    def convs(self):
        return [self.conv1, self.conv2]


class DenseBlock(nn.Sequential):           # :56-61
    def __init__(self, in_channels, growth_rate, drop_rate, layer_type, dilations):
        super().__init__()
        for i, d in enumerate(dilations):
            self.add_module('denselayer%d' % (i + 1), layer_type(in_channels + i * growth_rate, growth_rate, drop_rate, int(d)))


def _round8(c):
    return (c + 7) // 8 * 8


def _buf(x16, c, hw=None):
    """an NHWC buffer of c channels (stride rounded up to 8) for the windows x16 (hw: at another map size), in x16's precision"""
    shape = x16.shape[:3] if hw is None else (x16.shape[0],) + tuple(hw)
    return torch.empty(shape + (_round8(c),), dtype=x16.dtype, device=x16.device)


class _Conv:
    """one launch: the Conv2d, its optional BatchNorm, the packed weights and the folded scale / shift of the current precision"""

    def __init__(self, conv, bn, leaky):
        self.conv, self.bn, self.leaky = conv, bn, leaky
        self.Cout, self.Cin = conv.weight.shape[:2]
        self.taps = conv.kernel_size[0] * conv.kernel_size[1]
        self.dilation = int(conv.dilation[0])
        self.key = self.wp = self.scale = self.shift = None
        self.p_drop = 0.0                         # dropout behind this layer's BatchNorm (the last ConvLayer of a dense layer, training)
        self.needs_dx = True                      # False: the stem, whose input is the image
        self.wpb = self.wpb_key = self.mean = self.invstd = None

    def prepare(self, device, fold=True):
        """fold False (training): the pack alone, no eval-mode scale / shift"""
        f32 = runtime.PRECISION == 'fp32'
        ts = [self.conv.weight] + ([] if self.bn is None else [self.bn.weight, self.bn.bias, self.bn.running_mean, self.bn.running_var])
        # (the optimiser kernels and the training forward write parameters and running statistics through raw pointers: the epoch counts them)
        key = (f32, str(device), fold, runtime.WEIGHTS_EPOCH[0]) + tuple((t.data_ptr(), t._version) for t in ts)
        if key == self.key:
            return
        w = self.conv.weight.detach().to(device=device, dtype=torch.float32).contiguous()
        n = _lib.load().cdnet_dilated_packed_weight_elems(self.Cin, self.Cout, self.taps, int(f32))
        self.wp = torch.empty(n, dtype=torch.bfloat16, device=device)
        _lib.call('cdnet_dilated_pack_weights', _lib.ptr(w), _lib.ptr(self.wp), self.Cin, self.Cout, self.taps, int(f32), _lib.stream_ptr())
        self.scale = self.shift = None
        if self.bn is not None and fold:          # eval-mode BatchNorm: y = (x - mean) / sqrt(var + eps) * weight + bias
            bn = self.bn
            sc = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
            sh = bn.bias.detach().double() - bn.running_mean.detach().double() * sc
            self.scale, self.shift = sc.float().to(device).contiguous(), sh.float().to(device).contiguous()
        self.key = key

    def prepare_train(self, device):
        """the forward pack without the fold, the backward-data pack w'[ci][co][8 - tap] and the saved statistics' buffers"""
        self.prepare(device, fold=False)
        if self.needs_dx and self.wpb_key != self.key:
            w = self.conv.weight.detach()
            n = _lib.load().cdnet_dilated_packed_weight_elems(self.Cout, self.Cin, self.taps, 1)
            if self.wpb is None or self.wpb.numel() != n or self.wpb.device != w.device:
                self.wpb = torch.empty(n, dtype=torch.bfloat16, device=device)
            _lib.call('cdnet_dilated_pack_weights_bwd', _lib.ptr(w), _lib.ptr(self.wpb), self.Cin, self.Cout, self.taps, 1, _lib.stream_ptr())
            self.wpb_key = self.key
        if self.bn is not None and (self.mean is None or self.mean.device != self.conv.weight.device):
            self.mean = torch.empty(self.Cout, dtype=torch.float32, device=device)
            self.invstd = torch.empty(self.Cout, dtype=torch.float32, device=device)

    def bn_forward(self, z, dst, dst_stride, dst_coff, P, layer, key, ws):
        """z -> batch statistics (saved, running statistics updated) -> BatchNorm + this layer's dropout into dst's channel slice"""
        bn = self.bn
        a = _lib.SliceBnFwdArgs()
        a.z, a.out, a.gamma, a.beta = z.data_ptr(), dst.data_ptr(), bn.weight.data_ptr(), bn.bias.data_ptr()
        if bn.track_running_stats:
            a.running_mean, a.running_var = bn.running_mean.data_ptr(), bn.running_var.data_ptr()
        a.mean, a.invstd, a.ws, a.ws_floats = self.mean.data_ptr(), self.invstd.data_ptr(), ws.data_ptr(), ws.numel()
        a.P, a.C, a.z_cstride, a.out_cstride, a.out_coff = P, self.Cout, z.shape[3], dst_stride, dst_coff
        a.eps, a.momentum, a.p_drop, a.layer, a.key = bn.eps, bn.momentum, self.p_drop, layer, key
        _lib.call('cdnet_slice_bn_train_forward', C.byref(a), _lib.stream_ptr())

    def bn_backward(self, dy, dy_stride, dy_coff, z, g, g_stride, P, layer, key, ws):
        """gradient of the slice -> dgamma, dbeta (the parameters' views of the flat gradient buffer) and g, the gradient of the raw output"""
        bn = self.bn
        a = _lib.SliceBnBwdArgs()
        a.dy, a.z, a.mean, a.invstd, a.gamma = dy.data_ptr(), z.data_ptr(), self.mean.data_ptr(), self.invstd.data_ptr(), bn.weight.data_ptr()
        a.dgamma, a.dbeta, a.g, a.ws, a.ws_floats = bn.weight.grad.data_ptr(), bn.bias.grad.data_ptr(), g.data_ptr(), ws.data_ptr(), ws.numel()
        a.P, a.C, a.z_cstride, a.dy_cstride, a.dy_coff, a.g_cstride = P, self.Cout, z.shape[3], dy_stride, dy_coff, g_stride
        a.slope, a.p_drop, a.layer, a.key = LEAKY_SLOPE, self.p_drop, layer, key
        _lib.call('cdnet_slice_bn_train_backward', C.byref(a), _lib.stream_ptr())

    def weight_grad(self, x, x_stride, g, g_stride, N, H, W, ws):
        a = _lib.DilatedWgradArgs()
        a.x, a.g, a.dw, a.ws, a.ws_bytes = x.data_ptr(), g.data_ptr(), self.conv.weight.grad.data_ptr(), ws.data_ptr(), ws.numel() * 4
        a.N, a.H, a.W, a.Cin, a.x_cstride, a.Cout, a.g_cstride = N, H, W, self.Cin, x_stride, self.Cout, g_stride
        a.taps, a.dilation = self.taps, self.dilation
        _lib.call('cdnet_dilated_conv_backward_weight', C.byref(a), _lib.stream_ptr())

    def backward_data(self, g, g_stride, dx, dx_stride, N, H, W, accumulate):
        a = _lib.DilatedBwdDataArgs()
        a.g, a.w, a.dx = g.data_ptr(), self.wpb.data_ptr(), dx.data_ptr()
        a.N, a.H, a.W, a.Cout, a.g_cstride, a.Cin, a.dx_cstride, a.dx_coff = N, H, W, self.Cout, g_stride, self.Cin, dx_stride, 0
        a.taps, a.dilation, a.accumulate, a.f32 = self.taps, self.dilation, int(accumulate), 1
        _lib.call('cdnet_dilated_conv_backward_data', C.byref(a), _lib.stream_ptr())

    def run(self, src, src_stride, dst, dst_stride, dst_coff, N, H, W, nchw=False):
        a = _lib.DilatedConvArgs()
        a.in_, a.w, a.out = src.data_ptr(), self.wp.data_ptr(), dst.data_ptr()
        a.scale = None if self.scale is None else self.scale.data_ptr()
        a.shift = None if self.shift is None else self.shift.data_ptr()
        a.N, a.H, a.W = N, H, W
        a.Cin, a.in_cstride = self.Cin, src_stride
        a.Cout, a.out_cstride, a.out_coff = self.Cout, dst_stride, dst_coff
        a.taps, a.dilation = self.taps, self.dilation
        a.leaky, a.slope = int(self.leaky), LEAKY_SLOPE
        a.f32, a.out_nchw = int(runtime.PRECISION == 'fp32'), int(nchw)
        _lib.call('cdnet_dilated_conv_forward', C.byref(a), _lib.stream_ptr())


class FullNet(nn.Module):
    def __init__(self, color_channels, output_channels=2, n_layers=6, growth_rate=24, compress_ratio=0.5,
                 drop_rate=0.1, dilations=(1, 2, 4, 8, 16, 4, 1), is_hybrid=True, layer_type='basic'):
        super().__init__()
        layer = BasicLayer if layer_type == 'basic' else BottleneckLayer
        width = 24
        self.conv1 = ConvLayer(color_channels, width, 3, padding=1)
        self.blocks = nn.Sequential()
        for i, ds in enumerate(block_dilations(n_layers, dilations, is_hybrid)):
            self.blocks.add_module('block%d' % (i + 1), DenseBlock(width, growth_rate, drop_rate, layer, ds))
            total = width + n_layers * growth_rate
            width = int(math.floor(total * compress_ratio))
            self.blocks.add_module('trans%d' % (i + 1), ConvLayer(total, width, 1))
        self.conv2 = nn.Conv2d(width, output_channels, kernel_size=3, stride=1, padding=1, bias=False)
        for m in self.modules():                                               # :124-132
            if isinstance(m, nn.Conv2d):
                m.weight.data.normal_(0, math.sqrt(2. / (m.kernel_size[0] * m.kernel_size[1] * m.out_channels)))
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.data.fill_(1)
                m.bias.data.zero_()
        self.color_channels, self.output_channels = color_channels, output_channels
        self.n_blocks, self.growth_rate = len(dilations), growth_rate
        self._rt = None

    RESAMPLE = {}                              # block index -> what follows its transition, 'pool' or 'up' (FCN_pooling); FullNet: nothing

    def _map_sizes(self, H, W):
        """(h, w) of every block's buffer and, last, of conv2's input"""
        return [(H, W)] * (self.n_blocks + 1)

    @property
    def final_conv(self):
        """the classifier under the name pipeline.mask_channels asks a one-output network for (a property: no extra state_dict key)"""
        return self.conv2

    def _build_runtime(self):
        def cl(m):
            return _Conv(m.conv, m.bn, True)
        blocks = []
        for i in range(self.n_blocks):
            block = getattr(self.blocks, 'block%d' % (i + 1))
            blocks.append(([[cl(c) for c in layer.convs()] for layer in block], cl(getattr(self.blocks, 'trans%d' % (i + 1)))))
            for layer, convs in zip(block, blocks[-1][0]):
                convs[-1].p_drop = float(layer.drop_rate)              # :33-35, :49-51: dropout on the appended channels only
        self._rt = (cl(self.conv1), blocks, _Conv(self.conv2, None, False))
        self._rt[0].needs_dx = False

    def _convs(self):
        stem, blocks, final = self._rt
        return [stem] + [c for layers, trans in blocks for layer in layers for c in layer] + [trans for _, trans in blocks] + [final]

    def _channels_per_pixel(self):
        """channels of the two widest live buffers (a block and its successor) plus the bottleneck's intermediate"""
        stem, blocks, final = self._rt
        widths = [_round8(trans.Cin) for _, trans in blocks] + [_round8(final.Cin)]
        inter = max(_round8(layer[0].Cout) if len(layer) == 2 else 0 for layers, _ in blocks for layer in layers)
        return max(a + b for a, b in zip(widths, widths[1:])) + inter

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError('cdnet_amd.models.FullNet.FullNet runs on the MI355X only (no CPU fallback)')
        return self.forward_packed(runtime.input_pack(x.float()))[0]

    def forward_packed(self, x16):
        """forward on packed NHWC windows [N,H,W,16] (color_channels real channels; bf16, or fp32 in the fp32 precision mode).  Returns `(logits,)`
        with logits f32 [N,K,H,W].  The batch runs in sub-batches whose block buffers stay under WORKSPACE_BYTES; a window's result does not
        depend on the batch it ran in."""
        if self.training and runtime.TAPE is None:
            raise RuntimeError('FullNet is inference only outside a trainer: call model.eval() first (a training forward needs the tape of '
                               'cdnet_amd.trainer.FullNetTrainer)')
        if not x16.is_cuda:
            raise RuntimeError('cdnet_amd.models.FullNet.FullNet runs on the MI355X only (no CPU fallback)')
        assert x16.dim() == 4 and x16.shape[3] == 16 and x16.dtype == runtime.act_dtype() and x16.is_contiguous(), 'packed NHWC [N,H,W,16] windows'
        assert self.color_channels <= 16
        if self._rt is None:
            self._build_runtime()
        if self.training:
            return (self._train_forward(x16),)
        for c in self._convs():
            c.prepare(x16.device)
        N, H, W, _ = x16.shape
        out = torch.empty((N, self.output_channels, H, W), dtype=torch.float32, device=x16.device)
        per_window = self._channels_per_pixel() * H * W * x16.element_size()
        sub = max(1, min(N, WORKSPACE_BYTES // per_window))
        sub = -(-N // -(-N // sub))                                            # equal-sized sub-batches (64 windows: 32 + 32, not 56 + 8)
        for s in range(0, N, sub):
            self._forward_nhwc(x16[s:s + sub], out[s:s + sub])
        return (out,)

    def _walk(self, x16, out, step, rec=None):
        """the network once, for both modes: stem, the dense layers' in-place appends (a bottleneck through its intermediate), the
        transitions, conv2 into `out`.  step(c, src, src_stride, dst, dst_stride, dst_coff, hw) runs one ConvLayer on maps of hw = (h, w);
        rec, a TrainRecord, keeps the block buffers and the bottlenecks' intermediates.  A transition with a resampling step behind it
        (FCN_pooling) writes a compact temporary that _resample_forward resamples into the next block's base channels."""
        stem, blocks, final = self._rt
        N, H, W, _ = x16.shape
        sizes = self._map_sizes(H, W)
        cur = _buf(x16, blocks[0][1].Cin, sizes[0])
        step(stem, x16, 16, cur, cur.shape[3], 0, sizes[0])
        for i, (layers, trans) in enumerate(blocks):
            cs, hw = cur.shape[3], sizes[i]
            if rec is not None:
                rec.bufs.append(cur)
            for layer in layers:
                if len(layer) == 1:                                    # BasicLayer: append in place
                    step(layer[0], cur, cs, cur, cs, layer[0].Cin, hw)
                else:                                                  # BottleneckLayer: 1x1 to 4 * growth, then the dilated 3x3 appends
                    mid = _buf(x16, layer[0].Cout, hw)
                    step(layer[0], cur, cs, mid, mid.shape[3], 0, hw)
                    step(layer[1], mid, mid.shape[3], cur, cs, layer[0].Cin, hw)
                    if rec is not None:
                        rec.mids[id(layer[0])] = mid
            nxt = _buf(x16, blocks[i + 1][1].Cin if i + 1 < len(blocks) else final.Cin, sizes[i + 1])
            if i not in self.RESAMPLE:
                step(trans, cur, cs, nxt, nxt.shape[3], 0, hw)
            else:
                tmp = _buf(x16, trans.Cout, hw)
                step(trans, cur, cs, tmp, tmp.shape[3], 0, hw)
                self._resample_forward(i, tmp, nxt, trans.Cout, rec)
            cur = nxt
        if rec is not None:
            rec.bufs.append(cur)
        final.run(cur, cur.shape[3], out, 0, 0, N, H, W, nchw=True)

    def _forward_nhwc(self, x16, out):
        N = x16.shape[0]
        self._walk(x16, out, lambda c, src, ss, dst, ds, coff, hw: c.run(src, ss, dst, ds, coff, N, hw[0], hw[1]))

    # ------------------------------------------------------------------------------------------------
    # training (fp32 precision mode): forward with a record for backward, and the backward walk
    def _ws(self, name, need, device):
        """grow-only fp32 workspace of the training kernels"""
        wss = self.__dict__.setdefault('_train_ws', {})
        ws = wss.get(name)
        if ws is None or ws.numel() < need or ws.device != device:
            ws = wss[name] = torch.empty((max(need, 1),), dtype=torch.float32, device=device)
        return ws

    def _train_forward(self, x16):
        if runtime.PRECISION != 'fp32':
            raise NotImplementedError('FullNet trains in the fp32 precision mode only (runtime.set_precision("fp32"))')
        convs = self._convs()
        index = {id(c): k for k, c in enumerate(convs)}
        N, H, W, _ = x16.shape
        P, dev = N * H * W, x16.device
        lib = _lib.load()
        for c in convs:
            c.prepare_train(dev)
        ws = self._ws('bn', max(lib.cdnet_slice_bn_workspace_floats(P, c.Cout) for c in convs), dev)     # (P: the largest map's)
        rec = TrainRecord(x16, (N, H, W), int(getattr(self, '_train_key', 0)), index)

        def conv_bn(c, src, ss, dst, ds, coff, hw):
            h, w = hw
            z = _buf(x16, c.Cout, hw)
            c.run(src, ss, z, z.shape[3], 0, N, h, w)             # (prepare_train left no scale / shift: the LeakyReLU output)
            c.bn_forward(z, dst, ds, coff, N * h * w, index[id(c)], rec.key, ws)
            rec.z[id(c)] = z
            if c.p_drop > 0:
                rec.drops.append((index[id(c)], (N, h, w, c.Cout), c.p_drop))
        out = torch.empty((N, self.output_channels, H, W), dtype=torch.float32, device=dev)
        self._walk(x16, out, conv_bn, rec)
        runtime.TAPE.append(rec)
        return out

    def train_backward(self, rec, dlogits):
        """gradients of every parameter (into their views of the flat gradient buffer) from dlogits f32 [N,K,H,W]"""
        stem, blocks, final = self._rt
        N, H, W = rec.shape
        P, dev, key, index = N * H * W, dlogits.device, rec.key, rec.index
        lib = _lib.load()
        convs = self._convs()
        ws = self._ws('bn', max(lib.cdnet_slice_bn_workspace_floats(P, c.Cout) for c in convs), dev)
        sizes = self._map_sizes(H, W)
        wws = self._ws('wgrad', max(lib.cdnet_dilated_wgrad_workspace_bytes(N, h, w, c.Cin, c.Cout, c.taps)
                                    for h, w in set(sizes) for c in convs) // 4, dev)
        gmax = max(_round8(c.Cout) for c in convs)
        gflat = self._ws('g', P * gmax, dev)                      # g, the gradient of a raw convolution output: one compact scratch

        def bn_back(c, dy, dy_stride, dy_coff, hw=(H, W)):
            gs = _round8(c.Cout)
            c.bn_backward(dy, dy_stride, dy_coff, rec.z[id(c)], gflat, gs, N * hw[0] * hw[1], index[id(c)], key, ws)
            return gs
        dl = runtime.input_pack(dlogits)                          # [N,H,W,16] fp32
        last = rec.bufs[-1]
        final.weight_grad(last, last.shape[3], dl, 16, N, H, W, wws)
        dB = torch.empty_like(last)
        final.backward_data(dl, 16, dB, dB.shape[3], N, H, W, False)
        for i in reversed(range(len(blocks))):
            layers, trans = blocks[i]
            cur = rec.bufs[i]
            cs, hw = cur.shape[3], sizes[i]
            h, w = hw
            if i in self.RESAMPLE:                                 # the next block's base channels, resampled back to this map
                dB = self._resample_backward(i, dB, trans.Cout, rec)
            gs = bn_back(trans, dB, dB.shape[3], 0, hw)
            trans.weight_grad(cur, cs, gflat, gs, N, h, w, wws)
            dcur = torch.empty_like(cur)
            trans.backward_data(gflat, gs, dcur, cs, N, h, w, False)          # stores every channel of the block's gradient buffer
            for layer in reversed(layers):
                coff = layer[0].Cin
                gs = bn_back(layer[-1], dcur, cs, coff, hw)                  # this layer's slice is complete: the later layers ran
                if len(layer) == 1:
                    layer[0].weight_grad(cur, cs, gflat, gs, N, h, w, wws)
                    layer[0].backward_data(gflat, gs, dcur, cs, N, h, w, True)
                else:
                    mid = rec.mids[id(layer[0])]
                    ms = mid.shape[3]
                    layer[1].weight_grad(mid, ms, gflat, gs, N, h, w, wws)
                    dmid = torch.empty_like(mid)
                    layer[1].backward_data(gflat, gs, dmid, ms, N, h, w, False)
                    gs = bn_back(layer[0], dmid, ms, 0, hw)
                    layer[0].weight_grad(cur, cs, gflat, gs, N, h, w, wws)
                    layer[0].backward_data(gflat, gs, dcur, cs, N, h, w, True)
            dB = dcur
        gs = bn_back(stem, dB, dB.shape[3], 0)
        stem.weight_grad(rec.x16, 16, gflat, gs, N, H, W, wws)


class FCN_pooling(FullNet):
    """FullNet's pooled ablation twin (reference models/FullNet.py:141-193): the same seven dense blocks and transitions with
    nn.MaxPool2d(2, 2) behind trans1..trans4 and nn.UpsamplingBilinear2d(scale_factor=4) behind trans5 and trans6, so the blocks run on maps
    of H, H/2, H/4, H/8, H/16, H/4 and H rows.  The six resampling modules are parameter-free children of `blocks` in the reference's
    order; state_dict() is a seven-block FullNet's.  The resampling runs on csrc/resample.hip: a resampled transition writes a compact
    temporary, cdnet_maxpool2_forward / cdnet_upsample4_bilinear_forward resample it into the next block's base channels; backward reads the
    next block's gradient buffer as a slice (cdnet_maxpool2_backward with the stored arg-max bytes, cdnet_upsample4_bilinear_backward)."""
    RESAMPLE = {0: 'pool', 1: 'pool', 2: 'pool', 3: 'pool', 4: 'up', 5: 'up'}

    def __init__(self, color_channels, output_channels=2, n_layers=6, growth_rate=24, compress_ratio=0.5,
                 drop_rate=0.1, dilations=(1, 2, 4, 8, 16, 4, 1), is_hybrid=True, layer_type='basic'):
        dilations = tuple(dilations)
        if len(dilations) < 7:
            raise IndexError('FCN_pooling has seven dense blocks: %d dilations given' % len(dilations))      # (:162-163 dilation_list[i])
        super().__init__(color_channels, output_channels, n_layers, growth_rate, compress_ratio, drop_rate, dilations[:7], is_hybrid, layer_type)
        # the reference's children of `blocks`, in its order (:164-172); the parameters and their initial values are untouched
        children = list(self.blocks.named_children())
        self.blocks = nn.Sequential()
        for name, mod in children:
            self.blocks.add_module(name, mod)
            if name.startswith('trans'):
                i = int(name[5:])
                if i <= 4:
                    self.blocks.add_module('pool%d' % i, nn.MaxPool2d(kernel_size=2, stride=2))
                elif i <= 6:
                    self.blocks.add_module('upsample%d' % i, nn.UpsamplingBilinear2d(scale_factor=4))

    def _map_sizes(self, H, W):
        return [(H // d, W // d) for d in (1, 2, 4, 8, 16, 4, 1, 1)]

    def _channels_per_pixel(self):
        """FullNet's bound (taken at the full map size for every block) plus the widest transition's compact temporary"""
        return super()._channels_per_pixel() + max(_round8(trans.Cout) for _, trans in self._rt[1])

    def forward_packed(self, x16):
        if x16.dim() == 4 and (x16.shape[1] % 16 or x16.shape[2] % 16):
            raise ValueError('FCN_pooling needs H and W that are multiples of 16 (four 2x2 pools, then two 4x upsamplings): got %d x %d'
                             % (x16.shape[1], x16.shape[2]))
        return super().forward_packed(x16)

    def _resample_forward(self, i, tmp, nxt, C, rec):
        N, h, w, ts = tmp.shape
        f32 = int(tmp.dtype == torch.float32)
        if self.RESAMPLE[i] == 'pool':
            idx = None
            if rec is not None:
                idx = rec.pool_idx[i] = torch.empty((N, h // 2, w // 2, ts), dtype=torch.uint8, device=tmp.device)
            _lib.call('cdnet_maxpool2_forward', _lib.ptr(tmp), ts, _lib.ptr(nxt), nxt.shape[3], 0, _lib.ptr(idx), ts, N, h, w, C, f32,
                      _lib.stream_ptr())
        else:
            _lib.call('cdnet_upsample4_bilinear_forward', _lib.ptr(tmp), ts, _lib.ptr(nxt), nxt.shape[3], 0, N, h, w, C, f32, _lib.stream_ptr())

    def _resample_backward(self, i, dnxt, C, rec):
        """the gradient of block i's compact transition output from channels [0, C) of the next block's gradient buffer"""
        N, h, w, _ = rec.bufs[i].shape
        d = torch.empty((N, h, w, _round8(C)), dtype=torch.float32, device=dnxt.device)
        if self.RESAMPLE[i] == 'pool':
            idx = rec.pool_idx[i]
            _lib.call('cdnet_maxpool2_backward', _lib.ptr(dnxt), dnxt.shape[3], 0, _lib.ptr(idx), idx.shape[3], _lib.ptr(d), d.shape[3], N, h, w, C,
                      _lib.stream_ptr())
        else:
            _lib.call('cdnet_upsample4_bilinear_backward', _lib.ptr(dnxt), dnxt.shape[3], 0, _lib.ptr(d), d.shape[3], N, h, w, C, _lib.stream_ptr())
        return d


class TrainRecord:
    """what a training forward keeps for backward: the packed input, the block buffers, every z, the bottlenecks' intermediates"""

    def __init__(self, x16, shape, key, index):
        self.x16, self.shape, self.key, self.index = x16, shape, key, index
        self.bufs, self.z, self.mids = [], {}, {}
        self.pool_idx = {}                     # FCN_pooling: block index -> u8 [N,h/2,w/2,round8(C)], 2 dy + dx of every pooled element's arg-max
        self.drops = []                        # (layer index, [N,H,W,C], p) of every dropout applied: cdnet_dropout_mask regenerates its mask
