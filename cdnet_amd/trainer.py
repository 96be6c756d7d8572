"""Training step of the CDNet model on the HIP kernels: forward (batch-statistics BatchNorm), the five-term loss,
backward, gradient all-reduce over RCCL, optimiser step - the device-side replacement of the body of the reference's
train_util_dam.train (train_util_dam.py:54-311) with the host loops (:73-142, :278-289) moved onto the GPU.

This module is the tape walk.  No autograd: the forward leaves one record per convolution layer and fuse node it ran
(runtime.ConvRecord / FuseRecord); backward walks the tape in reverse and reads those records only.  For every layer it (1) turns the consumers' gradients into the gradient of the raw convolution output
(BatchNorm + residual + ReLU + max-pool/pad routing fused, cdnet_bn_backward), (2) computes dW on the matrix cores
(cdnet_conv_backward_weight, on a second stream, its split-K sums deferred and batched) and (3) computes the input gradient
as a forward convolution with a flipped/transposed weight pack (cdnet_conv_forward); it tells the all-reduce which
parameters' gradients are final, and re-packs the weights behind the optimiser step.

What the step works on lives elsewhere: the flat fp32 buffers the nn.Parameters are views into, the step of the six
optimisers over them and the optimiser entry of a checkpoint in cdnet_amd.optim (`Trainer(optimizer=)` selects the rule;
`Trainer` holds the hyperparameters), the bucketed gradient all-reduce in cdnet_amd.allreduce.
"""
import ctypes as C
import os

import torch

from . import _lib, engine, optim, runtime, streams
from ._lib import BnBwdArgs, GradIn, GradTerm             # noqa: F401 (the mirrors live in _lib; the names resolve here as before)
from .allreduce import BucketReducer, bucketed_allreduce
from .engine import Src
from .optim import HEAD_PARAMS, FlatState                    # noqa: F401 (HEAD_PARAMS: the tests import it from here)
from .synth import synthetic_batch


# workgroups of one weight-gradient launch while it runs beside the input-gradient chain (bf16 mode; see _wgrad_wgs):
# layers of up to 128 x 128 pixels / larger ones
_WGRAD_WGS_DEEP, _WGRAD_WGS_SHALLOW = 128, 160
_WGRAD_WGS_KQ = 128                        # wgrad_ws_kernel<1, 1> on 512 x 512 layers (HRNet's branch 1)
_WGRAD_WGS_F32 = 160                      # (128 / 160 / 256: 989 / 994 / 987 tiles/s, three runs each on one box)
_RU_1X1_SIDE = True      # residual units' 1x1 backward-data beside the chain (tests flip it: same gradients either way)
WGRAD_STREAM = True       # weight gradients on a second stream beside the input-gradient chain
HEAD_BWD_FUSE = True      # fp32 mode, rev1 head: head backward + its weight gradients in one launch, dF3 behind the unit's ReLU (same bits)
# ... and dF1 / dF2 never stored: the launch leaves the pixels' 16 coefficients, the sums passes of mask_feature.bn2 / direction_feature.bn2
# rebuild their element (cdnet_dam_head_backward_coef, cdnet_bn_bwd_args.hc_*; same bits, 0.9 GB less traffic).  CDNET_HEAD_COEF_SRC=0: off
HEAD_COEF_SRC = os.environ.get('CDNET_HEAD_COEF_SRC', '1') != '0'
_WGRAD_DEFER = 0x100                       # CDNET_WGRAD_DEFER_REDUCE (include/cdnet_hip.h)
_WGRAD_DEEP_HW = 16384


class _on_stream:
    """`with torch.cuda.stream(s)` without its bookkeeping (device checks, Stream objects: ~15 us per use, once per layer of the
    backward pass): make `s` current, restore the previous stream on exit"""
    __slots__ = ('s', 'prev')

    def __init__(self, s):
        self.s = s

    def __enter__(self):
        self.prev = torch.cuda.current_stream()
        torch.cuda.set_stream(self.s)

    def __exit__(self, *exc):
        torch.cuda.set_stream(self.prev)
        return False


class _G:
    """a gradient contribution for a stored tensor"""
    __slots__ = ('t', 'Hg', 'Wg', 'oy', 'ox', 'pooled', 'coff', 'cstride', 'event', 'masked', 'hc')

    def __init__(self, t, Hg, Wg, oy=0, ox=0, pooled=0, coff=0, cstride=0):
        self.t, self.Hg, self.Wg, self.oy, self.ox, self.pooled, self.coff, self.cstride = t, Hg, Wg, oy, ox, pooled, coff, cstride
        self.event = None                    # produced on another stream: the consumer's stream waits for this event first
        self.masked = False                  # t is already dz of a residual unit's bn2: the consumer's gradient behind the unit's ReLU
                                             # (cdnet_dam_head_backward_fused, _head_fusable)
        self.hc = None                       # t is None: a head-coefficient source (coefficient rows, head weight block, first weight
                                             # float, first column, terms) that the sums pass of a residual unit's bn2 rebuilds (_bn_args)


def _choose_ci_tiles(C_src, Cout):
    if Cout <= 32 and runtime.PRECISION != 'fp32':
        return 1            # 16-bit path: 32-input-channel blocks; with at most 32 output channels the library runs ONE 32 x 32 block per
                            # workgroup and splits the tile's rows over the consumer waves (wgrad_ws_kernel<1, 1>)
    best, best_cost = 2, None
    for ci_t in (2, 1, 4):
        CI, CO = ci_t * 32, (4 // ci_t) * 32
        cost = -(-C_src // CI) * CI * -(-Cout // CO) * CO
        if best_cost is None or cost < best_cost:
            best, best_cost = ci_t, cost
    return best


def _wgrad_wgs(beside, HW, Cout):
    """most workgroups of one weight-gradient launch over a layer of HW pixels; beside: it runs beside the input-gradient chain"""
    # beside the input-gradient chain the weight-gradient kernels take fewer workgroups than there are CUs: a full grid of
    # them holds every CU's LDS, and the chain's producer / consumer convolutions (one 157 KB workgroup per CU) then queue
    # behind it - measured 1 663 -> 1 745 / 1 730 -> 1 813 tiles/s (two boxes).  fp32 mode: 160 workgroups since the
    # end of round 3 (+0.7 %; with round 2's kernels the caps cost 1.7 %).
    if not beside:
        return 256                                      # (the first layer's weight gradient runs after the chain has ended: whole chip)
    if runtime.PRECISION == 'fp32':
        return _WGRAD_WGS_F32
    if Cout <= 32 and HW > 65536:
        return _WGRAD_WGS_KQ
    return _WGRAD_WGS_DEEP if HW <= _WGRAD_DEEP_HW or HW > 65536 else _WGRAD_WGS_SHALLOW    # (512 x 512 layers of HRNet: 128 again)


class Trainer:
    def __init__(self, model, lr=1e-3, weight_decay=1e-4, betas=(0.9, 0.99), eps=None, quirk_sample0=True,
                 world_size=1, bucket_mb=25, optimizer='adam', momentum=0.95):
        """optimizer: one of cdnet_amd.optim.OPTIMIZERS (utils.py:907-939, matched case-insensitively); momentum serves 'sgd' only;
        eps None = the rule's own default (1e-5 for Ranger, ranger.py:28; 1e-8 otherwise)"""
        self.model = model
        self._pack_jobs = None
        self._pack_prec = None
        self._ar = None
        self.optimizer = str(optimizer).lower()
        if self.optimizer not in optim.OPTIMIZERS:
            raise ValueError('Optimizer {} not available (one of {})'.format(optimizer, ', '.join(optim.OPTIMIZERS)))
        if eps is None:
            eps = optim.RANGER_EPS if self.optimizer == 'ranger' else 1e-8
        self.lr, self.wd, self.betas, self.eps, self.momentum = lr, weight_decay, betas, eps, momentum
        self.quirk = int(quirk_sample0)
        self.world = world_size
        self.bucket = int(float(bucket_mb) * (1 << 20) // 4)
        self.flat = FlatState(model, self.optimizer)
        # the frozen set (Unet.freeze_encoder), read once: parameters outside the stepped range; _backward_tape finds the layers whose
        # output no trainable parameter and no input upstream wants a gradient for, and the walk never reaches them
        frozen = set(self.flat.frozen)
        self._frozen_ids = frozenset(id(p) for n, p in model.named_parameters() if n in frozen)
        self._nograd = set()
        self.narrowed = {}                                 # layer -> output channels its backward-data launch stops at (None: the full launch stays)
        model._trainer_bound = True                        # (freeze_encoder from here on raises)
        model._head_flat = self.flat.P[:self.flat.n_head] if self.flat.n_head == 855 else None
        self.dev = self.flat.P.device
        self._bufs = {}
        self._wss = {}
        self.losses = torch.zeros((11,), dtype=torch.float32, device=self.dev)     # 6 loss values + 5 pixel metrics
        self.alpha = 0.0                                   # 1: + the instance variance term (train_util_dam.py:174-180), cdnet_variance_loss;
        #                                                    2: 2 x that term instead of the mask cross-entropy (:182-189)
        self.dice, self.weight_map = 1, 1                  # --dice 0|1|2, --weight-map 0|1: the `terms` word of the loss entries (utils.loss_terms)
        self.loss_var = torch.full((1,), -1.0, dtype=torch.float32, device=self.dev)       # -1 as long as the term is off (:192)
        self.boundary = 0                                  # 1 / 2 / 3: + BoundaryLoss / FocalLoss2d / RobustFocalLoss2d of the mask logits (:195-205)
        self.loss_boundary = torch.zeros((1,), dtype=torch.float32, device=self.dev)       # the term's value of the last step (0 while it is off)
        self.tape = []
        self._cat_cache = {}
        self._wstream, self._events = None, {}
        self.ar_stats = None                     # buckets of the last step's all-reduce: total / released before backward ended
        self._packb_pending = False
        self._packb_stream = True              # backward-data re-packs beside the next forward
        self._side_active = False
        self.head_fused = False                 # the last backward took cdnet_dam_head_backward_fused (_head_fusable)
        self.head_coef = False                  # ... in the form that stores coefficients instead of dF1 / dF2 (HEAD_COEF_SRC)
        # split-K sums of the weight gradients: deferred and batched (one cdnet_wgrad_reduce_batch launch per ~CDNET_WGRAD_REDUCE_MB of
        # slabs instead of one reduce behind every weight-gradient launch; every call keeps its own slab buffer - 1.4 GB for the UNet)
        # Memory: with the default every weight-gradient call keeps its own split-K slab buffer for the trainer's lifetime (`buf(('wslab', ...))`,
        # ~1.4 GB for the DAM-Unet at 16 tiles, more for HRNet at 512²; a batch-size change re-allocates the buffers of the new shapes and frees
        # the old ones); CDNET_WGRAD_REDUCE_MB=0 returns to one shared slab and a reduce behind every launch.
        self._rd_mb = float(os.environ.get('CDNET_WGRAD_REDUCE_MB', '300'))        # 0: the reduce inside every call (one shared slab)
        self._rd_pending, self._rd_params, self._rd_bytes, self._rd_tables = [], [], 0, {}
        self._forwards, self._bn_base = 0, 0                 # training forwards run here / counted in a loaded checkpoint
        if world_size > 1:
            self.sync_from_rank0()                           # replicas start identical whatever each rank's RNG / checkpoint did

    # ------------------------------------------------------------------------------------------------
    def sync_from_rank0(self, src=0):
        """Broadcast rank `src`'s parameters (the whole flat buffer incl. the never-used ones), Adam moments, step counter and
        every module buffer (BatchNorm running statistics) to all ranks - what nn.DataParallel's per-iteration replicate
        (train.py:185) guarantees in the reference.  Called at construction and after a checkpoint load; without it a rank whose
        RNG drifted or that loaded a different file would silently train a different replica."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return
        f = self.flat
        works = [dist.broadcast(t, src=src, async_op=True) for t in (f.P, f.M, f.V, f.S) if t is not None]
        meta = torch.tensor([float(f.step_count), float(self._bn_base + self._forwards)], dtype=torch.float64, device=self.dev)
        works.append(dist.broadcast(meta, src=src, async_op=True))
        bufs = [b for b in self.model.buffers() if b.is_floating_point()]
        if bufs:
            flatb = torch.cat([b.detach().reshape(-1).float() for b in bufs])
            dist.broadcast(flatb, src=src)
            off = 0
            with torch.no_grad():
                for b in bufs:
                    b.copy_(flatb[off:off + b.numel()].view(b.shape))
                    off += b.numel()
        for w in works:
            w.wait()
        f.step_count = int(meta[0].item())
        self._bn_base, self._forwards = int(meta[1].item()), 0
        self.refresh_parameters()

    def reduce_scalars(self, values):
        """mean over ranks of a small vector of logging scalars (the 11 values of train_util_dam.train): with nn.DataParallel the
        reference computes them on the gathered global batch; here every rank holds its shard's means"""
        import torch.distributed as dist
        if self.world <= 1 or not (dist.is_available() and dist.is_initialized()):
            return values
        t = torch.as_tensor(values, dtype=torch.float64).to(self.dev)
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        return (t / dist.get_world_size()).cpu().numpy()

    # ------------------------------------------------------------------------------------------------
    def buf(self, key, shape, dtype):
        b = self._bufs.get(key)
        if b is None or tuple(b.shape) != tuple(shape) or b.dtype != dtype:
            b = torch.empty(shape, dtype=dtype, device=self.dev)
            self._bufs[key] = b
        return b

    def _ws(self, name, need, side=False):
        """grow-only fp32 workspace `name` of at least `need` floats; side: the weight-gradient stream uses it too"""
        ws = self._wss.get(name)
        if ws is None or ws.numel() < need:
            if side and self._wstream is not None:
                self._wstream.synchronize()          # the old workspace may still be in use on the weight-gradient stream
            ws = self._wss[name] = torch.empty((need,), dtype=torch.float32, device=self.dev)
        return ws

    def grad_sum(self, gl, mask, npix, Cc, out):
        """out = [mask > 0] * sum of the gradient contributions `gl` (cdnet_grad_sum)"""
        assert 1 <= len(gl) <= 6
        arr = (GradTerm * len(gl))()
        for k, g in enumerate(gl):
            assert not g.pooled and g.oy == 0 and g.ox == 0
            arr[k].g, arr[k].cstride, arr[k].coff = g.t.data_ptr(), g.cstride or Cc, g.coff
        _lib.call(_lib.entry('cdnet_grad_sum', out.dtype == torch.float32), C.byref(arr), len(gl), None if mask is None else _lib.ptr(mask),
                  npix, Cc, _lib.ptr(out), _lib.stream_ptr())

    def take(self, grads, key):
        """pop the gradient contributions of a stored tensor for a consumer on the CURRENT stream: a contribution computed beside the chain
        (_RU_1X1_SIDE: the residual units' 1x1 backward-data on the weight-gradient stream) carries an event the consumer's stream must
        wait for first - wherever the list is consumed (a layer's BatchNorm backward, cat_grad, _fuse_backward)"""
        gl = grads.pop(key, None)
        if gl is not None:
            for g_ in gl:
                if g_.event is not None:
                    torch.cuda.current_stream().wait_event(g_.event)
                    g_.event = None
        return gl

    def cat_grad(self, o, grads):
        """gradient of a concatenation buffer (several consumers, several writers): summed once per backward"""
        key = id(o)
        if key not in self._cat_cache:
            gl = self.take(grads, key)
            if gl is None:
                d = None
            elif len(gl) == 1 and not gl[0].coff and gl[0].cstride in (0, o.shape[3]):
                d = gl[0].t
            else:
                d = self.buf(('dcat', key), o.shape, runtime.act_dtype())
                self.grad_sum(gl, None, o.shape[0] * o.shape[1] * o.shape[2], o.shape[3], d)
            self._cat_cache[key] = d
        return self._cat_cache[key]

    # ------------------------------------------------------------------------------------------------
    def forward(self, x):
        m = self.model
        m.train()
        self._forwards += 1
        runtime.TAPE = self.tape
        del self.tape[:]
        try:
            out = m(x)
        finally:
            runtime.TAPE = None
        return out

    def loss_and_grads(self, mask, point, direction, label, dirlab, point_t, weight):
        B, _, H, W = mask.shape
        lib = _lib.load()
        ND = direction.shape[1]                       # 5 / 9 / 17 direction classes (options.py:45)
        ws = self._ws('loss', lib.cdnet_dam_loss_classes_workspace_floats(B, H * W, ND))
        dmask = self.buf('dmask', mask.shape, torch.float32)
        dpoint = self.buf('dpoint', point.shape, torch.float32)
        ddir = self.buf('ddir', direction.shape, torch.float32)
        assert label.dtype == torch.uint8 and dirlab.dtype == torch.uint8 and weight.dtype == torch.uint8
        assert point_t.dtype == torch.float16
        if self.dice != 1:
            raise ValueError('dice = %r with a DAM model: the reference dies on an unbound loss_direction_dice (train_util_dam.py:297); only 1 works'
                             % (self.dice,))
        from .utils import loss_terms
        terms = loss_terms(self.dice, self.weight_map, self.alpha)
        args = (_lib.ptr(mask), _lib.ptr(point), _lib.ptr(direction), _lib.ptr(label.contiguous()),
                _lib.ptr(dirlab.contiguous()), _lib.ptr(point_t.contiguous()), _lib.ptr(weight.contiguous()), B, H, W, ND,
                self.quirk, _lib.ptr(ws), ws.numel(), _lib.ptr(self.losses), _lib.ptr(dmask),
                _lib.ptr(dpoint), _lib.ptr(ddir), _lib.stream_ptr())
        if terms == 7:                                 # every term: the entry of the default configuration
            _lib.call('cdnet_dam_loss_classes', *args)
        else:                                          # --weight-map 0 and / or --alpha 2
            _lib.call('cdnet_dam_loss_terms', *args, terms)
        if self.alpha:
            self._variance_term(mask, label, dmask)
        if self.boundary:
            self._boundary_term(mask, label, dmask)
        return dmask, dpoint, ddir

    def _variance_term(self, mask, label, dmask, total=None):
        """alpha = 1 or 2 (train_util_dam.py:174-189): loss_var of the mask logits into self.loss_var, alpha x it added to `total` (losses[0]
        unless given) and alpha x its gradient to dmask; dmask None: the value alone (total stays untouched)"""
        if self.alpha not in (1, 2):
            raise ValueError('alpha = %r: the variance term is built for alpha = 1 and 2 (0 switches it off)' % (self.alpha,))
        B, K, H, W = mask.shape
        need = _lib.load().cdnet_variance_loss_workspace_bytes(B, K, H, W)
        ws = self._ws('variance', (need + 3) // 4)
        total = self.losses[0:1] if total is None else total
        _lib.call('cdnet_variance_loss', _lib.ptr(mask), _lib.ptr(label.contiguous()), 1, B, K, H, W, float(self.alpha), _lib.ptr(ws),
                  ws.numel() * 4, _lib.ptr(self.loss_var), None if dmask is None else _lib.ptr(total), None if dmask is None else _lib.ptr(dmask),
                  None, None, _lib.stream_ptr())

    def _boundary_term(self, mask, label, dmask, total=None):
        """boundary_loss = 1 / 2 / 3 (train_util_dam.py:195-205, beta = 1): the term of the mask logits into self.loss_boundary, added to
        `total` (losses[0] unless given) and its gradient to dmask (cdnet_boundary_loss)"""
        if self.boundary not in (1, 2, 3):
            raise ValueError('boundary = %r: 1 (BoundaryLoss), 2 (FocalLoss2d) or 3 (RobustFocalLoss2d); 0 switches the term off' % (self.boundary,))
        B, K, H, W = mask.shape
        need = _lib.load().cdnet_boundary_loss_workspace_bytes(self.boundary, B, K, H, W)
        if need == 0:
            raise ValueError('the boundary term serves three-class mask logits, got %s' % (tuple(mask.shape),))
        ws = self._ws('boundary', (need + 3) // 4)
        total = self.losses[0:1] if total is None else total
        _lib.call('cdnet_boundary_loss', _lib.ptr(mask), _lib.ptr(label.contiguous()), self.boundary, B, K, H, W, 1.0, _lib.ptr(ws),
                  ws.numel() * 4, _lib.ptr(self.loss_boundary), _lib.ptr(total), _lib.ptr(dmask), _lib.stream_ptr())

    # ------------------------------------------------------------------------------------------------
    def backward(self, dmask, dpoint, ddir):
        m = self.model
        f1, f2, f3 = m._last_feats
        N, H, W, _ = f1.x.shape
        hf = [runtime.head_feat(f) for f in (f1, f2, f3)]
        dhead = self.flat.G[:self.flat.n_head]
        owner = self._head_fusable(f1, f2, f3)
        self.head_fused = owner is not None
        # (the rebuilt source needs the second BatchNorm pass on the stored dz: with the library's A/B switch CDNET_BN_DZ_REUSE=0 the tensors stay)
        self.head_coef = owner is not None and HEAD_COEF_SRC and os.environ.get('CDNET_BN_DZ_REUSE', '1').strip() not in ('0', '') \
            and self._head_coef_ok(f1) and self._head_coef_ok(f2)
        if self.head_coef:
            # the same launch without dF1 and dF2: 16 coefficients a pixel instead of 2 x 64 gradient values; each one's only reader, the
            # sums pass of its unit's bn2, rebuilds its element from them and the head's weight rows (wd at float 64, wm at 640 of the block)
            coef = self.buf('head_coef', (N, H, W, 16), torch.float32)
            dz3 = self.buf('dF2', (N, H, W, 64), torch.float32)
            hw = m.head_weight_block()
            ws = self._ws('head', _lib.load().cdnet_dam_head_backward_fused_workspace_floats())
            _lib.call('cdnet_dam_head_backward_coef', C.byref(hf[0]), C.byref(hf[1]), C.byref(hf[2]), _lib.ptr(hw), _lib.ptr(dmask),
                      _lib.ptr(dpoint), _lib.ptr(ddir), N, H, W, _lib.ptr(coef), _lib.ptr(dz3), _lib.ptr(ws), ws.numel(), _lib.ptr(dhead),
                      _lib.stream_ptr())
            heads = [(f1.x, _G(None, H, W)), (f2.x, _G(None, H, W)), (f3.x, _G(dz3, H, W))]
            heads[0][1].hc = (coef, hw, 640, 10, 3)
            heads[1][1].hc = (coef, hw, 64, 1, 9)
            heads[2][1].masked = True
            self._run_tape(heads, None)
            return
        df = [self.buf('dF%d' % k, (N, H, W, 64), runtime.act_dtype()) for k in range(3)]
        if owner is not None:
            # one launch instead of two (every feature read once, no coefficient tensor), bit-identical to them; dF3 leaves as dz3, behind
            # the unit's ReLU - the tape walk runs point_feature.bn2's backward on it without the mask (_bn_backward_masked)
            ws = self._ws('head', _lib.load().cdnet_dam_head_backward_fused_workspace_floats())
            _lib.call('cdnet_dam_head_backward_fused', C.byref(hf[0]), C.byref(hf[1]), C.byref(hf[2]), _lib.ptr(m.head_weight_block()),
                      _lib.ptr(dmask), _lib.ptr(dpoint), _lib.ptr(ddir), N, H, W, _lib.ptr(df[0]), _lib.ptr(df[1]), _lib.ptr(df[2]),
                      _lib.ptr(ws), ws.numel(), _lib.ptr(dhead), _lib.stream_ptr())
            heads = [(f.x, _G(d, H, W)) for f, d in zip((f1, f2, f3), df)]
            heads[2][1].masked = True
            self._run_tape(heads, None)
            return
        ws = self._ws('head', _lib.load().cdnet_dam_head_backward_workspace_floats(N, H, W))
        _lib.call('cdnet_dam_head_backward', C.byref(hf[0]), C.byref(hf[1]), C.byref(hf[2]), _lib.ptr(m.head_weight_block()),
                  _lib.ptr(dmask), _lib.ptr(dpoint), _lib.ptr(ddir), N, H, W, _lib.ptr(df[0]), _lib.ptr(df[1]),
                  _lib.ptr(df[2]), _lib.ptr(ws), ws.numel(), _lib.ptr(dhead), _lib.stream_ptr())
        self._run_tape([((f.grad_to or (f.x,))[0], _G(d, H, W)) for f, d in zip((f1, f2, f3), df)], None)

    def _head_coef_ok(self, f):
        """the head's gradient of feature f may stay a head-coefficient source: f.x is the stored output of a residual unit with the fused
        epilogue, so the consumers' gradients go unsummed to the unit's bn2 (the flat fp32 residual form, mask from f.x, dz stored) - at
        most two more of them, same size, and no fuse node that would sum them first"""
        readers = 0
        for Rt in self.tape:
            if isinstance(Rt, runtime.FuseRecord):
                if any(t.x is f.x for t in Rt.terms):
                    return False
                continue
            for sx in Rt.srcs:
                if sx.res is f.x or (sx.x is f.x and (sx.pool or tuple(sx.off) != (0, 0))):
                    return False
                readers += sx.x is f.x
        P = next((Rt for Rt in self.tape if not isinstance(Rt, runtime.FuseRecord) and Rt.out is f.x), None)
        owner = None if P is None or P.layer.kind != 'conv1' else P.fused_res_of
        return readers <= 2 and owner is not None and owner.layer.bn is not None and owner.relu == 2 and owner.res is f.x \
            and owner.out.dtype == torch.float32 and tuple(owner.out.shape) == tuple(f.x.shape)

    def _head_fusable(self, f1, f2, f3):
        """cdnet_dam_head_backward_fused's one case: fp32 mode, the rev1 head over three plain stored fp32 features, the third one the
        output of a residual unit with the fused epilogue (BatchNorm + mask from the stored output) that nothing on the tape reads.
        Returns the record of that unit's conv2 or None"""
        if not HEAD_BWD_FUSE or runtime.PRECISION != 'fp32' or getattr(self.model, 'VARIANT', None) != 'rev1':
            return None
        for f in (f1, f2, f3):
            if f.x.dtype != torch.float32 or f.scale is not None or f.shift is not None or f.res is not None or f.relu or f.pool \
                    or f.grad_to is not None or tuple(f.off) != (0, 0) or f.C != 64:
                return None
        owner = None
        for Rt in self.tape:
            if isinstance(Rt, runtime.FuseRecord):
                if any(t.x is f3.x for t in Rt.terms):
                    return None
                continue
            if any(sx.x is f3.x or sx.res is f3.x for sx in Rt.srcs):
                return None
            if Rt.out is f3.x:
                owner = Rt.fused_res_of if Rt.layer.kind == 'conv1' else None
        if owner is None or owner.layer.bn is None or owner.relu != 2 or owner.res is not f3.x \
                or owner.out.dtype != torch.float32 or tuple(owner.out.shape) != tuple(f3.x.shape):
            return None
        return owner

    def _classifier_backward(self, key, f, conv, dl):
        """backward of a plain 1x1 classifier `conv` on the 64-channel feature `f` (cdnet_final_conv1x1_backward): fills the gradients of
        its weight and bias; returns the gradient of the feature as a _G"""
        N, H, W, _ = f.x.shape
        K = conv.out_channels
        df = self.buf(key, (N, H, W, 64), runtime.act_dtype())
        ws = self._ws('slab', _lib.load().cdnet_final_conv1x1_backward_workspace_floats(), side=True)
        hf = runtime.head_feat(f)
        w = conv.weight.detach().reshape(K, 64)
        _lib.call('cdnet_final_conv1x1_backward', C.byref(hf), _lib.ptr(w), _lib.ptr(dl), K, N, H, W, _lib.ptr(df), _lib.ptr(ws),
                  ws.numel(), _lib.ptr(conv.weight.grad), _lib.ptr(conv.bias.grad), _lib.stream_ptr())
        return _G(df, H, W)

    def _run_tape(self, heads, params):
        """the rest of backward from the head gradients `heads` [(stored tensor, _G)]; `params`: the head's parameters, whose gradients
        are final by now (None: the head block of the flat buffer)"""
        grads = {}                      # id(stored tensor) -> [_G]

        def add(t, g):
            grads.setdefault(id(t), []).append(g)
        for t, g in heads:
            add(t, g)
        self._overlap_begin()
        self._overlap_done(params)
        self._backward_tape(grads, add)

    def _backward_tape(self, grads, add):
        """walk the forward tape backwards: BatchNorm(+ReLU, residual, pool/pad/concat routing) backward, then the
        weight and input gradients of every convolution that received a gradient"""
        self._cat_cache = {}
        # (a backward that raised midway - CDNET_REQUIRE failure, OOM - must not leave its deferred split-K descriptors to this one)
        self._rd_pending, self._rd_params, self._rd_bytes = [], [], 0
        if len(self._rd_tables) > 16:
            self._rd_tables.clear()                 # (one small device table per distinct call sequence: batch-size changes add entries)
        # who reads what: a BatchNorm layer whose raw output has exactly one reader - a 3x3 convolution - gets the first pass of its
        # backward (the channel sums) from that reader's backward-data launch (_input_backward), see _stats_fusable
        self._readers, self._producer, self._bn_partials = {}, {}, {}
        self._tape_pos = {Rt: k for k, Rt in enumerate(self.tape)}
        for Rt in self.tape:
            if isinstance(Rt, runtime.FuseRecord):
                for t in Rt.terms:                   # (counted too: _fuse_backward hands a residual sum's BatchNorm term its gradients unsummed
                    self._readers[id(t.x)] = self._readers.get(id(t.x), 0) + 1       # only when nothing else reads that term)
                continue
            for sx in Rt.srcs:
                self._readers[id(sx.x)] = self._readers.get(id(sx.x), 0) + 1
                if sx.res is not None:
                    self._readers[id(sx.res)] = self._readers.get(id(sx.res), 0) + 1
            self._producer[id(Rt.out)] = Rt
        self._nograd = self._no_grad_outputs()
        side = self._side_stream()
        self._side_active = side is not None
        if self._packb_pending:
            torch.cuda.current_stream().wait_event(self._event('packb'))      # backward-data packs made beside the forward
            self._packb_pending = False
        for k, R in enumerate(reversed(self.tape)):
            if isinstance(R, runtime.FuseRecord):
                self._fuse_backward(R, grads, add)
                continue
            gl = self.take(grads, id(R.out))
            if gl is None:
                continue
            owner = R.fused_res_of
            if owner is not None:
                # ResidualUnit.conv_1x1 with the fused residual epilogue: its stored output is the unit's output f.  The consumers'
                # gradients of f first pass bn2 + ReLU of the other branch (mask read from f); that dz is this layer's gradient.
                grads.setdefault(id(owner.out), []).extend(gl)
                owner.deferred = R
                continue
            self._layer_backward(k, R, gl, grads, add, side)
            d = R.deferred
            if d is not None:
                R.deferred = None
                self._layer_backward(('deferred', k), d, self.take(grads, id(d.out)), grads, add, side)
        if side is not None:
            with _on_stream(side):
                self._flush_reduces()
            ev = self._event(-1)
            ev.record(side)
            torch.cuda.current_stream().wait_event(ev)
        else:
            self._flush_reduces()

    def _no_grad_outputs(self):
        """ids of the stored outputs nothing upstream of which wants a gradient - autograd's rule for requires_grad = False: the layer's own
        parameters are all frozen and every source is the network's input or such an output itself (a frozen encoder: all of its layers).
        Their readers' backward-data launches leave those sources out (_input_backward), so no gradient ever arrives and the walk issues
        no BatchNorm-backward, weight-gradient, backward-data, pool-routing or pack launch for them"""
        dead = set()
        if not self._frozen_ids:
            return dead
        fr = self._frozen_ids
        for Rt in self.tape:
            if isinstance(Rt, runtime.FuseRecord):
                continue
            L = Rt.layer
            ps = (L.weight, L.bias, None if L.bn is None else L.bn.weight, None if L.bn is None else L.bn.bias)
            if all(p is None or id(p) in fr for p in ps) and \
                    all(sx.res is None and (sx.is_input or id((sx.grad_to or (sx.x,))[0]) in dead) for sx in Rt.srcs):
                dead.add(id(Rt.out))
        return dead

    def _fuse_backward(self, R, grads, add):
        """a fuse node: gradient of the (slice of the) output -> one contribution per term"""
        terms, o, relu, H, W, Cc, coff, name = R.terms, R.out, R.relu, R.H, R.W, R.C, R.coff, R.node.name
        sliced = o.shape[3] != Cc
        if sliced:
            d, dcs, dco = self.cat_grad(o, grads), o.shape[3], coff      # the whole concatenation's gradient, summed once
            if d is None:
                return
        else:
            gl = self.take(grads, id(o))
            if gl is None:
                return
            if relu and self._residual_tail(grads, gl, terms, o, H, W, Cc):
                return
            if relu or len(gl) > 1 or gl[0].coff or gl[0].cstride not in (0, Cc):
                d = self.buf(('dfuse', name), o.shape, o.dtype)
                self.grad_sum(gl, o if relu else None, o.shape[0] * H * W, Cc, d)
            else:
                d = gl[0].t
            dcs, dco = 0, 0
        N = o.shape[0]
        for k, t in enumerate(terms):
            if t.Hs == H and t.Ws == W:
                add(t.x, _G(d, H, W, coff=dco, cstride=dcs))
            else:
                din = self.buf(('dup', name, k), (N, t.Hs, t.Ws, Cc), d.dtype)
                _lib.call(_lib.entry('cdnet_upsample_bilinear_backward', d.dtype == torch.float32), _lib.ptr(d),
                          N, H, W, Cc, dcs, dco, t.Hs, t.Ws, _lib.ptr(din), _lib.stream_ptr())
                add(t.x, _G(din, t.Hs, t.Ws))

    def _residual_tail(self, grads, gl, terms, o, H, W, Cc):
        """relu(bn(y) + x) with x stored and y read by this node alone (BasicBlock / Bottleneck tails, seg_hrnet_rev1.py:76-92, :113-133): the
        masked sum of the consumers' gradients is the first thing y's BatchNorm backward computes anyway (the kernels' residual form: mask read
        from the stored output, dz stored for the other branch - what the DAM head's residual units use), so the separate grad_sum pass - one
        more read and write of the tensor - is skipped and the gradient list goes to y's layer as it is.  Returns False when the shape is not that."""
        if runtime.DEBUG_NORELU:
            return False
        if len(terms) == 1:
            # relu(bn(y)) stored for a stride-2 reader (`_plain`, the down-sampling chains): y's BatchNorm backward takes the ReLU mask from its
            # own forward values - no masked sum at all
            y = terms[0]
            P = self._producer.get(id(y.x)) if y.scale is not None else None
            if P is None or P.layer.bn is None or P.res is not None or self._readers.get(id(y.x), 0) != 1 or id(y.x) in grads \
                    or tuple(y.x.shape) != tuple(o.shape) or P.fused_res_of is not None or (y.Hs, y.Ws) != (H, W):
                return False
            P.relu, P.res = True, None
            grads[id(y.x)] = gl
            return True
        if len(terms) != 2 or len(gl) > 3:
            return False
        bn_t = [t for t in terms if t.scale is not None]
        if not bn_t or any((t.Hs, t.Ws) != (H, W) for t in terms):
            return False
        # (two BatchNorm terms - a Bottleneck with its downsample branch: the one whose layer comes first in backward takes the list, the other
        #  one reads the dz that pass stores)
        y = max(bn_t, key=lambda t: self._tape_pos.get(self._producer.get(id(t.x)), -1))
        x = terms[1] if terms[0] is y else terms[0]
        P = self._producer.get(id(y.x))
        if P is None or P.layer.bn is None or P.res is not None or self._readers.get(id(y.x), 0) != 1 or id(y.x) in grads \
                or tuple(y.x.shape) != tuple(o.shape) or P.fused_res_of is not None:
            return False
        if any(g.pooled or g.oy or g.ox or (g.Hg, g.Wg) != (H, W) for g in gl):
            return False
        P.relu, P.res, P.res_grad_to = 2, o, x.x
        grads[id(y.x)] = gl
        return True

    def _weights_done(self, params):
        """the weight-gradient launches of a layer are queued (current stream = the one they run on): sum their slabs now or later, then
        hand the layer's parameters to the all-reduce"""
        if not self._rd_pending:
            self._overlap_done(params)
            return
        self._rd_params.append(params)
        if self._rd_bytes >= self._rd_mb * (1 << 20):
            self._flush_reduces()

    def _flush_reduces(self):
        """one cdnet_wgrad_reduce_batch launch over every deferred weight gradient (bit-identical to the per-call reduction).  The
        descriptor table of a launch is built once per distinct sequence of calls and kept on the device."""
        if self._rd_pending:
            key = tuple(self._rd_pending)
            tab = self._rd_tables.get(key)
            if tab is None:
                lib = _lib.load()
                descs = (_lib.WgradReduceDesc * len(key))()
                b0 = 0
                for i, a in enumerate(key):
                    _lib.call('cdnet_wgrad_reduce_desc_fill', *a, b0, C.byref(descs[i]))
                    b0 += descs[i].blocks
                dev_tab = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(self.dev)
                tab = self._rd_tables[key] = (dev_tab, len(key), b0)
            _lib.call('cdnet_wgrad_reduce_batch', _lib.ptr(tab[0]), tab[1], tab[2], _lib.stream_ptr())
        for params in self._rd_params:
            self._overlap_done(params)
        self._rd_pending, self._rd_params, self._rd_bytes = [], [], 0

    def _layer_backward(self, k, R, gl, grads, add, side):
        """one convolution layer: BatchNorm / residual / ReLU backward of its output, weight gradient (side stream), input gradient.
        `gl` comes from take() on this stream: the events of contributions computed beside the chain are already waited for"""
        L, srcs, out, Hl, Wl = R.layer, R.srcs, R.out, R.H, R.W
        No, Ho, Wo, Co = out.shape
        params = (L.weight, L.bias, None if L.bn is None else L.bn.weight, None if L.bn is None else L.bn.bias)
        part = self._bn_partials.pop(id(out), None)
        if len(gl) == 1 and gl[0].masked:
            g = self._bn_backward_masked(R, out, gl[0], add)
        elif part is not None:
            # the reader's backward-data launch left the channel sums: finalize + second pass only
            assert len(gl) == 1, (L.name, len(gl))
            a, ktab = self._bn_backward_stats(L, out, gl[0], partial=part)
            g = self.buf(('draw', L.name), (No, Ho, Wo, Co), runtime.act_dtype())
            _lib.call('cdnet_bn_backward_apply', C.byref(a), _lib.ptr(ktab), _lib.ptr(g), _lib.stream_ptr())
        elif L.bn is not None or len(gl) > 1 or gl[0].pooled or gl[0].coff or (gl[0].cstride not in (0, Co)):
            g = self._bn_backward(R, out, gl, add)
        else:
            g = gl[0].t                                     # plain pass-through (conv_1x1 residual branch)
        if side is None:
            self._weight_backward(L, srcs, g, Hl, Wl)
            self._weights_done(params)
            self._input_backward(L, srcs, g, Hl, Wl, add)
        else:
            # the weight gradient only feeds the optimiser: it runs on a second stream beside the input-gradient chain.  The chain's
            # next kernel is issued first (under rocprofv3, whose interception slows every launch call, the chain otherwise sits idle
            # in the 512-channel layers while the host is still issuing the side stream's launches; without the profiler the host
            # keeps its lead either way)
            ev = self._event(k)
            ev.record()             # (recorded after backward-data instead, the weight gradient overlaps the HBM-bound BatchNorm passes of
            beside = _RU_1X1_SIDE and L.kind == 'conv1' and isinstance(k, tuple) and L.needs_input_grad
            if not beside:
                self._input_backward(L, srcs, g, Hl, Wl, add)      # the next layer rather than the convolution: -2 %)
            side.wait_event(ev)
            with _on_stream(side):
                if beside:
                    # the 1x1 branch of a residual unit: its input gradient is first needed by the BatchNorm backward of the PREVIOUS unit,
                    # three convolutions down the chain - it runs beside the chain, in front of the weight gradients queued from here on
                    ev2 = self._event(('beside', k))

                    def add_beside(tgt, g_):
                        g_.event = ev2
                        add(tgt, g_)
                    self._input_backward(L, srcs, g, Hl, Wl, add_beside)
                    ev2.record()
                self._weight_backward(L, srcs, g, Hl, Wl)
                self._weights_done(params)         # (a bucket released here is ordered after both streams' work so far)

    def _bn_backward_stats(self, L, out, g, partial):
        """finalize pass over the partial channel sums a backward-data launch left (cdnet_conv_args.ws = 2, fp32 mode): dgamma, dbeta and
        the [7][C] table the second pass reads"""
        a = self._bn_args(L, out, [_G(g.t, g.Hg, g.Wg)], res=None, relu=1)          # (one plain source, BatchNorm + ReLU, no residual)
        ktab = self.buf(('ktab', L.name), (7, out.shape[3]), torch.float32)
        bn = L.bn
        _lib.call('cdnet_bn_backward_finalize', C.byref(a), _lib.ptr(bn.weight.detach()), _lib.ptr(bn.weight.grad), _lib.ptr(bn.bias.grad),
                  _lib.ptr(partial), partial.shape[0], _lib.ptr(ktab), _lib.stream_ptr())
        return a, ktab

    def _bn_backward_masked(self, R, out, g, add):
        """a residual unit's bn2 backward behind cdnet_dam_head_backward_fused: g.t is dz already (the consumer's gradient through the
        unit's ReLU), so both passes take it as one plain relu = 0 source without residual - the sums pass reads two tensors instead of
        three and stores none, the same sums in the same order as _bn_backward's; dz goes to the 1x1 branch as there"""
        L = R.layer
        No, Ho, Wo, Co = out.shape
        a = self._bn_args(L, out, [_G(g.t, g.Hg, g.Wg)], res=None, relu=0)
        draw = self.buf(('draw', L.name), (No, Ho, Wo, Co), runtime.act_dtype())
        ws = self._ws('bn', _lib.load().cdnet_bn_backward_workspace_floats(Co))
        bn = L.bn
        _lib.call('cdnet_bn_backward', C.byref(a), _lib.ptr(bn.weight.detach()), _lib.ptr(bn.weight.grad), _lib.ptr(bn.bias.grad),
                  _lib.ptr(ws), ws.numel(), _lib.ptr(draw), None, _lib.stream_ptr())
        add(R.res, _G(g.t, Ho, Wo))
        return draw

    def _stats_fusable(self, L, srcs, H, W, N, wpb, cfgb, cin_total):
        """the single lazily transformed BatchNorm + ReLU source of a 3x3 convolution that is its only reader, and a backward-data
        launch that runs on the producer / consumer kernel: returns (producer layer, partial-row buffer) or None"""
        # fp32 mode only (conv_ws32_kernel): the sums ride in the CONSUMERS' deferred epilogue (raw quarters by DMA into LDS).  Round 2's
        # 16-bit form - the sums accumulated by the movers of conv_ws_kernel - saved 11 reduce passes and was not faster (the movers'
        # per-element arithmetic costs the matrix pipe issue time); it was removed in round 3.
        f32 = runtime.PRECISION == 'fp32'
        if not f32 or os.environ.get('CDNET_BN_STATS_FUSE', '1') != '1' or runtime.DEBUG_NORELU:
            return None
        if L.kind != 'conv3' or L.transposed or len(srcs) != 1:
            return None
        sx = srcs[0]
        if sx.is_input or sx.scale is None or sx.shift is None or sx.relu is not True or sx.res is not None or sx.pool \
                or tuple(sx.off) != (0, 0) or sx.x.dtype != runtime.raw_dtype() or sx.grad_to is not None or sx.row_stride:
            return None
        if f32 and cin_total % 64:
            return None
        PR = self._producer.get(id(sx.x))
        if PR is None or PR.layer.bn is None or PR.res is not None or PR.relu is not True \
                or self._readers.get(id(sx.x), 0) != 1 or tuple(sx.x.shape) != (N, H, W, cin_total):
            return None
        P = PR.layer
        key = ('statsfusable', L.name, N, H, W, runtime.PRECISION)
        hit = self._bufs.get(key)
        if hit is None:
            part = torch.zeros((1024, 2, cin_total), dtype=torch.float32, device=self.dev)
            gin = self.buf(('din', L.name), (N, H, W, cin_total), runtime.act_dtype())
            gdummy = self.buf(('draw', L.name), (N, H, W, L.Cout), runtime.act_dtype())
            ok = engine.conv_forward([Src(gdummy)], wpb, cin_total, cfgb, taps=L.taps, out=gin, H=H, W=W, query_ws=True,
                                     bns=(sx.x, P.scale, P.shift, P.save_mean, P.save_invstd, part))
            hit = self._bufs[key] = (part if ok else False)
        if hit is False:
            return None
        return P, hit

    def _bn_args(self, L, out, gl, res, relu):
        """cdnet_bn_bwd_args of layer L's stored output `out`: its gradient sources `gl` (at most 3), the residual branch `res`, the
        ReLU mode"""
        a = BnBwdArgs()
        a.raw = out.data_ptr()
        a.res = None if res is None else res.data_ptr()
        if L.bn is not None:
            a.scale, a.shift = L.scale.data_ptr(), L.shift.data_ptr()
            a.mean, a.invstd = L.save_mean.data_ptr(), L.save_invstd.data_ptr()
        a.ngin = len(gl)
        assert 1 <= len(gl) <= 3, (L.name, len(gl))
        for k, g in enumerate(gl):
            if g.hc is not None:
                coef, hw, w0, k0, nk = g.hc
                a.hc_coef, a.hc_w, a.hc_slot, a.hc_k0, a.hc_nk = coef.data_ptr(), hw.data_ptr() + 4 * w0, k, k0, nk
            a.gin[k].g = None if g.t is None else g.t.data_ptr()
            a.gin[k].Hg, a.gin[k].Wg, a.gin[k].oy, a.gin[k].ox = g.Hg, g.Wg, g.oy, g.ox
            a.gin[k].pooled, a.gin[k].coff, a.gin[k].cstride = int(g.pooled), g.coff, g.cstride or out.shape[3]
        a.f16 = {torch.bfloat16: 0, torch.float16: 1, torch.float32: 2}[out.dtype]
        a.relu = relu
        a.N, a.H, a.W, a.C = out.shape
        return a

    def _bn_backward(self, R, out, gl, add):
        L = R.layer
        No, Ho, Wo, Co = out.shape
        res = R.res
        has_bn = L.bn is not None
        if len(gl) > 3:
            # more consumers than the kernel takes gradient sources (an ablation head's first residual unit feeds two units, four
            # backward-data terms): fold the plain same-size terms beyond the second into one tensor first
            plain = [g for g in gl if not g.pooled and g.oy == 0 and g.ox == 0 and (g.Hg, g.Wg) == (Ho, Wo)]
            rest = [g for g in gl if g not in plain]
            assert len(rest) <= 2 and len(plain) >= 2, (L.name, len(gl))
            d = self.buf(('gsum', L.name), (No, Ho, Wo, Co), runtime.act_dtype())
            self.grad_sum(plain, None, No * Ho * Wo, Co, d)
            gl = rest + [_G(d, Ho, Wo)]
        a = self._bn_args(L, out, gl, res, int(R.relu))
        draw = self.buf(('draw', L.name), (No, Ho, Wo, Co), runtime.act_dtype())
        dz = None
        if res is not None:
            dz = self.buf(('dz', L.name), (No, Ho, Wo, Co), runtime.act_dtype())
        ws = self._ws('bn', _lib.load().cdnet_bn_backward_workspace_floats(Co))
        bn = L.bn
        _lib.call('cdnet_bn_backward', C.byref(a), _lib.ptr(bn.weight.detach()) if has_bn else None,
                  _lib.ptr(bn.weight.grad) if has_bn else None, _lib.ptr(bn.bias.grad) if has_bn else None,
                  _lib.ptr(ws), ws.numel(), _lib.ptr(draw), _lib.ptr(dz), _lib.stream_ptr())
        if res is not None:
            # gradient of the residual branch = dz; its producer (conv_1x1) is on the tape.  (HRNet's residual sums: `res` is the stored
            # output the mask is read from, the branch is the block's input - _residual_tail names it)
            add(R.res_grad_to if R.res_grad_to is not None else res, _G(dz, Ho, Wo))
            R.res_grad_to = None
        return draw

    def _side_stream(self):
        """second HIP stream for the weight-gradient kernels (trainer.WGRAD_STREAM = False: everything on one stream)"""
        if not WGRAD_STREAM or self.dev.type != 'cuda':
            return None
        if self._wstream is None:
            self._wstream = streams.side_stream(self.dev)      # (probed: a stream on another hardware queue than the compute stream's)
            self._events = {}
        return self._wstream

    def _event(self, k):
        e = self._events.get(k)
        if e is None:
            e = self._events[k] = torch.cuda.Event()
        return e

    def _weight_backward(self, L, srcs, g, H, W):
        lib = _lib.load()
        N = g.shape[0]
        Cout = L.Cout
        cin_total = sum(s.C for s in srcs)
        cin_real = L.Cin
        mode = {'conv3': 0, 'conv1': 0, 'convT4': 2, 'convT2': 3, 'conv3s2': 6}[L.kind]
        taps, npar, ostride = L.taps, (4 if L.transposed else 1), (2 if L.transposed else 1)
        cap = _wgrad_wgs(self._side_active and L.needs_input_grad, H * W, Cout)
        coff = 0
        for s in srcs:
            ci_t = _choose_ci_tiles(s.C, Cout)
            CI, CO = ci_t * 32, (4 // ci_t) * 32
            other = -(-s.C // CI) * -(-Cout // CO) * npar
            ntiles = N * (-(-H // 8)) * (-(-W // 16))
            ksplit = max(1, min(ntiles, cap // other if other < cap else 1))      # one 8-wave workgroup per CU
            nslab = lib.cdnet_conv_wgrad_slab_floats(s.C, Cout, taps, npar, ci_t, ksplit)
            defer = self._rd_mb > 0
            slab = self.buf(('wslab', L.name, coff), (nslab,), torch.float32) if defer else self._ws('slab', nslab, side=True)
            cs = engine.ConvSrc()
            s.fill(cs)
            csrc_real = min(s.C, cin_real - coff) if cin_total != cin_real else s.C
            _lib.call('cdnet_conv_backward_weight', C.byref(cs), coff, csrc_real, cin_real, _lib.ptr(g), Cout, N, H, W, taps,
                      npar, ostride, ci_t, ksplit, _lib.ptr(slab), _lib.ptr(L.weight.grad), mode | (_WGRAD_DEFER if defer else 0),
                      _lib.stream_ptr())
            if defer:
                self._rd_pending.append((s.C, coff, csrc_real, cin_real, Cout, taps, npar, ci_t, ksplit, slab.data_ptr(),
                                         L.weight.grad.data_ptr(), mode))
                self._rd_bytes += nslab * 4
            coff += s.C
        if L.bias is not None and L.bn is None:
            # bias of a BN-less conv (ResidualUnit.conv_1x1): sum of its output gradient == dbeta of the unit's bn2
            owner = L.bias_grad_from
            if owner is not None:
                L.bias.grad.copy_(owner.bn.bias.grad)
            else:
                # stand-alone biased convolution (plain UNet's ConvTranspose2d): db = sum of the output gradient
                ws = self._ws('slab', lib.cdnet_bias_grad_workspace_floats(Cout), side=True)
                _lib.call(_lib.entry('cdnet_bias_grad', g.dtype == torch.float32), _lib.ptr(g), g.numel() // Cout, Cout,
                          _lib.ptr(ws), ws.numel(), _lib.ptr(L.bias.grad), _lib.stream_ptr())

    def _narrow_ok(self, L, g, wpb, cfgb, gin, H, W, c_live):
        """may L's backward-data launch stop at output channel c_live?  The pack is laid out output-channel tile first (csrc/pack.hip), so
        its leading tiles are the pack of the narrower convolution, and an output element's sum does not depend on the other channels -
        as long as the same kernel family serves both launches (asked once per layer and shape; nothing is launched).  Otherwise the
        full launch stays"""
        key = ('narrow', L.name, tuple(g.shape), c_live, runtime.PRECISION, engine.CONV_DEBUG)
        ok = self._bufs.get(key)
        if ok is None:
            q = [engine.conv_forward([Src(g)], wpb, c, cfgb, taps=L.taps, out=gin, H=H, W=W, query_ws=True) for c in (gin.shape[3], c_live)]
            ok = self._bufs[key] = c_live % 8 == 0 and q[0] == q[1]
            self.narrowed[L.name] = c_live if ok else None     # (for tools/bench_finetune.py and the tests' printout)
        return ok

    def _input_backward(self, L, srcs, g, H, W, add):
        """g: the gradient w.r.t. the layer's raw output, or a prepared Src (BatchNorm-backward source of the fused path)"""
        if not L.needs_input_grad:
            return
        N = g.N if isinstance(g, Src) else g.shape[0]
        Cout = L.Cout
        cin_total = sum(s.C for s in srcs)
        # sources whose gradient has no reader (a frozen encoder's skip tensors and output, _no_grad_outputs)
        dead = [id((s.grad_to or (s.x,))[0]) in self._nograd for s in srcs] if self._nograd else [False] * len(srcs)
        if all(dead):
            return                                           # (the first decoder block's transposed convolution: nothing to compute)
        # input gradient: forward convolution with the backward-data pack
        wpb, cfgb = L.backward_pack(cin_total, H, W)
        if L.kind == 'conv3s2':
            # stride-2 convolution: gradient in the space-to-depth layout [N,H,W,(a,b,c)], then permuted to [N,2H,2W,C]
            Cp = cin_total // 4
            gs2d = self.buf(('ds2d', L.name), (N, H, W, cin_total), runtime.act_dtype())
            engine.conv_forward([Src(g)], wpb, cin_total, cfgb, taps=9, out=gs2d, H=H, W=W)
            gin = self.buf(('din', L.name), (N, 2 * H, 2 * W, Cp), runtime.act_dtype())
            _lib.call(_lib.entry('cdnet_s2d_to_nhwc', gin.dtype == torch.float32), _lib.ptr(gs2d), N, H, W, Cp, _lib.ptr(gin),
                      _lib.stream_ptr())
            add(srcs[0].x, _G(gin, 2 * H, 2 * W))
            return
        if not L.transposed:
            gin = self.buf(('din', L.name), (N, H, W, cin_total), runtime.act_dtype())
            fuse = None if isinstance(g, Src) else self._stats_fusable(L, srcs, H, W, N, wpb, cfgb, cin_total)
            if fuse is not None:
                # this launch also leaves the channel sums of the BatchNorm backward of its only source's producer
                P, part = fuse
                engine.conv_forward([Src(g)], wpb, cin_total, cfgb, taps=L.taps, out=gin, H=H, W=W,
                                    bns=(srcs[0].x, P.scale, P.shift, P.save_mean, P.save_invstd, part))
                self._bn_partials[id(srcs[0].x)] = part
            else:
                # torch.cat([x, skip]) -> conv2 with a dead skip: the launch computes the output channels [0, x.C) only - the leading
                # output-channel tiles of the same pack, written into the same wide buffer, so the reader sees the bits and the strides
                # of the full launch (_narrow_ok); the skip's channels of the buffer are neither written nor read
                c_live = srcs[0].C if dead == [False, True] and not isinstance(g, Src) and self._narrow_ok(L, g, wpb, cfgb, gin, H, W, srcs[0].C) \
                    else cin_total
                engine.conv_forward([g if isinstance(g, Src) else Src(g)], wpb, c_live, cfgb, taps=L.taps, out=gin, H=H, W=W)
        else:
            # space-to-depth view of g [N,2H,2W,Cout]: two row-parity sources of 2*Cout channels each
            gin = self.buf(('din', L.name), (N, H, W, cin_total), runtime.act_dtype())
            views = [Src(g, view=(a * 2 * W * Cout, H, W, 2 * Cout, 4 * W * Cout)) for a in (0, 1)]
            engine.conv_forward(views, wpb, cin_total, cfgb, taps=(9 if L.kind == 'convT4' else 1), out=gin, H=H, W=W)
        coff = 0
        for s, dead_s in zip(srcs, dead):
            if s.is_input or dead_s:
                coff += s.C
                continue
            tgt, pool = s.grad_to or (s.x, int(s.pool))          # a materialised max-pool hands its gradient to the producer
            add(tgt, _G(gin, H, W, oy=s.off[0], ox=s.off[1], pooled=pool, coff=coff, cstride=cin_total))
            coff += s.C

    # ------------------------------------------------------------------------------------------------
    # Gradient all-reduce overlapped with backward.  The flat gradient buffer is laid out in forward order, backward
    # fills it from the end: after every layer, each fixed-size bucket that lies completely above the highest parameter
    # still waiting for its gradient is handed to RCCL (async: the collective waits for the kernels already queued on
    # the compute stream and runs beside the rest of backward).  CDNET_ALLREDUCE_OVERLAP=0 keeps the single
    # post-backward pass.
    def _overlap_begin(self):
        self._ar = None
        if not self._reduce_active() or os.environ.get('CDNET_ALLREDUCE_OVERLAP', '1') == '0':
            return
        f = self.flat
        base = f.G.data_ptr()
        pend = {}
        owners = [p for L in (R.layer for R in self.tape if not isinstance(R, runtime.FuseRecord)) for p in (L.weight, L.bias, None if L.bn is None else L.bn.weight,
                                                 None if L.bn is None else L.bn.bias) if p is not None]
        for p in owners:
            off = (p.grad.data_ptr() - base) // 4
            if 0 <= off < f.n_used:
                pend[off] = off + p.numel()
        if f.n_head:
            pend[0] = f.n_head                       # the head block, written by the head backward kernel
        self._ar = BucketReducer(f.G, f.n_used, self.bucket, pend)

    def _overlap_done(self, params):
        """the gradients of `params` (or the head block when None) are final: launch every bucket now complete"""
        if self._ar is None:
            return
        if params is None:
            self._ar.done([0])
        else:
            base = self.flat.G.data_ptr()
            self._ar.done([(p.grad.data_ptr() - base) // 4 for p in params if p is not None])

    def _reduce_active(self):
        return self.world > 1 or os.environ.get('CDNET_FORCE_ALLREDUCE', '0') == '1'

    def allreduce_and_step(self):
        f = self.flat
        gscale = 1.0
        works = None
        if self._reduce_active():
            if self._ar is not None:
                # whatever backward did not release yet; then the optimiser follows the collectives bucket by bucket (top-down, the
                # order they were launched in): the last bucket's all-reduce - the first layers' gradients, complete only when backward
                # ends - runs while Adam already updates the ranges above it
                ranges = self._ar.finish(wait=False)
                works = self._ar.works
                self.ar_stats = dict(buckets=len(works), released_during_backward=self._ar.early)
                self._ar = None
            else:
                bucketed_allreduce(f.G, f.n_used, self.bucket)
            gscale = 1.0 / self.world
        f.step_count += 1
        step = self._rule_stepper(gscale)
        if works is None:
            step(0, f.n_used)
        else:
            for w, (a, b) in zip(works, ranges):
                w.wait()                                 # (the current stream waits, not the host)
                step(a, b)
        runtime.WEIGHTS_EPOCH[0] += 1
        self._repack_all()

    def _rule_stepper(self, gscale):
        """step(a, b) of this trainer's optimiser over the range [a, b) of the flat buffers.  The rules live in optim.stepper; this name
        stays because tests/test_gpu_optim.py steps bucket ranges through it - nothing else belongs here"""
        return optim.stepper(self, gscale)

    def _repack_all(self):
        """Re-pack every layer's forward / backward-data weights in one launch (they would otherwise be re-packed one by
        one, lazily, by the next forward and backward).  The job table is built after the first step, once every layer
        has its packed buffers."""
        f = self.flat
        lo, hi = f.P.data_ptr(), f.P.data_ptr() + f.P.numel() * 4
        if self._pack_jobs is not None and self._pack_prec != runtime.PRECISION:
            self._pack_jobs = None                           # the layers re-made their packs for the other precision
        if self._pack_jobs is None:
            groups = ([], []), ([], [])                      # (jobs, owners) of the forward packs / the backward-data packs
            for L in runtime.LAYERS:
                if not (lo <= L.weight.data_ptr() < hi):
                    continue
                w = L.weight.detach()
                if L.wp is not None and not L.wp_padded:
                    groups[0][0].append(engine.pack_job(w, L.cfg, L.pack_mode, L.wp, split=L.cfg_f32)); groups[0][1].append((L, 'wp_version'))
                if L.wpb is not None:
                    mode = (4 if L.kind == 'convT4' else 5) if L.transposed else (7 if L.kind == 'conv3s2' else 1)
                    groups[1][0].append(engine.pack_job(w, L.cfg_bwd, mode, L.wpb, split=L.cfg_f32)); groups[1][1].append((L, 'wpb_version'))
            if not groups[0][0] or not groups[1][0] or self.flat.step_count < 1:
                return
            self._pack_jobs = []
            self._pack_prec = runtime.PRECISION
            for jobs, owners in groups:
                arr = (engine.PackJob * len(jobs))(*jobs)
                nbytes = _lib.load().cdnet_pack_batch_table_bytes(len(jobs))
                table = torch.empty((nbytes,), dtype=torch.uint8, device=f.P.device)
                self._pack_jobs.append((arr, len(jobs), table, owners, [True]))
        side = self._side_stream()
        for k, (arr, n, table, owners, first) in enumerate(self._pack_jobs):
            if k == 1 and side is not None and self._packb_stream:
                # the backward-data packs are not needed before the next backward: pack them beside the next forward
                ev = self._event('adam')
                ev.record()
                side.wait_event(ev)
                with _on_stream(side):
                    _lib.call('cdnet_pack_conv_weights_batch', C.byref(arr), n, _lib.ptr(table), table.numel(), int(first[0]), _lib.stream_ptr())
                    self._event('packb').record()
                self._packb_pending = True
            else:
                _lib.call('cdnet_pack_conv_weights_batch', C.byref(arr), n, _lib.ptr(table), table.numel(), int(first[0]), _lib.stream_ptr())
            first[0] = False
            for L, attr in owners:
                setattr(L, attr, (L.weight._version, runtime.WEIGHTS_EPOCH[0]))

    # ------------------------------------------------------------------------------------------------
    def write_bn_counters(self):
        """nn.BatchNorm2d.num_batches_tracked of every BatchNorm that ran = the number of training forwards (PyTorch adds one per
        forward, `nn.BatchNorm2d.forward`); kept as a host counter during training and written out for checkpoints"""
        with torch.no_grad():
            unused = tuple(getattr(self.model, 'UNUSED_PREFIXES', ()))
            for name, mod in self.model.named_modules():
                if isinstance(mod, torch.nn.BatchNorm2d) and mod.num_batches_tracked is not None and not (name + '.').startswith(unused or ('\0',)):
                    mod.num_batches_tracked.fill_(self._bn_base + self._forwards)

    def refresh_parameters(self):
        """call after writing parameters behind the trainer's back (load_state_dict does not need it: the module's parameters
        ARE views of the flat buffer; this only invalidates every packed bf16 weight copy and BatchNorm fold)"""
        if hasattr(self.model, 'sync_real_parameters') and getattr(self.model, '_rt', None) is not None:
            self.model._ensure_runtime()
        runtime.WEIGHTS_EPOCH[0] += 1

    def state_dict(self):
        """the optimiser entry of a checkpoint, in the layout of the reference's object for this optimiser (optim.state_dict)"""
        return optim.state_dict(self)

    def load_state_dict(self, sd):
        """continue from such an entry: the state buffers, the step count and the group's lr / weight decay / betas / eps / momentum
        (optim.load_state_dict)"""
        optim.load_state_dict(self, sd)

    def train_step(self, x, label, dirlab, point_t, weight):
        """x f32 [B,3,H,W]; label u8 [B,H,W] in {0,1,2}; dirlab u8 [B,H,W] 0..8; point_t f16 [B,H,W]; weight u8 [B,H,W]
        (the png weight map; /20 on the fly).  Returns the device tensor of 11 values: [total, direction CE, direction dice,
        MSE, CE, dice, pixel accuracy, IoU, recall, precision, F1] (train_util_dam.py:297-299; slot 5 holds the mask dice
        term where the reference logs its variance term; that one is `self.loss_var`, part of the total when alpha = 1)."""
        mask, point, direction = self.forward(x)
        dmask, dpoint, ddir = self.loss_and_grads(mask, point, direction, label, dirlab, point_t, weight)
        self.backward(dmask, dpoint, ddir)
        self.allreduce_and_step()
        return self.losses


class UNetTrainer(Trainer):
    """Body of the plain-UNet train iteration (train_util.py:58-234): log-softmax + NLL (x weight map / 20 with `weight_map`) mean,
    + MulticlassDiceLoss on the softmax (`dice` 1; 2: the dice term alone; 0: none), `alpha` 1 adds the variance term and 2 puts twice
    that term in the cross-entropy's place, `boundary` adds its term -> backward -> the optimiser step.  The loss, its gradient and the
    pixel metrics of the arg-max come from one cdnet_mask_loss call: `unet_losses` = [total, CE, dice], `unet_metrics` = [accuracy, IoU,
    recall, precision, F1] (:209-218)."""

    def __init__(self, model, **kw):
        super().__init__(model, **kw)
        self.mask_losses = torch.zeros((8,), dtype=torch.float32, device=self.dev)      # cdnet_mask_loss: total, ce, dice, 5 metrics
        self.unet_losses = self.mask_losses[0:3]
        self.unet_metrics = self.mask_losses[3:8]

    def mask_loss(self, logits, label, weight, terms, dmask):
        """one cdnet_mask_loss call into `mask_losses`; dmask None: values only (validate)"""
        B, K, H, W = logits.shape
        if K != 3:
            raise ValueError('the mask loss serves the 3-class configuration (options.py: out_c = 3), got %d classes' % K)
        assert label.dtype == torch.uint8 and (weight is None or weight.dtype == torch.uint8)
        ws = self._ws('mask_loss', _lib.load().cdnet_mask_loss_workspace_floats(B, H * W))
        _lib.call('cdnet_mask_loss', _lib.ptr(logits), _lib.ptr(label.contiguous()), None if weight is None else _lib.ptr(weight.contiguous()),
                  B, H, W, terms, _lib.ptr(ws), ws.numel(), _lib.ptr(self.mask_losses), None if dmask is None else _lib.ptr(dmask),
                  _lib.stream_ptr())

    def loss_and_grads(self, logits, label, weight):
        from .utils import loss_terms
        terms = loss_terms(self.dice, self.weight_map, self.alpha)
        dmask = self.buf('dmask', logits.shape, torch.float32)
        self.mask_loss(logits, label, weight, terms, dmask)
        total = self.mask_losses[0:1]
        if self.dice == 2:
            # train_util.py:187-190: loss = loss_dice - the variance term is computed for the log only, the boundary term not at all
            if self.alpha:
                self._variance_term(logits, label, None)
            return dmask
        if self.alpha:
            self._variance_term(logits, label, dmask, total)       # loss = loss_CE + loss_var (alpha 1) | 2 * loss_var (alpha 2) (+ dice)
        if self.boundary:
            self._boundary_term(logits, label, dmask, total)       # train_util.py:170-178: loss = loss + beta * boundary_loss, beta = 1
        return dmask

    def backward(self, dlogits):
        conv, feat = self.model.final_conv, self.model._last_feat
        self._run_tape([(feat.x, self._classifier_backward('dF', feat, conv, dlogits))], [conv.weight, conv.bias])

    def train_step(self, x, label, weight):
        """x f32 [B,3,H,W]; label u8 [B,H,W] in {0,1,2}; weight u8 [B,H,W] (png weight map, /20 on the fly,
        train_util.py:109).  Returns the device tensor [total, CE, dice]."""
        logits = self.forward(x)
        dlogits = self.loss_and_grads(logits, label, weight)
        self.backward(dlogits)
        self.allreduce_and_step()
        return self.unet_losses


class BackboneUNetTrainer(UNetTrainer):
    """Train iteration of the backbone U-Net (models/model_unet.py through train_util.train): the plain UNet's loss, optimiser, all-reduce
    and checkpoint entry; the classifier reads the decoder's 16-channel feature (cdnet_final_conv1x1_c16_backward), the rest is the rev1
    tape."""

    def _classifier_backward(self, key, f, conv, dl):
        N, H, W, _ = f.x.shape
        K = conv.out_channels
        df = self.buf(key, (N, H, W, 16), runtime.act_dtype())
        ws = self._ws('classifier16', _lib.load().cdnet_final_conv1x1_c16_backward_workspace_floats())
        hf = runtime.head_feat16(f)
        w = conv.weight.detach().reshape(K, 16)
        _lib.call('cdnet_final_conv1x1_c16_backward', C.byref(hf), _lib.ptr(w), _lib.ptr(dl), K, N, H, W, _lib.ptr(df), _lib.ptr(ws),
                  ws.numel(), _lib.ptr(conv.weight.grad), _lib.ptr(conv.bias.grad), _lib.stream_ptr())
        return _G(df, H, W)


class FullNetTrainer(UNetTrainer):
    """Train iteration of FullNet (models/FullNet.py through train_util.train): the plain UNet's loss, optimiser, all-reduce and checkpoint
    entry around the network's own training forward and backward (models/FullNet.py: _train_forward / train_backward on csrc/dilated.hip and
    csrc/dilated_train.hip).  fp32 precision mode only; one stream, the gradients reduced after backward (bucketed_allreduce).
    The dropout masks are a hash of (seed, optimiser steps taken so far, layer, element): `seed` is opt.train['seed'] + rank."""

    def __init__(self, model, seed=0, **kw):
        if runtime.PRECISION != 'fp32':
            raise NotImplementedError('FullNet trains in the fp32 precision mode only (CDNET_PRECISION=fp32 / runtime.set_precision("fp32")); '
                                      'bf16-mode training is not built')
        super().__init__(model, **kw)
        self.seed = int(seed)

    def dropout_key(self):
        """the 64-bit key of this step's masks (cdnet_dropout_mask)"""
        return ((self.seed & 0xffffffff) << 32) | (self.flat.step_count & 0xffffffff)

    def forward(self, x):
        self.model._train_key = self.dropout_key()
        return super().forward(x)

    def backward(self, dlogits):
        self._ar = None                                    # (no overlap: allreduce_and_step reduces the whole buffer behind backward)
        self.model.train_backward(self.tape[-1], dlogits)


class AblationTrainer(Trainer):
    """Train iteration of the ablation heads (models/dam/model_unet_MandD.py / model_unet_MandDandP.py through
    train_util_dam.train, which unpacks the model's outputs by their number, :152-166): the same five-term loss - without the point
    term for the two-output model (options direction = 1, mseloss = 0) - plain 1x1 classifiers instead of the gated head
    (cdnet_final_conv1x1 / cdnet_final_conv1x1_backward), everything else the rev1 tape.  The direction branch has 5, 9 or 17
    classes (model_unet_MandD4 / MandD / MandD16; cdnet_dam_loss_classes)."""

    def __init__(self, model, **kw):
        assert getattr(model, 'VARIANT', 'rev1') in ('MandD', 'MandDandP') and model.DIRECTION_OUT in (5, 9, 17), \
            'AblationTrainer serves model_unet_MandD / MandD4 / MandD16 / MandDandP'
        super().__init__(model, **kw)

    def loss_and_grads(self, outputs, label, dirlab, point_t, weight):
        if len(outputs) == 3:
            return super().loss_and_grads(outputs[0], outputs[1], outputs[2], label, dirlab, point_t, weight)
        mask, direction = outputs
        B, _, H, W = mask.shape
        point = self.buf('zero_point', (B, 1, H, W), torch.float32)
        pt = self.buf('zero_point_t', (B, H, W), torch.float16)
        point.zero_()
        pt.zero_()
        dmask, _, ddir = super().loss_and_grads(mask, point, direction, label, dirlab, pt, weight)
        return dmask, None, ddir

    def backward(self, dmask, dpoint, ddir):
        m = self.model
        f1m, f2, f3 = m._last_feats
        heads, params = [], []
        for name, f, conv, dl in (('m', f1m, m.mask_conv, dmask), ('d', f2, m.direction_conv, ddir), ('p', f3, m.point_conv, dpoint)):
            if f is None or dl is None:
                continue
            heads.append(((f.grad_to or (f.x,))[0], self._classifier_backward('dF' + name, f, conv, dl)))
            params += [conv.weight, conv.bias]
        self._run_tape(heads, params)

    def train_step(self, x, label, dirlab, point_t, weight):
        out = self.forward(x)
        g = self.loss_and_grads(out, label, dirlab, point_t, weight)
        self.backward(*g)
        self.allreduce_and_step()
        return self.losses


# ----------------------------------------------------------------------------------------------------------
def make_bench_step(model, B, dev, rank, world):
    """the benchmark's training step on a fixed synthetic batch: eager launches (a HIP-graph replay of forward + loss + backward was measured
    6-20 % slower on this step - the GPU, not the launch path, bounds it; cdnet_amd.graphs stays for the launch-bound HRNet step,
    tools/bench_hrnet.py)"""
    tr = Trainer(model, world_size=world)
    batch = synthetic_batch(B, dev, seed=2022 + rank)

    def step():
        return tr.train_step(*batch)
    metric = 'tiles/sec (train fwd+bwd+Adam), 256x256'
    workload = ('CDNet UNet2RevA1_vgg16 (UNet+DAM) training step: forward, 5-term loss, backward%s, %s fused Adam; '
                '256x256x3 synthetic tiles, batch %d per GPU' % ('', 'RCCL gradient all-reduce,' if world > 1 else '', B))
    return step, metric, workload
