"""Digest of two consecutive training steps from a fixed seed: which ABI calls the steps make, with which arguments, and the bits they leave.

The step is deterministic (tests/test_gpu_train_step.py: test_full_size_step_is_deterministic_and_learns), so two trees that print the same
lines for a configuration make the same launches in the same order on the same streams and compute the same bits - the evidence a
host-side refactor of the runtime / trainer needs.  Every launching entry goes through _lib.call (what the package calls on
_lib.load() directly are size, eligibility and version queries), which this tool wraps for the duration of a step.  Per step it prints
  * the number of ABI calls;
  * a SHA-256 over the sequence of (entry name, the stream's ordinal by first appearance, every scalar argument including the scalar fields
    of struct arguments, a null / non-null flag per pointer) - addresses themselves differ from process to process and stay out;
  * the SHA-256 of the flat parameter buffer, the flat gradient buffer and the loss values after the step.

  python3 tools/step_digest.py --list                                     the configurations, one command line each
  python3 tools/step_digest.py rev1 2 64 --precision fp32 --wgrad-stream 0
  python3 tools/step_digest.py hrnet 4 512 --root /path/to/another/tree   the same file against another checkout's cdnet_amd
  (--dump FILE writes the call sequence itself, one call per line, to locate a difference)"""
import argparse
import ctypes as C
import hashlib
import importlib
import os
import sys

# (model, batch, height, precision, weight-gradient stream[, width]): the shapes of the models' own training tests, the benchmark's 16 x 256 x 256 and HRNet's 4 x 512 x 512
CONFIGS = [('rev1', 2, 64, p, w) for p in ('fp32', 'bf16') for w in (1, 0)] + [('rev1', 16, 256, p, w) for p in ('fp32', 'bf16') for w in (1, 0)] + \
    [('hrnet', 4, 512, 'bf16', 1), ('hrnet', 2, 64, 'fp32', 1)] + \
    [(m, 2, 64, p, 1) for m in ('unet', 'MandD', 'MandDandP', 'UNet_vgg16') for p in ('fp32', 'bf16')] + \
    [('FullNet', 2, 40, 'fp32', 1, 36), ('FCN_pooling', 2, 32, 'fp32', 1)]


# the batched re-pack's job table is built by iterating runtime.LAYERS, a WeakSet: the order of its (independent) jobs follows object addresses
# and differs from process to process as pointers do - its elements enter the digest sorted
UNORDERED = ('cdnet_pack_conv_weights_batch',)


def tokens(ctype, v, out, unordered=False):
    """the digest's view of one argument of declared type `ctype`: pointers as a null flag, scalars as they are, structs field by field"""
    obj = getattr(v, '_obj', None)                     # C.byref(struct or array of structs)
    if obj is not None:
        elems = []
        for e in (obj if isinstance(obj, C.Array) else (obj,)):
            elems.append([])
            tokens(type(e), e, elems[-1])
        for e in (sorted(elems) if unordered else elems):
            out += e
    elif isinstance(v, C.Structure):
        for name, ftype in v._fields_:
            tokens(ftype, getattr(v, name), out)
    elif isinstance(v, C.Array):
        for e in v:
            tokens(v._type_, e, out)
    elif ctype is C.c_void_p or ctype is C.c_char_p:
        p = v.value if isinstance(v, C.c_void_p) else v
        out.append('p%d' % bool(p))
    else:
        out.append(repr(v.value if isinstance(v, C._SimpleCData) else v))


class Recorder:
    def __init__(self, _lib):
        self._lib, self.inner, self.calls, self.streams = _lib, _lib.call, [], {}

    def __enter__(self):
        self._lib.call = self
        return self

    def __exit__(self, *exc):
        self._lib.call = self.inner
        return False

    def __call__(self, name, *args):
        types = self._lib.SIGNATURES[name][1]
        assert len(types) == len(args), name
        out, n = [name], len(args)
        if types and types[-1] is C.c_void_p and isinstance(args[-1], C.c_void_p):          # the stream: always the last argument
            out.append('s%d' % self.streams.setdefault(args[-1].value, len(self.streams)))
            n -= 1
        for t, a in zip(types[:n], args[:n]):
            tokens(t, a, out, name in UNORDERED)
        self.calls.append(' '.join(out))
        return self.inner(name, *args)


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(-1).numpy().tobytes()).hexdigest()


def make(model, B, H, W, dev):
    """(trainer, arguments of train_step, the tensor of loss values)"""
    import torch
    from cdnet_amd import trainer
    x, label, dirlab, point_t, weight = trainer.synthetic_batch(B, dev, seed=11, H=H, W=W)
    torch.manual_seed(3)
    if model in ('rev1', 'MandD', 'MandDandP'):
        m = importlib.import_module('cdnet_amd.models.dam.model_unet_' + model).Unet(backbone_name='vgg16_bn', pretrained=False, classes=3)
        tr = (trainer.Trainer if model == 'rev1' else trainer.AblationTrainer)(m.to(dev))
        return tr, (x, label, dirlab, point_t, weight), tr.losses
    if model == 'hrnet':
        from cdnet_amd.models.dam.seg_hrnet_rev1 import HighResolutionNet
        tr = trainer.Trainer(HighResolutionNet(argparse.Namespace(model={'out_c': 3})).to(dev).train())
        return tr, (x, label, dirlab, point_t, weight), tr.losses
    if model == 'unet':
        from cdnet_amd.models.unet import UNet
        tr = trainer.UNetTrainer(UNet(num_classes=3).to(dev))
    elif model == 'UNet_vgg16':
        from cdnet_amd.models.model_unet import Unet
        tr = trainer.BackboneUNetTrainer(Unet(backbone_name='vgg16_bn', pretrained=False, encoder_freeze=False, classes=3).to(dev))
    else:
        from cdnet_amd.models import FullNet
        tr = trainer.FullNetTrainer(getattr(FullNet, model)(3, 3).to(dev), seed=7)
    return tr, (x, label, weight), tr.mask_losses


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('model', nargs='?', choices=sorted(set(c[0] for c in CONFIGS)))
    ap.add_argument('batch', nargs='?', type=int, default=2)
    ap.add_argument('size', nargs='?', type=int, default=64)
    ap.add_argument('--precision', choices=('fp32', 'bf16'), default='bf16')
    ap.add_argument('--width', type=int, help='default: the size')
    ap.add_argument('--wgrad-stream', type=int, choices=(0, 1), default=1)
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help='the tree whose cdnet_amd runs')
    ap.add_argument('--dump', help='write the call sequence of both steps to this file')
    ap.add_argument('--list', action='store_true')
    a = ap.parse_args()
    if a.list or a.model is None:
        for m, B, S, p, w, *width in CONFIGS:
            print('%s %d %d --precision %s --wgrad-stream %d%s' % (m, B, S, p, w, ' --width %d' % width[0] if width else ''))
        return
    sys.path.insert(0, a.root)
    import torch
    from cdnet_amd import _lib, runtime, trainer
    assert os.path.abspath(trainer.__file__).startswith(os.path.abspath(a.root) + os.sep), trainer.__file__
    runtime.set_precision(a.precision)
    trainer.WGRAD_STREAM = bool(a.wgrad_stream)
    tr, batch, losses = make(a.model, a.batch, a.size, a.width or a.size, torch.device('cuda:0'))
    tag = '%s %dx%dx%d %s wgrad_stream=%d' % (a.model, a.batch, a.size, a.width or a.size, a.precision, a.wgrad_stream)
    dump = []
    for step in (1, 2):
        with Recorder(_lib) as rec:
            tr.train_step(*batch)
        torch.cuda.synchronize()
        dump += ['# step %d' % step] + rec.calls
        print('%s step %d: calls %d streams %d seq %s P %s G %s losses %s' % (
            tag, step, len(rec.calls), len(rec.streams), hashlib.sha256('\n'.join(rec.calls).encode()).hexdigest()[:16],
            sha(tr.flat.P)[:16], sha(tr.flat.G)[:16], sha(losses)[:16]), flush=True)
    if a.dump:
        with open(a.dump, 'w') as f:
            f.write('\n'.join(dump) + '\n')


if __name__ == '__main__':
    main()
