"""SHA-256 of every parameter of HighResolutionNet after two training steps from a fixed seed (4 tiles of 64 x 64, synthetic batch), in
the precision mode of CDNET_PRECISION: two builds of the library print the same line exactly when the training step computes the same bits.

  [CDNET_PRECISION=fp32] [CDNET_LIB_PATH=...] python tools/hrnet_train_digest.py"""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from cdnet_amd import runtime, trainer  # noqa: E402
from cdnet_amd.models.dam.seg_hrnet_rev1 import HighResolutionNet  # noqa: E402


class O:
    model = {'out_c': 3}


torch.manual_seed(0)
m = HighResolutionNet(O()).cuda().train()
tr = trainer.Trainer(m)
batch = trainer.synthetic_batch(4, torch.device('cuda:0'), seed=5, H=64, W=64)
losses = [float(tr.train_step(*batch)[0]) for _ in range(2)]
torch.cuda.synchronize()
h = hashlib.sha256()
for name, p in sorted(m.named_parameters()):
    h.update(name.encode())
    h.update(p.detach().float().cpu().numpy().tobytes())
print('%s %s losses %r' % (runtime.PRECISION, h.hexdigest(), losses))
