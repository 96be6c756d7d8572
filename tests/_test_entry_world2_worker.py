"""Worker of tests/test_gpu_test_entry.py: one of TWO ranks that share the one GPU of the box (gloo group) running `cdnet_amd.test.main` on
its shard of the images; writes its return value to <out>/rank<r>.json (argv: out, then main's arguments)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ['CDNET_DIST_BACKEND'] = 'gloo'
import torch

torch.cuda.set_device(0)
from cdnet_amd import test

avg = test.main(sys.argv[2:])
with open(os.path.join(sys.argv[1], 'rank%s.json' % os.environ['RANK']), 'w') as fh:
    json.dump(avg, fh)
