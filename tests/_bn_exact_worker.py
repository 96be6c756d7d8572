"""child process of tests/test_gpu_bn_bwd_exact.py::test_flat_residual_apply_without_dz_reuse, started with CDNET_BN_DZ_REUSE=0 (read once
per process by libcdnet_hip.so): the rows named on the command line through check_row with the apply pass on the caller's sources.
Prints {row id: apply plan} as one JSON line."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main(ids):
    import _bn_exact_cases as bx
    from cdnet_amd import _lib
    assert os.environ.get('CDNET_BN_DZ_REUSE') == '0'
    plans = {}
    for rid in ids:
        row = bx.ROW_BY_ID[rid]
        d = bx.make_data(row)
        ref = bx.reference(row, d, reuse=False)
        bx.guard(row, d, ref)
        bx.check_row(row, d, ref, reuse=False)
        plans[rid] = _lib.load().cdnet_bn_backward_last_plan()
    print(json.dumps(plans))


if __name__ == '__main__':
    main(sys.argv[1:])
