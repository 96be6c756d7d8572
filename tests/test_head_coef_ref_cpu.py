"""The reference that tests/test_gpu_head_coef_src.py compares bits with (tests/_head_coef_ref.py) is itself checked here, without a
GPU: its fused multiply-add rounds once, and its chains stay within the rounding bound of fp64 - a reference that returned zeros or
the wrong columns would fail here, not pass there in silence.  And the refusals that need no device."""
import ctypes as C

import pytest
import torch

from _head_coef_ref import K0, fma32, rebuild


def test_fma32_rounds_once():
    """a * b + c = 1 + 2^-23 + 2^-24 - 2^-70: just below the midpoint of two fp32 values.  Rounded to fp64 first it IS the midpoint, and
    the second rounding then goes up to the even neighbour 1 + 2^-22; one rounding gives 1 + 2^-23"""
    a = torch.tensor([2.0 ** -24 * (1 + 2.0 ** -23)], dtype=torch.float32)
    b = torch.tensor([1 - 2.0 ** -23], dtype=torch.float32)
    c = torch.tensor([1 + 2.0 ** -23], dtype=torch.float32)
    assert float((a.double() * b.double() + c.double()).float()) == 1 + 2.0 ** -22          # (the trap is real)
    assert float(fma32(a, b, c)) == 1 + 2.0 ** -23
    assert float(fma32(-a, b, -c)) == -(1 + 2.0 ** -23)
    # exact cases, and the sign of zero: (-0) + (+0) = +0
    x = torch.tensor([3.0, -0.0, 0.0, 1.5], dtype=torch.float32)
    y = torch.tensor([0.5, 2.0, -2.0, 1.5], dtype=torch.float32)
    z = torch.tensor([0.25, 0.0, 0.0, -2.25], dtype=torch.float32)
    r = fma32(x, y, z)
    assert r.tolist() == [1.75, 0.0, 0.0, 0.0]
    assert not torch.signbit(r).any()


def test_fma32_against_exact_integers():
    """24-bit integers: a * b + c computed in int64 is exact; its fp32 rounding (int64 -> float64 is exact below 2^53, float64 -> fp32
    rounds once) must be what fma32 gives"""
    g = torch.Generator().manual_seed(5)
    a = torch.randint(-2 ** 24 + 1, 2 ** 24, (20000,), generator=g)
    b = torch.randint(-2 ** 24 + 1, 2 ** 24, (20000,), generator=g)
    c = torch.randint(-2 ** 24 + 1, 2 ** 24, (20000,), generator=g) * 2 ** 20
    want = (a * b + c).double().float()           # |a b + c| < 2^49
    got = fma32(a.float(), b.float(), c.float())
    assert torch.equal(got, want)


@pytest.mark.parametrize('nk', [3, 9])
def test_rebuild_stays_within_the_rounding_bound_of_fp64(nk):
    """every one of the nk steps rounds a partial sum whose magnitude is at most S = sum_k |coef_k w_k|, by at most half an ulp: relative
    2^-24 of it.  So |chain - exact| <= nk 2^-24 S (1 ulp-scale per step); the fp64 value is exact to 2^-53 S per operation, far below"""
    g = torch.Generator().manual_seed(11 + nk)
    coef = torch.randn((500, 16), generator=g)
    w = torch.randn((nk, 64), generator=g)
    got = rebuild(coef, w, K0[nk], nk)
    cols = coef[:, K0[nk]:K0[nk] + nk].double()
    want = cols @ w.double()
    bound = nk * 2.0 ** -24 * (cols.abs() @ w.double().abs())
    err = (got.double() - want).abs()
    assert got.dtype == torch.float32 and got.shape == (500, 64)
    assert bool((err <= bound).all()), float((err / bound).max())
    assert float(err.max()) > 0            # (and it is an fp32 chain, not the fp64 product rounded at the end)
    # the other columns are not read
    other = coef.clone()
    keep = torch.zeros(16, dtype=torch.bool)
    keep[K0[nk]:K0[nk] + nk] = True
    other[:, ~keep] = 1e30
    assert torch.equal(rebuild(other, w, K0[nk], nk), got)


def test_rebuild_of_a_zero_row_is_plus_zero():
    w = -torch.rand((9, 64)) - 0.5
    v = rebuild(torch.zeros((4, 16)), w, 1, 9)
    assert torch.equal(v, torch.zeros((4, 64))) and not torch.signbit(v).any()


def _args(**kw):
    from cdnet_amd import _lib
    A = _lib.BnBwdArgs()
    fake = 4096                                     # (never dereferenced: every call below is refused before any HIP call)
    A.raw, A.res, A.scale, A.shift, A.mean, A.invstd = [fake] * 6
    A.ngin = 3
    for k in range(3):
        A.gin[k].g, A.gin[k].Hg, A.gin[k].Wg, A.gin[k].cstride = fake, 8, 8, 64
    A.f16, A.relu, A.N, A.H, A.W, A.C = 2, 2, 1, 8, 8, 64
    A.hc_coef, A.hc_w, A.hc_slot, A.hc_k0, A.hc_nk = fake, fake, 1, 10, 3
    A.gin[1].g = None
    for k, v in kw.items():
        setattr(A, k, v)
    return A


@pytest.mark.parametrize('bad', [dict(hc_nk=4), dict(hc_k0=9), dict(hc_nk=9, hc_k0=10), dict(hc_coef=None), dict(hc_w=None), dict(C=128),
                                 dict(f16=0), dict(f16=1), dict(relu=1, mean=None, invstd=None),
                                 # (refused by an older rule: a null source that is not the slot, relu = 2 without res)
                                 dict(hc_slot=3), dict(hc_slot=-1), dict(res=None)])
def test_bad_head_coefficient_arguments_are_refused_before_any_launch(bad):
    from cdnet_amd import _lib
    lib = _lib.load()
    fake = C.c_void_p(4096)
    A = _args(**bad)
    assert lib.cdnet_bn_backward(C.byref(A), fake, fake, fake, fake, 1 << 30, fake, fake, None) == 1, bad
    if 'hc_slot' not in bad and 'res' not in bad:
        assert b'head-coefficient' in lib.cdnet_last_error()


def test_a_slot_past_the_sources_is_refused():
    from cdnet_amd import _lib
    lib = _lib.load()
    fake = C.c_void_p(4096)
    A = _args(hc_slot=2, ngin=2)
    A.gin[1].g = 4096
    assert lib.cdnet_bn_backward(C.byref(A), fake, fake, fake, fake, 1 << 30, fake, fake, None) == 1
    assert b'head-coefficient' in lib.cdnet_last_error()


def test_entries_that_cannot_serve_a_head_coefficient_source_refuse_it():
    from cdnet_amd import _lib
    lib = _lib.load()
    fake = C.c_void_p(4096)
    A = _args()
    assert lib.cdnet_bn_backward(C.byref(A), fake, fake, fake, fake, 1 << 30, fake, None, None) == 1            # no dz_out: no stored dz
    A = _args()
    A.gin[0].pooled, A.gin[0].Hg, A.gin[0].Wg = 1, 4, 4                                                       # a pooled source beside it
    assert lib.cdnet_bn_backward(C.byref(A), fake, fake, fake, fake, 1 << 30, fake, fake, None) == 1
    A = _args(ngin=1, hc_slot=0, res=None, relu=1)
    A.gin[0].g = None
    assert lib.cdnet_bn_backward_stats(C.byref(A), fake, fake, fake, fake, 1 << 30, fake, None) == 1
    assert lib.cdnet_bn_backward_apply(C.byref(A), fake, fake, None) == 1
    assert lib.cdnet_bn_backward_finalize(C.byref(A), fake, fake, fake, fake, 1, fake, None) == 1
