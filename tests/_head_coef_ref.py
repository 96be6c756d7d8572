"""Reference of the head-coefficient gradient source (cdnet_bn_bwd_args.hc_*): the DAM head's feature gradient rebuilt from a pixel's
coefficient row and the head's weight rows with the kernels' own chain of fp32 fused multiply-adds,

    v = fma(coef[p][k0], w[0][c], +0);   v = fma(coef[p][k0 + k], w[k][c], v),  k = 1 .. nk - 1

computed exactly in torch (CPU or device), so a test can ask for equal bits."""
import torch

K0 = {3: 10, 9: 1}          # first column of the row [dpt | du[9] | dm[3] | 0 0 0] for the mask head (3 terms) / the direction head (9)
W0 = {3: 640, 9: 64}        # first float of the weight rows wm[3][64] / wd[9][64] inside the 855-float head weight block


def fma32(a, b, c):
    """the fp32 fused multiply-add, round_to_nearest_even_f32(a * b + c) with one rounding, of fp32 tensors.

    In float64 the product of two fp32 values is exact (48 bits).  The sum p + c is not, and rounding it to 53 bits and then to 24 can
    round twice; so the sum is rounded to ODD instead (its exact error comes from the two-sum): a 53-bit round-to-odd value rounds to
    fp32 like the exact one (53 >= 2 * 24 + 2)."""
    assert a.dtype == b.dtype == c.dtype == torch.float32
    a, b, c = torch.broadcast_tensors(a.double(), b.double(), c.double())
    p = a * b
    s = p + c
    t = s - p
    err = (p - (s - t)) + (c - t)                 # exact: p + c == s + err
    even = (s.contiguous().view(torch.int64) & 1) == 0
    inf = torch.full_like(s, float('inf'))
    s = torch.where(even & (err > 0), torch.nextafter(s, inf), torch.where(even & (err < 0), torch.nextafter(s, -inf), s))
    return s.float()


def rebuild(coef, w, k0, nk):
    """coef f32 [..., 16], w f32 [nk][64] -> f32 [..., 64]"""
    v = torch.zeros(coef.shape[:-1] + (64,), dtype=torch.float32, device=coef.device)          # +0
    for k in range(nk):
        v = fma32(coef[..., k0 + k:k0 + k + 1], w[k], v)
    return v
