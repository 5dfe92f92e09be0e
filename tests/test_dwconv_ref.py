"""tests/dwconv_ref.py — the float64 restatement the depthwise-convolution kernels (csrc/bhg_dwconv.hip) are held to — against autograd's
own double backward of F.conv2d(groups=C) in float64, over the whole geometry family: k in {3, 5, 7} x stride in {1, 2} x dilation in
{1, 2} x three paddings (none, half, full) x four shapes.  Gate: max|got - want| <= 1e-10 max|want| per array; observed: 1.8e-15 of max|want| at worst (the test prints it per k)."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import dwconv_ref

SHAPES = [(2, 3, 13, 14), (1, 1, 15, 13), (3, 2, 16, 16), (2, 5, 14, 19)]   # every extent >= 13 = 2 * (7 - 1) + 1: no empty output at pad 0
GATE = 1e-10


def _autograd(x, w, gy, a, b, stride, pad, dil):
    x, w, gy = (t.clone().requires_grad_(True) for t in (x, w, gy))
    y = F.conv2d(x, w, None, stride, pad, dil, w.shape[0])
    gx, gw = torch.autograd.grad(y, (x, w), gy, create_graph=True)
    phi = (gx * a).sum() + (gw * b).sum()
    return torch.autograd.grad(phi, (x, w, gy))


@pytest.mark.parametrize("k", [3, 5, 7])
def test_restatement_matches_autograds_double_backward_fp64(k):
    worst = 0.0
    for stride, dil, shape in itertools.product((1, 2), (1, 2), SHAPES):
        for pad in (0, dil * (k - 1) // 2, dil * (k - 1)):
            N, C, H, W = shape
            g = torch.Generator().manual_seed(((k * 7 + stride) * 7 + dil) * 101 + pad + H * W)
            Ho, Wo = dwconv_ref.out_extent(H, k, stride, pad, dil), dwconv_ref.out_extent(W, k, stride, pad, dil)
            assert Ho >= 1 and Wo >= 1
            x, a = (torch.randn(shape, generator=g, dtype=torch.float64) for _ in range(2))
            w, b = (torch.randn(C, 1, k, k, generator=g, dtype=torch.float64) for _ in range(2))
            gy = torch.randn(N, C, Ho, Wo, generator=g, dtype=torch.float64)
            want = _autograd(x, w, gy, a, b, stride, pad, dil)
            got = dwconv_ref.dwconv_backward_vjp(x, w, gy, a, b, stride, pad, dil)
            for name, u, v in zip(("dx", "dw", "dgy"), got, want):
                err = float((u - v).abs().max()) / float(v.abs().max())
                worst = max(worst, err)
                assert err <= GATE, (name, k, stride, dil, pad, shape, err)
    print(f"dwconv_ref vs autograd's double backward, k = {k}: worst max|diff| / max|want| = {worst:.2e}")


def test_absent_cotangents_are_zeros():
    g = torch.Generator().manual_seed(0)
    x, a = (torch.randn(2, 3, 9, 8, generator=g, dtype=torch.float64) for _ in range(2))
    w, b = (torch.randn(3, 1, 3, 3, generator=g, dtype=torch.float64) for _ in range(2))
    gy = torch.randn(2, 3, 5, 4, generator=g, dtype=torch.float64)
    full = dwconv_ref.dwconv_backward_vjp(x, w, gy, a, b, 2, 1, 1)
    no_a = dwconv_ref.dwconv_backward_vjp(x, w, gy, None, b, 2, 1, 1)
    no_b = dwconv_ref.dwconv_backward_vjp(x, w, gy, a, None, 2, 1, 1)
    assert not no_a[1].any() and not no_b[0].any()
    torch.testing.assert_close(no_a[0], full[0], rtol=0, atol=0)
    torch.testing.assert_close(no_b[1], full[1], rtol=0, atol=0)
    torch.testing.assert_close(no_a[2] + no_b[2], full[2], rtol=1e-13, atol=1e-13)
    assert dwconv_ref.dwconv_backward_vjp(x, w, gy, a, b, 2, 1, 1, need_dx=False, need_dw=False)[:2] == (None, None)
