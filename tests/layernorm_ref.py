"""Float64 restatement of layer norm's double backward: what csrc/bhg_layernorm.hip (bhg_layernorm_backward_vjp) and FusedLayerNorm are
held to.  Plain tensor operations in the dtype of the inputs (the tests pass float64); tests/test_layernorm_ref.py holds it to autograd's
own float64 double backward of F.layer_norm.

The layer over the last D elements of M rows: xh = (x - mean) * rstd, y = gamma * xh + beta.  Its first backward is
    F : (x, gy, gamma) -> (gx, ggamma, gbeta)       g = gamma * gy, gx = rstd * (g - mean g - xh * mean(g * xh))
and for cotangents a (of gx), b (of ggamma), c (of gbeta) — any of them None = absent = zero — this returns
    (dx, dgy, dgamma) = d( <a, gx> + <b, ggamma> + <c, gbeta> ) / d(x, gy, gamma)
with mean and rstd (one per row, as given: the kernel's tests hand in the fp32 statistics the kernel itself read) treated as the
functions of x they are.  gamma None (elementwise_affine = False): gamma = 1 and dgamma is None."""
import torch


def stats(x, eps):
    """(mean, rstd) per row of the [M, D] tensor x, as the forward saves them (biased variance)."""
    mean = x.mean(dim=1)
    var = ((x - mean[:, None]) ** 2).mean(dim=1)
    return mean, 1.0 / torch.sqrt(var + eps)


def _terms(x, gy, a, gamma, mean, rstd):
    """xh, r, the centred cotangent at = a - mean a - xh mean(a xh), and the two row means it is made of."""
    r = rstd[:, None]
    xh = (x - mean[:, None]) * r
    a = torch.zeros_like(x) if a is None else a
    A0 = a.mean(dim=1, keepdim=True)
    A1 = (a * xh).mean(dim=1, keepdim=True)
    return xh, r, a, a - A0 - xh * A1, A0, A1


def layernorm_backward_vjp(x, gy, a, gamma, mean, rstd, b, c):
    """x, gy, a: [M, D]; gamma, b, c: [D]; mean, rstd: [M].  Returns (dx, dgy, dgamma)."""
    xh, r, a, at, A0, A1 = _terms(x, gy, a, gamma, mean, rstd)
    g = gy if gamma is None else gamma[None, :] * gy
    m1 = g.mean(dim=1, keepdim=True)
    m2 = (g * xh).mean(dim=1, keepdim=True)
    dgy = r * at if gamma is None else gamma[None, :] * r * at
    q = -r * (g * A1 + m2 * a)
    if b is not None:
        dgy = dgy + b[None, :] * xh
        q = q + b[None, :] * gy
    if c is not None:
        dgy = dgy + c[None, :]
    t = r * ((a * g).mean(dim=1, keepdim=True) - m1 * A0 - m2 * A1)
    dx = r * (q - q.mean(dim=1, keepdim=True) - xh * (q * xh).mean(dim=1, keepdim=True)) - r * xh * t
    dgamma = None if gamma is None else (gy * r * at).sum(dim=0)
    return dx, dgy, dgamma


def dgamma_abs_terms(x, gy, a, gamma, mean, rstd):
    """sum_i |gy_ij r_i at_ij| per column: the scale of dgamma's rounding error (cancellation in a column does not shrink it)."""
    _, r, _, at, _, _ = _terms(x, gy, a, gamma, mean, rstd)
    return (gy * r * at).abs().sum(dim=0)
