"""Float64 restatement of RMS norm's double backward: what csrc/bhg_rmsnorm.hip (bhg_rmsnorm_backward_vjp) and FusedRMSNorm are held to.
Plain tensor operations in the dtype of the inputs (the tests pass float64); tests/test_rmsnorm_ref.py holds it to autograd's own float64
double backward of F.rms_norm.

x is [M, D] (or anything whose trailing dimensions make up D, with rstd holding one value per row): r = rstd = rsqrt(mean_j x^2 + eps),
xh = x * r, y = gamma * xh.  The first backward is
    F : (x, gy, gamma) -> (gx, ggamma)       g = gamma * gy, m2 = mean(g * xh), gx = r * (g - xh * m2), ggamma_j = sum_i gy_ij xh_ij
(means over the row) and for cotangents a (of gx) and b (of ggamma) — either None = absent = zero — rmsnorm_backward_vjp returns
    (dx, dgy, dgamma) = d( <a, gx> + <b, ggamma> ) / d(x, gy, gamma)
with rstd ([M], as given: the kernel's tests hand in the fp32 statistic the kernel itself read) treated as the function of x it is.
gamma None (elementwise_affine = False): gamma = 1, no b exists and dgamma is None.  mean xh^2 = 1 is NOT used: it is 1 - eps r^2.

The two gate scales are the sums of the ABSOLUTE terms of dx / dgy (per element) and of dgamma (per column): what a rounding error is
proportional to where the result itself is a difference of nearly equal terms (a one-element row: 1 - xh^2 = eps r^2)."""
import torch


def stats(x, eps=None):
    """rstd, [M], of the [M, D] tensor x, as the forward saves it; eps None: torch.finfo(x.dtype).eps, as torch does."""
    if eps is None:
        eps = torch.finfo(x.dtype).eps
    return torch.rsqrt((x * x).mean(dim=1) + eps)


def _rows(t, M):
    return t.reshape(M, -1)


def _spread(p, M):
    return p.reshape(1, -1)


def rmsnorm_first_backward(x, gy, gamma, rstd):
    """(gx, ggamma): gx shaped like x, ggamma like gamma (None when gamma is)."""
    M = rstd.numel()
    xr, gyr, r = _rows(x, M), _rows(gy, M), rstd.reshape(M, 1)
    xh = xr * r
    g = gyr if gamma is None else _spread(gamma, M) * gyr
    m2 = (g * xh).mean(dim=1, keepdim=True)
    gx = r * (g - xh * m2)
    gg = None if gamma is None else (gyr * xh).sum(dim=0).reshape(gamma.shape)
    return gx.reshape(x.shape), gg


def _terms(x, gy, a, gamma, rstd, b):
    M = rstd.numel()
    xr, gyr, r = _rows(x, M), _rows(gy, M), rstd.reshape(M, 1)
    xh = xr * r
    ar = torch.zeros_like(xr) if a is None else _rows(a, M)
    gm = torch.ones_like(xr[:1]) if gamma is None else _spread(gamma, M)
    bb = torch.zeros_like(xr[:1]) if (b is None or gamma is None) else _spread(b, M)
    g = gm * gyr
    m2 = (g * xh).mean(dim=1, keepdim=True)
    A1 = (ar * xh).mean(dim=1, keepdim=True)
    Sag = (ar * g).mean(dim=1, keepdim=True)
    B1 = (bb * gyr * xh).mean(dim=1, keepdim=True)
    return xh, gyr, r, ar, gm, bb, g, m2, A1, Sag, B1


def rmsnorm_backward_vjp(x, gy, a, gamma, rstd, b):
    """x, gy, a: [M, D] (a may be None); gamma, b: [D] (may be None); rstd: [M].  Returns (dx, dgy, dgamma), shaped like x, x and gamma."""
    xh, gyr, r, ar, gm, bb, g, m2, A1, Sag, B1 = _terms(x, gy, a, gamma, rstd, b)
    at = ar - xh * A1
    dgy = gm * r * at + bb * xh
    q = -r * (g * A1 + m2 * ar) + bb * gyr
    t = r * (Sag - m2 * A1)
    mqx = -2.0 * r * m2 * A1 + B1
    dx = r * (q - xh * mqx) - r * xh * t
    dgamma = None if gamma is None else (gyr * r * at).sum(dim=0).reshape(gamma.shape)
    return dx.reshape(x.shape), dgy.reshape(x.shape), dgamma


def elementwise_abs_terms(x, gy, a, gamma, rstd, b):
    """(dx's, dgy's) sums of absolute terms, [M, D] each: r (|q| + |xh mqx| + |xh t|) and |gamma r| (|a| + |xh A1|) + |b xh|."""
    xh, gyr, r, ar, gm, bb, g, m2, A1, Sag, B1 = _terms(x, gy, a, gamma, rstd, b)
    q = -r * (g * A1 + m2 * ar) + bb * gyr
    t = r * (Sag - m2 * A1)
    mqx = -2.0 * r * m2 * A1 + B1
    sdx = r * (q.abs() + (xh * mqx).abs() + (xh * t).abs())
    sdgy = (gm * r).abs() * (ar.abs() + (xh * A1).abs()) + (bb * xh).abs()
    return sdx, sdgy


def dgamma_abs_terms(x, gy, a, rstd):
    """sum_i |gy r| (|a| + |xh A1|) per column: the scale of dgamma's rounding error (cancellation in a column does not shrink it)."""
    M = rstd.numel()
    xr, gyr, r = _rows(x, M), _rows(gy, M), rstd.reshape(M, 1)
    xh = xr * r
    ar = torch.zeros_like(xr) if a is None else _rows(a, M)
    A1 = (ar * xh).mean(dim=1, keepdim=True)
    return ((gyr * r).abs() * (ar.abs() + (xh * A1).abs())).sum(dim=0)
