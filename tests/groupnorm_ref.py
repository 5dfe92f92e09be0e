"""Float64 restatement of group norm's double backward: what csrc/bhg_groupnorm.hip (bhg_groupnorm_backward_vjp) and FusedGroupNorm are
held to.  Plain tensor operations in the dtype of the inputs (the tests pass float64); tests/test_groupnorm_ref.py holds it to autograd's
own float64 double backward of F.group_norm.

x is [N, C, *spatial], HW = prod(spatial), G | C, Cg = C / G.  Row (n, g) is the D = Cg * HW contiguous elements of the channels
g * Cg .. g * Cg + Cg - 1: xh = (x - mean_ng) * rstd_ng, y = gamma_ch * xh + beta_ch.  The first backward is
    F : (x, gy, gamma) -> (gx, ggamma, gbeta)       g = gamma_ch * gy, gx = rstd * (g - mean g - xh * mean(g * xh))
(means over the row) and for cotangents a (of gx), b (of ggamma), c (of gbeta) — any of them None = absent = zero — this returns
    (dx, dgy, dgamma) = d( <a, gx> + <b, ggamma> + <c, gbeta> ) / d(x, gy, gamma)
with mean and rstd ([N, G], as given: the kernel's tests hand in the fp32 statistics the kernel itself read) treated as the functions of
x they are.  gamma None (affine = False): gamma = 1 and dgamma is None."""
import torch


def _rows(t, N, G):
    return t.reshape(N, G, -1)


def stats(x, G, eps):
    """(mean, rstd), each [N, G], of the [N, C, *spatial] tensor x, as the forward saves them (biased variance)."""
    r = _rows(x, x.shape[0], G)
    mean = r.mean(dim=2)
    var = ((r - mean[:, :, None]) ** 2).mean(dim=2)
    return mean, 1.0 / torch.sqrt(var + eps)


def _per_channel(p, N, C, G, HW):
    """The [C] parameter p spread over the rows: [N, G, D]."""
    return p.reshape(1, C, 1).expand(N, C, HW).reshape(N, G, -1)


def _terms(x, a, mean, rstd, G):
    """xh, r, a, the centred cotangent at = a - mean a - xh mean(a xh), and the two row means it is made of: all [N, G, D] / [N, G, 1]."""
    N = x.shape[0]
    r = rstd.reshape(N, G, 1)
    xh = (_rows(x, N, G) - mean.reshape(N, G, 1)) * r
    a = torch.zeros_like(xh) if a is None else _rows(a, N, G)
    A0 = a.mean(dim=2, keepdim=True)
    A1 = (a * xh).mean(dim=2, keepdim=True)
    return xh, r, a, a - A0 - xh * A1, A0, A1


def groupnorm_backward_vjp(x, gy, a, gamma, mean, rstd, b, c, G):
    """x, gy, a: [N, C, *spatial]; gamma, b, c: [C]; mean, rstd: [N, G].  Returns (dx, dgy, dgamma), shaped like x, x and gamma."""
    N, C = x.shape[0], x.shape[1]
    HW = x.numel() // (N * C)
    xh, r, a, at, A0, A1 = _terms(x, a, mean, rstd, G)
    gy = _rows(gy, N, G)
    spread = lambda p: _per_channel(p, N, C, G, HW)   # noqa: E731
    g = gy if gamma is None else spread(gamma) * gy
    m1 = g.mean(dim=2, keepdim=True)
    m2 = (g * xh).mean(dim=2, keepdim=True)
    dgy = r * at if gamma is None else spread(gamma) * r * at
    q = -r * (g * A1 + m2 * a)
    if b is not None:
        dgy = dgy + spread(b) * xh
        q = q + spread(b) * gy
    if c is not None:
        dgy = dgy + spread(c)
    t = r * ((a * g).mean(dim=2, keepdim=True) - m1 * A0 - m2 * A1)
    dx = r * (q - q.mean(dim=2, keepdim=True) - xh * (q * xh).mean(dim=2, keepdim=True)) - r * xh * t
    dgamma = None if gamma is None else (gy * r * at).reshape(N, C, HW).sum(dim=(0, 2))
    return dx.reshape(x.shape), dgy.reshape(x.shape), dgamma


def dgamma_abs_terms(x, gy, a, mean, rstd, G):
    """sum_{n,hw} |gy r at| per channel: the scale of dgamma's rounding error (cancellation in a channel does not shrink it)."""
    N, C = x.shape[0], x.shape[1]
    _, r, _, at, _, _ = _terms(x, a, mean, rstd, G)
    return (_rows(gy, N, G) * r * at).abs().reshape(N, C, -1).sum(dim=(0, 2))
