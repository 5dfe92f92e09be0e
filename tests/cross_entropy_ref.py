"""Float64 restatement of cross-entropy's double backward: what csrc/bhg_cross_entropy.hip (bhg_cross_entropy_backward_vjp) and the
declared cross_entropy are held to.  Plain tensor operations in the dtype of the inputs (the tests pass float64);
tests/test_cross_entropy_ref.py holds it to autograd's own float64 double backward of F.cross_entropy.

Per row i of the [N, C] logits: lsm_i = log_softmax(z_i) — as given: the kernel's tests hand in the fp32 tensor the kernel itself
reads — P = exp(lsm), target y_i, m_i = [y_i != ignore_index and 0 <= y_i < C] (a target outside [0, C) counts as ignored: the kernel
must never index with it).  The first backward is
    F : (z, g) -> gz        gz_ic = g_i m_i (P_ic - [c = y_i])
where g_i is the gradient that reaches row i's loss: g is [N] (reduction "none"), or one element (a 0-dim or one-element tensor:
"sum", and "mean" with denom = sum m, which divides g going in).  For the cotangent a of gz, with s_i = sum_c P_ic a_ic,
    dz_ic = g_i m_i P_ic (a_ic - s_i)        dg_i = m_i (s_i - a_{i, y_i})
and for a one-element g, dg = sum_i dg_i, divided by denom where one is given.  y is not differentiable; dz has no one-hot term.

The gate scales are sums of ABSOLUTE terms: a confident row (P nearly one-hot) makes a_k - s a difference of nearly equal terms."""
import torch


def valid(y, C, ignore_index=-100):
    """m, [N] bool."""
    return (y != ignore_index) & (y >= 0) & (y < C)


def _split_g(g, N, denom, scalar_g):
    if scalar_g is None:
        scalar_g = g.dim() == 0
    gi = g.reshape(-1)
    if scalar_g:
        assert gi.numel() == 1
        gi = gi.expand(N)
        if denom is not None:
            gi = gi / denom.reshape(())
    else:
        assert gi.numel() == N and denom is None
    return gi.reshape(N, 1), scalar_g


def _pick(a, y, m):
    """a_{i, y_i}, [N], zero where the row is ignored (never indexed with an invalid target)."""
    idx = torch.where(m, y, torch.zeros_like(y)).reshape(-1, 1)
    return torch.where(m, a.gather(1, idx).reshape(-1), torch.zeros_like(a[:, 0]))


def cross_entropy_first_backward(lsm, y, g, ignore_index=-100, denom=None, scalar_g=None):
    """gz, [N, C]."""
    N, C = lsm.shape
    m = valid(y, C, ignore_index)
    gi, _ = _split_g(g, N, denom, scalar_g)
    P = torch.exp(lsm)
    onehot = torch.zeros_like(P)
    onehot.scatter_(1, torch.where(m, y, torch.zeros_like(y)).reshape(-1, 1), 1.0)
    return torch.where(m.reshape(N, 1), gi * (P - onehot), torch.zeros_like(P))


def cross_entropy_backward_vjp(lsm, y, g, a, ignore_index=-100, denom=None, scalar_g=None):
    """lsm, a: [N, C]; y: [N] int64; g: [N], or one element (0-dim, or pass scalar_g=True); denom: one element or None (only with a
    one-element g).  Returns (dz [N, C], dg shaped like g).  Ignored rows of dz and dg are exact zeros whatever lsm and a hold."""
    N, C = lsm.shape
    m = valid(y, C, ignore_index)
    gi, scalar = _split_g(g, N, denom, scalar_g)
    mc = m.reshape(N, 1)
    P = torch.where(mc, torch.exp(lsm), torch.zeros_like(lsm))
    ar = torch.where(mc, a, torch.zeros_like(a))
    s = (P * ar).sum(dim=1, keepdim=True)
    dz = torch.where(mc, gi * P * (ar - s), torch.zeros_like(P))
    dgi = torch.where(m, s.reshape(N) - _pick(ar, y, m), torch.zeros_like(s.reshape(N)))
    if scalar:
        dg = dgi.sum()
        if denom is not None:
            dg = dg / denom.reshape(())
        dg = dg.reshape(g.shape)
    else:
        dg = dgi.reshape(g.shape)
    return dz, dg


def gate_scales(lsm, y, g, a, ignore_index=-100, denom=None, scalar_g=None):
    """(dz's scale per row, dg's scale per row or as one number), sums of absolute terms:
    dz, per row: |g_i| max_c P_ic (|a_ic| + sum_c' P_ic' |a_ic'|);   dg, per row: sum_c P_ic |a_ic| + |a_{i, y_i}|;
    a one-element dg: the sum of the per-row scales, divided by denom where one is given.  Zero for ignored rows."""
    N, C = lsm.shape
    m = valid(y, C, ignore_index)
    gi, scalar = _split_g(g, N, denom, scalar_g)
    mc = m.reshape(N, 1)
    P = torch.where(mc, torch.exp(lsm), torch.zeros_like(lsm))
    aa = torch.where(mc, a, torch.zeros_like(a)).abs()
    sa = (P * aa).sum(dim=1, keepdim=True)
    sdz = gi.abs().reshape(N) * (P * (aa + sa)).amax(dim=1)
    sdz = torch.where(m, sdz, torch.zeros_like(sdz))
    sdg = torch.where(m, sa.reshape(N) + _pick(aa, y, m), torch.zeros_like(sdz))
    if scalar:
        sdg = sdg.sum()
        if denom is not None:
            sdg = sdg / denom.reshape(()).abs()
    return sdz, sdg
